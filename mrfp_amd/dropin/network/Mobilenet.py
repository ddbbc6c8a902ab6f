from mrfp_amd.network.Mobilenet import *  # noqa: F401,F403
