from mrfp_amd.network.deepv3 import *  # noqa: F401,F403
from mrfp_amd.network.deepv3 import DeepV3Plus, _AtrousSpatialPyramidPoolingModule  # noqa: F401
