"""One seeded train step (forward + backward of loss1 + loss2) of DeepMobileNetV3PlusD and DeepMobileNetV3PlusD_OS8 at
16 x 768^2 bf16 on synthetic weights and batch, after `--warmup` steps: ms per step (median of `--steps`, timed with a device
synchronise, no profiler) and images/s.  Prints one JSON line per factory."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import synth  # noqa: E402
from mrfp_amd.config import cfg  # noqa: E402
from mrfp_amd.network import deepv3  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    cfg.MODEL.ACT_DTYPE = torch.bfloat16
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    x, y = synth.synth_batch(a.batch, a.size, a.size, seed=1)
    x, y = x.cuda(), y.cuda()
    for name in ("DeepMobileNetV3PlusD", "DeepMobileNetV3PlusD_OS8"):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            m = getattr(deepv3, name)(None, 19, crit, crit)
        m.load_state_dict(synth.synth_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=0))
        m = m.cuda().train()
        ts = []
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            l1, l2 = m(x, gts=y)
            (l1 + l2).backward()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            m.zero_grad(set_to_none=True)
        ts = sorted(ts[a.warmup:])
        ms = ts[len(ts) // 2]
        print(json.dumps({"model": name, "batch": a.batch, "size": a.size, "dtype": "bf16", "ms_per_step": ms,
                          "images_per_s": a.batch / ms * 1e3, "steps_ms": ts, "loss": [l1.item(), l2.item()]}), flush=True)
        del m


if __name__ == "__main__":
    main()
