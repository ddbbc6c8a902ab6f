"""Cost of the checked optimiser step on the bench model's arena (ResNet-101 MRFP+, 40.35 M trainable fp32 elements): device events
around `reps` calls, the variants ALTERNATING inside every round of one process, median over `rounds` rounds after a warm-up.

  (a) sgd       mrfp_sgd_step                                   reads p, g, m; writes p, m         5 arena streams
  (b) checked   mrfp_grad_check + mrfp_sgd_step_checked         (a) + one more read of g           6 arena streams, 3 launches
  (c) check     mrfp_grad_check alone (partials + finalize)     reads g                            1 arena stream, 2 launches

The gradient is finite and the scaler static, so every checked step is applied (a skipped step would return at once and look
cheap).  Entry points are called directly: the weight re-pack that follows either step in FlatSGD.step is the same work for both.

    python tools/step_check_bench.py [reps rounds]        -> one JSON line"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import _lib, deepv3  # noqa: E402
from mrfp_amd._lib import call, ptr, stream  # noqa: E402
from mrfp_amd.harness import FlatSGD, LossScaler  # noqa: E402


def main():
    a = [int(v) for v in sys.argv[1:]]
    reps, rounds = (a + [20, 25][len(a):])[:2]
    if not torch.cuda.is_available():
        raise _lib.MrfpHipError("step_check_bench measures on the GPU: no device found")
    dev = "cuda:0"
    torch.manual_seed(0)
    model = deepv3.MRFPPlus(19, trunk="resnet-101").to(dev)
    opt = FlatSGD(model, lr=1e-4)
    n = opt.n
    scaler = LossScaler(init_scale=65536.0, dynamic=False, device=dev)
    ws = torch.empty(4 * int(_lib.lib().mrfp_grad_check_nblocks(n)), dtype=torch.float32, device=dev)
    opt.flat_g.copy_(torch.randn(n, device=dev) * 1e-3 * 65536.0)
    p, g, m, st = ptr(opt.flat_p), ptr(opt.flat_g), ptr(opt.flat_m), ptr(scaler.state)

    def sgd():
        call("mrfp_sgd_step", p, g, m, n, 1e-4, 0.9, 5e-4, 1.0 / 65536.0, 0, stream())

    def check():
        call("mrfp_grad_check", g, n, 1.0, ptr(ws), st, 0, 2.0, 0.5, 2000, 1.0, stream())

    def checked():
        check()
        call("mrfp_sgd_step_checked", p, g, m, n, 1e-4, 0.9, 5e-4, st, stream())

    variants = [("sgd", sgd, 5), ("checked", checked, 6), ("check", check, 1)]
    for _, fn, _ in variants:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(rounds):
        for name, fn, _ in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps * 1e3)
    info = scaler.info()
    assert info["skipped"] == 0 and info["found_inf"] == 0, info          # every checked step was applied
    res = {}
    for name, _, streams in variants:
        t = sorted(times[name])
        med = t[len(t) // 2]
        res[name] = {"us": round(med, 1), "min": round(t[0], 1), "max": round(t[-1], 1), "bytes": streams * 4 * n,
                     "TB_per_s": round(streams * 4 * n / med / 1e6, 2)}
    print(json.dumps({"op": "optimiser step over the flat arena", "elements": n, "device": torch.cuda.get_device_name(0),
                      "reps": reps, "rounds": rounds, "iterations_per_variant": reps * rounds,
                      "checked_over_sgd": round(res["checked"]["us"] / res["sgd"]["us"], 3), "byte_ratio": 1.2,
                      "grad_norm": info["grad_norm"], "gmul": info["gmul"], **res}))


if __name__ == "__main__":
    main()
