"""Gradient accumulation on the bench workload (ResNet-101 MRFP+, 40.35 M trainable fp32 elements): what profiles/accum.md reports.

  kernel [reps rounds]      device events around `reps` calls of each variant, the variants ALTERNATING inside every round of one
                            process, median / min / max over `rounds` rounds after a warm-up:
      accumulate   mrfp_grad_accumulate(first = 0)    reads acc, g; writes acc             3 arena streams
      copy         mrfp_grad_accumulate(first = 1)    reads g; writes acc                  2 arena streams
      sgd          mrfp_sgd_step                      reads p, g, m; writes p, m           5 arena streams (the yardstick)
  window [k steps rounds batch size]
                            Trainer.step on the bench workload (bf16, all perturbations on, HRFP re-drawn every step), host clock
                            around `steps` calls that end in a device synchronise, accum_steps = 1 and accum_steps = k ALTERNATING
                            per round on ONE trainer (the window length is changed between windows): ms per micro-batch.

    python tools/accum_micro.py kernel|window [...]        -> one JSON line"""
import contextlib
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import _lib, deepv3, synth  # noqa: E402
from mrfp_amd._lib import call, ptr, stream  # noqa: E402
from mrfp_amd.harness import FlatSGD, Trainer  # noqa: E402


def _summary(t):
    t = sorted(t)
    return {"median": t[len(t) // 2], "min": t[0], "max": t[-1]}


def kernel(reps=20, rounds=25):
    dev = "cuda:0"
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = deepv3.MRFPPlus(19, trunk="resnet-101").to(dev)
    opt = FlatSGD(model, lr=1e-4)
    n = opt.n
    opt.flat_g.copy_(torch.randn(n, device=dev) * 1e-3)
    opt.accumulate(first=True)
    p, g, m, a = ptr(opt.flat_p), ptr(opt.flat_g), ptr(opt.flat_m), ptr(opt.flat_a)
    variants = [("accumulate", lambda: call("mrfp_grad_accumulate", a, g, n, 0, stream()), 3),
                ("copy", lambda: call("mrfp_grad_accumulate", a, g, n, 1, stream()), 2),
                ("sgd", lambda: call("mrfp_sgd_step", p, g, m, n, 1e-4, 0.9, 5e-4, 1.0, 0, stream()), 5)]
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
    res = {}
    for name, _, streams in variants:
        s = _summary(times[name])
        res[name] = {"us": round(s["median"], 1), "min": round(s["min"], 1), "max": round(s["max"], 1), "bytes": streams * 4 * n,
                     "TB_per_s": round(streams * 4 * n / s["median"] / 1e6, 2),
                     "TB_per_s_range": [round(streams * 4 * n / s["max"] / 1e6, 2), round(streams * 4 * n / s["min"] / 1e6, 2)]}
    return {"op": "gradient accumulation over the flat arena", "elements": n, "device": torch.cuda.get_device_name(0), "reps": reps,
            "rounds": rounds, "accumulate_over_sgd_rate": round(res["accumulate"]["TB_per_s"] / res["sgd"]["TB_per_s"], 3), **res}


def window(k=4, steps=8, rounds=5, batch=16, size=768):
    from mrfp_amd.config import cfg
    if steps % k:
        raise ValueError("steps (%d) must be a multiple of k (%d): whole windows only" % (steps, k))
    dev = "cuda:0"
    torch.manual_seed(0)
    cfg.MODEL.ACT_DTYPE = torch.bfloat16
    with contextlib.redirect_stdout(io.StringIO()):
        model = deepv3.MRFPPlus(19, trunk="resnet-101", criterion=torch.nn.CrossEntropyLoss(ignore_index=255))
    model.load_state_dict(synth.synth_state_dict(synth.spec_of(model.state_dict()), seed=0))
    model = model.to(dev).train()
    model.rng = deepv3.InjectedRandom((True, True, True), None, reinit=True)
    tr = Trainer(model)
    x, y = synth.synth_batch(batch, size, size, seed=1)
    x, y = x.to(dev), y.to(dev)

    def run(kk, count):
        assert tr.micro == 0
        tr.accum_steps = kk                       # between windows: the position inside a window is 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            loss = tr.step(x, y)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / count, float(loss)

    for kk in (1, k):                             # warm-up: every launch of both forms, flat_a allocated
        run(kk, max(k, 4) if kk == 1 else k)
    times = {1: [], k: []}
    for _ in range(rounds):
        for kk in (1, k):
            ms, loss = run(kk, steps)
            times[kk].append(ms)
    out = {"op": "Trainer.step per micro-batch, resnet-101 MRFP+ %dx%dx%d bf16" % (batch, size, size), "k": k, "steps_per_round": steps,
           "rounds": rounds, "device": torch.cuda.get_device_name(0), "final_loss": loss, "optimiser_steps": tr.opt.it}
    for kk in (1, k):
        s = _summary(times[kk])
        out["accum_steps=%d" % kk] = {"ms_per_micro_batch": round(s["median"], 2), "min": round(s["min"], 2), "max": round(s["max"], 2),
                                      "rounds_ms": [round(v, 2) for v in times[kk]]}
    return out


def main():
    if not torch.cuda.is_available():
        raise _lib.MrfpHipError("accum_micro measures on the GPU: no device found")
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    a = [int(v) for v in sys.argv[2:]]
    if mode == "kernel":
        print(json.dumps(kernel(*a)))
    elif mode == "window":
        print(json.dumps(window(*a)))
    else:
        raise SystemExit("usage: accum_micro.py kernel [reps rounds] | window [k steps rounds batch size]")


if __name__ == "__main__":
    main()
