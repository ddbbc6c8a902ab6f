"""Weight averaging inside the fused SGD step at the ResNet-101 arena size: what profiles/weight_average.md reports.

Device events around `reps` back-to-back calls of each variant, the variants ALTERNATING inside every round of one process, median /
min / max over `rounds` rounds after a warm-up of every variant:

    sgd_a, sgd_b   mrfp_sgd_step, twice per round        reads p, g, m; writes p, m          5 arena streams (the parent's step; the
                                                                                              two slots measure the run's own noise)
    avg_update     mrfp_sgd_step_avg, t on an update     + reads e, writes e                 7 arena streams
    avg_none       mrfp_sgd_step_avg, t off the period   e untouched                         5 arena streams
    unfused        mrfp_sgd_step, then e.lerp_(p, c)     the step + (reads p, e; writes e)   8 arena streams, 2 launches

    python tools/weight_average_micro.py [elements reps rounds]        -> one JSON line

The acceptance is relative and same-run: avg_update must not be slower than unfused, and avg_none must be within the sgd_a / sgd_b
noise of mrfp_sgd_step."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import _lib  # noqa: E402
from mrfp_amd._lib import call, ptr, stream  # noqa: E402
from mrfp_amd.harness import WeightAverage, average_coefficient, average_index  # noqa: E402

ELEMENTS = 40_350_000          # the trainable fp32 elements of the ResNet-101 model, as csrc/sgd.hip counts them


def _summary(t):
    t = sorted(t)
    return {"median": t[len(t) // 2], "min": t[0], "max": t[-1]}


def measure(n=ELEMENTS, reps=20, rounds=25):
    if n <= 0 or n % 4:
        raise ValueError("elements must be a positive multiple of 4, got %r" % (n,))
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    P, G, M, E = (torch.randn(n, device=dev, generator=gen) * s for s in (1e-1, 1e-3, 1e-3, 1e-1))
    p, g, m, e = ptr(P), ptr(G), ptr(M), ptr(E)
    avg = WeightAverage("ema", decay=0.999, warmup=True, start=2, every=2)
    t_on, t_off = 20002, 20003
    assert average_index(t_on, avg.start, avg.every) == 10000 and average_index(t_off, avg.start, avg.every) is None
    c = average_coefficient("ema", 10000, avg.decay, avg.warmup)
    hyper = (1e-4, 0.9, 5e-4, 1.0, 0)

    def sgd():
        call("mrfp_sgd_step", p, g, m, n, *hyper, stream())

    def avg_step(t):
        call("mrfp_sgd_step_avg", p, g, m, e, n, *hyper, *avg.c_args(), t, stream())

    def unfused():
        sgd()
        E.lerp_(P, c)

    variants = [("sgd_a", sgd, 5), ("avg_update", lambda: avg_step(t_on), 7), ("avg_none", lambda: avg_step(t_off), 5),
                ("unfused", unfused, 8), ("sgd_b", sgd, 5)]
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
                     "TB_per_s": round(streams * 4 * n / s["median"] / 1e6, 2)}
    pair = [abs(a - b) for a, b in zip(times["sgd_a"], times["sgd_b"])]
    noise = {"sgd_a_vs_sgd_b_median_us": round(abs(res["sgd_a"]["us"] - res["sgd_b"]["us"]), 2),
             "sgd_a_vs_sgd_b_per_round_max_us": round(max(pair), 2),
             "sgd_round_spread_us": round(max(res[k]["max"] - res[k]["min"] for k in ("sgd_a", "sgd_b")), 2)}
    sgd_us = 0.5 * (res["sgd_a"]["us"] + res["sgd_b"]["us"])
    return {"op": "weight averaging inside the fused SGD step", "elements": n, "device": torch.cuda.get_device_name(0), "reps": reps,
            "rounds": rounds, **res, "noise": noise,
            "avg_update_over_sgd": round(res["avg_update"]["us"] / sgd_us, 3),
            "avg_update_minus_unfused_us": round(res["avg_update"]["us"] - res["unfused"]["us"], 1),
            "avg_none_minus_sgd_us": round(res["avg_none"]["us"] - sgd_us, 2),
            "all_finite": bool(torch.isfinite(P).all() and torch.isfinite(E).all())}


def main():
    if not torch.cuda.is_available():
        raise _lib.MrfpHipError("weight_average_micro measures on the GPU: no device found")
    print(json.dumps(measure(*[int(v) for v in sys.argv[1:]])))


if __name__ == "__main__":
    main()
