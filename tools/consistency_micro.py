"""Timing of the two-view consistency losses, forward + backward from two sets of low-resolution class scores (19 classes, pitch 32,
bfloat16): the fused operators against the stock chain in one process, alternating, after a warm-up of every shape, with device events
over windows of >= 300 ms (or 3 calls, whichever is longer), medians of the rounds.

  kl / hard / js1 / js2              ops.upsample_consistency_loss (js1: the gradient to the student only, js2: to both views)
  stock_kl / stock_hard / stock_js1 / stock_js2
                                     what a caller writes without it: ops.upsample_bilinear of both views -> .float() -> softmax /
                                     log_softmax -> the formula -> a mean over the counted pixels, backward through all of it
  ce                                 ops.upsample_cross_entropy of the student against the labels: the yardstick the issue names
                                     ("about the fused cross entropy per view that takes a gradient")

at 16 x 192 x 192 -> 768 x 768 and 1 x 256 x 512 -> 1024 x 2048, T = 2, threshold 0.9, valid = a label map with 10 % ignored.
`peak_bytes` is torch's peak allocation over one forward + backward above what was allocated before it.

    python tools/consistency_micro.py [rounds]       # one JSON line"""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import _lib, ops  # noqa: E402
from tools.lovasz_micro import peak  # noqa: E402
from tools.region_loss_micro import make, window  # noqa: E402

C, T, THRESHOLD = 19, 2.0, 0.9
SHAPES = [(16, 192, 192, 768, 768), (1, 256, 512, 1024, 2048)]
WINDOW_MS = 300.0


def stock(kind, Ps, Pt, y, size):
    zs = ops.upsample_bilinear(Ps, size, channels=C).float()
    zt = ops.upsample_bilinear(Pt, size, channels=C).float()
    counted = ((y >= 0) & (y < C)).float()
    n = counted.sum().clamp_min(1.0)
    if kind == "hard":
        conf, k = torch.softmax(zt.detach(), 1).max(1)
        kept = counted * (conf >= THRESHOLD).float()
        return (F.cross_entropy(zs, k, reduction="none") * kept).sum() / kept.sum().clamp_min(1.0)
    lp, lq = F.log_softmax(zs / T, 1), F.log_softmax(zt / T, 1)
    if kind == "kl":
        return T * T * (F.kl_div(lp, lq.detach(), reduction="none", log_target=True).sum(1) * counted).sum() / n
    lm = torch.logaddexp(lp, lq) - 0.6931471805599453
    js = 0.5 * ((lp.exp() * (lp - lm)).sum(1) + (lq.exp() * (lq - lm)).sum(1))
    return T * T * (js * counted).sum() / n


def micro(rounds):
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    cases = []
    for shape in SHAPES:
        Ps, y = make(shape, g, dev)
        Pt, _ = make(shape, g, dev)
        s = shape[3:]

        def fb(f, grad_t, Ps=Ps, Pt=Pt):
            Ps.grad, Pt.grad = None, None
            f(Ps, Pt if grad_t else Pt.detach()).backward()
        fns = {}
        for name, kind, grad_t in (("kl", "kl", False), ("hard", "hard", False), ("js1", "js", False), ("js2", "js", True)):
            fns[name] = lambda kind=kind, grad_t=grad_t, y=y, s=s, fb=fb: fb(
                lambda a, b: ops.upsample_consistency_loss(a, b, s, C, y, kind=kind, temperature=T, threshold=THRESHOLD), grad_t)
            fns["stock_" + name] = lambda kind=kind, grad_t=grad_t, y=y, s=s, fb=fb: fb(lambda a, b: stock(kind, a, b, y, s), grad_t)
        fns["ce"] = lambda y=y, s=s, fb=fb: fb(lambda a, b: ops.upsample_cross_entropy(a, y, s, C), False)
        cases.append((shape, fns))
    reps = {}
    for i, (shape, fns) in enumerate(cases):                                   # warm-up of every shape, and the window lengths
        for k, fn in fns.items():
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            reps[(i, k)] = max(3, int(WINDOW_MS * 1e3 / window(fn, 3)) + 1)
    out = []
    for i, (shape, fns) in enumerate(cases):
        t = {k: [] for k in fns}
        for _ in range(rounds):                                                # alternating
            for k, fn in fns.items():
                t[k].append(window(fn, reps[(i, k)]))
        B, Hi, Wi, H, W = shape
        row = {"shape": list(shape), "dtype": "bfloat16", "stock_fp32_logits_bytes_per_view": B * H * W * C * 4,
               "peak_bytes": {k: peak(fns[k]) for k in fns}}
        for k in fns:
            v = sorted(t[k])
            row[k] = {"us": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1), "reps": reps[(i, k)]}
        for k in ("kl", "hard", "js1", "js2"):
            row["stock_over_" + k] = round(row["stock_" + k]["us"] / row[k]["us"], 2)
            row[k + "_over_ce"] = round(row[k]["us"] / row["ce"]["us"], 2)
        out.append(row)
    print(json.dumps({"op": "two-view consistency losses, forward + backward from low-resolution scores", "classes": C, "temperature": T,
                      "threshold": THRESHOLD, "device": torch.cuda.get_device_name(0), "rounds": rounds, "window_ms": WINDOW_MS,
                      "cases": out}))


def main():
    if not torch.cuda.is_available():
        raise _lib.MrfpHipError("consistency_micro measures on the GPU: no device found")
    micro(int(sys.argv[1]) if len(sys.argv) > 1 else 5)


if __name__ == "__main__":
    main()
