"""Timing of the Lovasz-Softmax loss, forward + backward from the low-resolution class scores (19 classes, pitch 32, bfloat16): the fused
operator against the stock chain in one process, alternating, after a warm-up of every shape, with device events over windows of
>= 300 ms (or 3 calls, whichever is longer), medians of the rounds.

  lovasz        ops.upsample_lovasz_softmax: keys, stable radix sort, scan and coefficients per class group; backward + bilinear backward
  ce_lovasz     loss.SumLoss(CE, 0.5 * LovaszSoftmax2d()).fused
  stock_lovasz  what a caller's module gets on the stock path: ops.upsample_bilinear -> .float() -> softmax -> the published formula
                (per present class: errors, torch.sort descending, lovasz_grad by cumulative sums, dot), backward through all of it

at 16 x 192 x 192 -> 768 x 768 and 1 x 256 x 512 -> 1024 x 2048.  `ws_bytes` is mrfp_lovasz_ws_bytes of the shape, `out_bytes` the saved
buffer (loss, factor table, coefficient plane), `peak_bytes` torch's peak allocation over one forward + backward above what was
allocated before it, for the fused operator and for the stock chain.

    python tools/lovasz_micro.py [rounds]       # one JSON line"""
import json
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import _lib, loss, ops  # noqa: E402
from tools.region_loss_micro import make, window  # noqa: E402

C, LAMBDA = 19, 0.5
SHAPES = [(16, 192, 192, 768, 768), (1, 256, 512, 1024, 2048)]
WINDOW_MS = 300.0


def stock_lovasz(P, y, size):
    """lovasz_softmax_flat(classes='present') of the published helper over the whole batch."""
    logits = ops.upsample_bilinear(P, size, channels=C).float()
    probas = torch.softmax(logits, 1).permute(0, 2, 3, 1).reshape(-1, C)
    labels = y.reshape(-1)
    valid = labels != 255
    vp, vl = probas[valid], labels[valid]
    losses = []
    for c in range(C):
        fg = (vl == c).float()
        if fg.sum() == 0:               # (a host wait per class, as published)
            continue
        errors = (fg - vp[:, c]).abs()
        es, perm = torch.sort(errors, 0, descending=True)
        fs = fg[perm]
        gts = fs.sum()
        jac = 1.0 - (gts - fs.cumsum(0)) / (gts + (1.0 - fs).cumsum(0))
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append(torch.dot(es, jac.detach()))
    return torch.stack(losses).mean()


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def micro(rounds):
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    both = loss.SumLoss((1.0, nn.CrossEntropyLoss(ignore_index=255)), (LAMBDA, loss.LovaszSoftmax2d())).to(dev)
    L = _lib.lib()
    cases = []
    for shape in SHAPES:
        P, y = make(shape, g, dev)
        s = shape[3:]

        def fb(f, P=P):
            P.grad = None
            f().backward()
        fns = {
            "lovasz": lambda P=P, y=y, s=s: fb(lambda: ops.upsample_lovasz_softmax(P, y, s, C)),
            "ce_lovasz": lambda P=P, y=y, s=s: fb(lambda: both.fused(P, y, s, C)),
            "stock_lovasz": lambda P=P, y=y, s=s: fb(lambda: stock_lovasz(P, y, s)),
        }
        cases.append((shape, fns, (P, y, s)))
    reps = {}
    for i, (shape, fns, _) in enumerate(cases):                                # warm-up of every shape, and the window lengths
        for k, fn in fns.items():
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            reps[(i, k)] = max(3, int(WINDOW_MS * 1e3 / window(fn, 3)) + 1)
    out = []
    for i, (shape, fns, (P, y, s)) in enumerate(cases):
        t = {k: [] for k in fns}
        for _ in range(rounds):                                                # alternating
            for k, fn in fns.items():
                t[k].append(window(fn, reps[(i, k)]))
        B, Hi, Wi, H, W = shape
        row = {"shape": list(shape), "dtype": "bfloat16", "ws_bytes": int(L.mrfp_lovasz_ws_bytes(B, H * W, C, 0)),
               "out_bytes": 4 * int(L.mrfp_lovasz_out_floats(B, H * W, C, 0)), "stock_fp32_logits_bytes": B * H * W * C * 4,
               "peak_bytes": {k: peak(fns[k]) for k in ("lovasz", "stock_lovasz")}}
        for k in fns:
            v = sorted(t[k])
            row[k] = {"us": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1), "reps": reps[(i, k)]}
        row["stock_over_lovasz"] = round(row["stock_lovasz"]["us"] / row["lovasz"]["us"], 2)
        out.append(row)
    print(json.dumps({"op": "Lovasz-Softmax loss, forward + backward from low-resolution scores", "classes": C,
                      "group_classes": int(L.mrfp_lovasz_group_classes()), "sort_tile_items": int(L.mrfp_sort_tile_items()),
                      "device": torch.cuda.get_device_name(0), "rounds": rounds, "window_ms": WINDOW_MS, "cases": out}))


def main():
    if not torch.cuda.is_available():
        raise _lib.MrfpHipError("lovasz_micro measures on the GPU: no device found")
    micro(int(sys.argv[1]) if len(sys.argv) > 1 else 5)


if __name__ == "__main__":
    main()
