"""Timing of the loss at the benchmark head shape: 16 x 19 (pitch 32) x 192 x 192 class scores -> 768 x 768 labels, bf16, forward +
backward (device events around `reps` calls after a warm-up, median of `rounds` windows).

  (a) plain       ops.upsample_cross_entropy as the default step calls it
  (b) weighted    the same with class weights [19]
  (c) weighted + label smoothing 0.1
  (d) per-image   loss.ImageBasedCrossEntropyLoss2d's work on the fused kernel: ops.label_class_weights (histogram) + per-image mean
  (e) stock       criterion(ops.upsample_bilinear(scores, size, channels=19).float(), labels) with nn.CrossEntropyLoss(weight=...):
                  what a weighted criterion cost before the fused kernels took it
  (f) soft-NLL    ops.upsample_soft_nll on relaxed words made once (border 1), shared class weights: the loss kernels alone, beside (a)
  (g) relaxed criterion   loss.ImgWtLossSoftNLL's work per step: ops.relax_labels with counts + ops.relaxed_class_weights + (f)
  and ops.relax_labels alone, with its achieved bytes/s against the 12 B per pixel the algorithm needs (8 read, 4 written)

    python tools/loss_micro.py [B low size reps rounds]"""
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import _lib, ops  # noqa: E402


def timed(fn, reps, rounds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    a = [int(v) for v in sys.argv[1:]]
    B, low, size, reps, rounds = (a + [16, 192, 768, 20, 7][len(a):])[:5]
    if not torch.cuda.is_available():
        raise _lib.MrfpHipError("loss_micro measures on the GPU: no device found")
    C, pitch = 19, 32
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    P = torch.zeros(B, pitch, low, low)
    P[:, :C] = torch.randn(B, C, low, low, generator=g) * 2
    P = P.to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = torch.randint(0, C, (B, size, size), generator=g)
    y[torch.rand(B, size, size, generator=g) < 0.1] = 255
    y = y.to(dev)
    w = (torch.rand(C, generator=g) + 0.5).to(dev)
    stock = nn.CrossEntropyLoss(weight=w, ignore_index=255)

    def step(loss_fn):
        def run():
            P.grad = None
            loss_fn().backward()
        return run

    def per_image():
        W = ops.label_class_weights(y, C)
        return ops.upsample_cross_entropy(P, y, (size, size), C, 255, weight=W, per_image=True)

    words = ops.relax_labels(y, C, 1)

    def relaxed_criterion():
        wd, counts = ops.relax_labels(y, C, 1, want_counts=True)
        return ops.upsample_soft_nll(P, wd, (size, size), C, weight=ops.relaxed_class_weights(counts))

    cases = [
        ("a_plain", lambda: ops.upsample_cross_entropy(P, y, (size, size), C, 255)),
        ("b_weighted", lambda: ops.upsample_cross_entropy(P, y, (size, size), C, 255, weight=w)),
        ("c_weighted_smoothed", lambda: ops.upsample_cross_entropy(P, y, (size, size), C, 255, weight=w, label_smoothing=0.1)),
        ("d_per_image_with_histogram", per_image),
        ("e_stock_upsample_float_criterion", lambda: stock(ops.upsample_bilinear(P, (size, size), channels=C).float(), y)),
        ("f_soft_nll", lambda: ops.upsample_soft_nll(P, words, (size, size), C, weight=w)),
        ("g_relaxed_criterion", relaxed_criterion),
    ]
    res = {}
    for name, fn in cases:
        med, lo, hi = timed(step(fn), reps, rounds)
        res[name] = {"us_fwd_bwd": round(med, 1), "min": round(lo, 1), "max": round(hi, 1)}
    res["hist_only_us"] = round(timed(lambda: ops.label_class_weights(y, C), reps, rounds)[0], 1)
    for name, fn in (("relax_labels", lambda: ops.relax_labels(y, C, 1)), ("relax_labels_with_counts", lambda: ops.relax_labels(y, C, 1, want_counts=True))):
        med, lo, hi = timed(fn, reps, rounds)
        res[name] = {"us": round(med, 1), "min": round(lo, 1), "max": round(hi, 1),
                     "algorithmic_GBps": round(12.0 * B * size * size / (med * 1e-6) / 1e9, 1)}
    print(json.dumps({"op": "loss forward + backward", "scores": [B, C, pitch, low, low], "labels": [B, size, size], "dtype": "bfloat16",
                      "device": torch.cuda.get_device_name(0), "reps": reps, "rounds": rounds,
                      "b_over_a": round(res["b_weighted"]["us_fwd_bwd"] / res["a_plain"]["us_fwd_bwd"], 3),
                      "f_over_a": round(res["f_soft_nll"]["us_fwd_bwd"] / res["a_plain"]["us_fwd_bwd"], 3), **res}))


if __name__ == "__main__":
    main()
