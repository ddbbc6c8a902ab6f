"""Timing of the focal and soft Dice losses, forward + backward from the low-resolution class scores (19 classes, pitch 32, bfloat16),
fused operators against the stock chain in one process, alternating, after a warm-up of every shape, with device events over
windows of >= 300 ms.

  ce          ops.upsample_cross_entropy: the existing fused cross entropy (the floor: every fused loss moves the same tensors)
  focal       ops.upsample_focal_loss(gamma 2)
  dice        ops.upsample_region_loss(kind 'dice')
  ce_dice     loss.SumLoss(CE, 0.5 * RegionLoss2d()).fused: the two fused losses and the sum
  stock_*     what a caller's module gets on the stock path: ops.upsample_bilinear -> .float() -> softmax / log_softmax -> the torch
              formula, backward through all of it

at 16 x 192 x 192 -> 768 x 768 and 1 x 256 x 512 -> 1024 x 2048.  `traffic_MB` is what one fused forward + backward has to move: the
scores once per pass (forward, backward), the int64 labels once per pass, d(logits) at pitch 24 written by the loss backward and
read by the bilinear backward, d(scores) written; `GBps` is that over the measured time, to set against ~6.3 TB/s of HBM.

    python tools/region_loss_micro.py [rounds]       # one JSON line"""
import json
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import _lib, loss, ops  # noqa: E402

C, PITCH, CD, GAMMA, LAMBDA = 19, 32, 24, 2.0, 0.5
SHAPES = [(16, 192, 192, 768, 768), (1, 256, 512, 1024, 2048)]
DTYPE = torch.bfloat16
WINDOW_MS = 300.0


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per call


def _stock_parts(P, y, size):
    logits = ops.upsample_bilinear(P, size, channels=C).float()
    valid = y != 255
    t = torch.where(valid, y, torch.zeros_like(y))
    return logits, valid, t


def stock_focal(P, y, size):
    logits, valid, t = _stock_parts(P, y, size)
    lpt = F.log_softmax(logits, 1).gather(1, t[:, None])[:, 0]
    l = -((1.0 - lpt.exp()) ** GAMMA) * lpt
    return (l * valid).sum() / valid.sum()


def stock_dice(P, y, size, logits=None):
    if logits is None:
        logits, valid, t = _stock_parts(P, y, size)
    else:
        valid = y != 255
        t = torch.where(valid, y, torch.zeros_like(y))
    p = torch.softmax(logits, 1) * valid[:, None]
    oh = F.one_hot(t, C).permute(0, 3, 1, 2) * valid[:, None]
    I, Ps, T = (p * oh).sum((0, 2, 3)), p.sum((0, 2, 3)), oh.sum((0, 2, 3)).float()
    K = (T > 0).float()
    S = (2.0 * I + 1.0) / (Ps + T + 1.0)
    return (K * (1.0 - S)).sum() / K.sum()


def stock_ce_dice(P, y, size):
    logits = ops.upsample_bilinear(P, size, channels=C).float()
    return F.cross_entropy(logits, y, ignore_index=255) + LAMBDA * stock_dice(P, y, size, logits)


def make(shape, g, dev):
    B, Hi, Wi, H, W = shape
    y = torch.randint(0, C, (B, H, W), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.1] = 255
    low = F.interpolate(y[:, None].float(), size=(Hi, Wi), mode="nearest")[:, 0].long()
    P = torch.zeros(B, Hi, Wi, PITCH)
    P[..., :C] = torch.randn(B, Hi, Wi, C, generator=g) * 2.5 + 3.0 * F.one_hot(low.clamp(max=C - 1), C) * (low != 255)[..., None]
    return P.to(dev, DTYPE).permute(0, 3, 1, 2).requires_grad_(True), y.to(dev)


def micro(rounds):
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    both = loss.SumLoss((1.0, nn.CrossEntropyLoss(ignore_index=255)), (LAMBDA, loss.RegionLoss2d())).to(dev)
    cases = []
    for shape in SHAPES:
        P, y = make(shape, g, dev)
        s = shape[3:]

        def fb(f, P=P):
            P.grad = None
            f().backward()
        fns = {
            "ce": lambda P=P, y=y, s=s: fb(lambda: ops.upsample_cross_entropy(P, y, s, C)),
            "focal": lambda P=P, y=y, s=s: fb(lambda: ops.upsample_focal_loss(P, y, s, C, gamma=GAMMA)),
            "dice": lambda P=P, y=y, s=s: fb(lambda: ops.upsample_region_loss(P, y, s, C)),
            "ce_dice": lambda P=P, y=y, s=s: fb(lambda: both.fused(P, y, s, C)),
            "stock_focal": lambda P=P, y=y, s=s: fb(lambda: stock_focal(P, y, s)),
            "stock_dice": lambda P=P, y=y, s=s: fb(lambda: stock_dice(P, y, s)),
            "stock_ce_dice": lambda P=P, y=y, s=s: fb(lambda: stock_ce_dice(P, y, s)),
        }
        cases.append((shape, fns))
    reps = {}
    for i, (shape, fns) in enumerate(cases):                                   # warm-up of every shape, and the window lengths
        for k, fn in fns.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            reps[(i, k)] = max(5, int(WINDOW_MS * 1e3 / window(fn, 5)) + 1)
    out = []
    for i, (shape, fns) in enumerate(cases):
        t = {k: [] for k in fns}
        for _ in range(rounds):                                                # alternating
            for k, fn in fns.items():
                t[k].append(window(fn, reps[(i, k)]))
        B, Hi, Wi, H, W = shape
        npix, esz = B * H * W, torch.empty((), dtype=DTYPE).element_size()
        traffic = 3 * B * Hi * Wi * PITCH * esz + 2 * npix * 8 + 2 * npix * CD * esz
        row = {"shape": list(shape), "dtype": str(DTYPE).replace("torch.", ""), "traffic_MB": round(traffic / 1e6, 1),
               "stock_fp32_logits_MB": round(npix * C * 4 / 1e6, 1)}
        for k in fns:
            v = sorted(t[k])
            row[k] = {"us": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1), "reps": reps[(i, k)]}
        for k, passes in (("ce", 1), ("focal", 1), ("dice", 1), ("ce_dice", 2)):
            row[k]["GBps"] = round(passes * traffic / row[k]["us"] / 1e3, 1)
            row[k]["over_ce"] = round(row[k]["us"] / row["ce"]["us"], 2)
        for k in ("focal", "dice", "ce_dice"):
            row["stock_over_" + k] = round(row["stock_" + k]["us"] / row[k]["us"], 2)
        out.append(row)
    print(json.dumps({"op": "focal / soft Dice losses, forward + backward from low-resolution scores", "classes": C, "pitch": PITCH,
                      "gamma": GAMMA, "lambda": LAMBDA, "device": torch.cuda.get_device_name(0), "rounds": rounds,
                      "window_ms": WINDOW_MS, "cases": out}))


def main():
    if not torch.cuda.is_available():
        raise _lib.MrfpHipError("region_loss_micro measures on the GPU: no device found")
    micro(int(sys.argv[1]) if len(sys.argv) > 1 else 5)


if __name__ == "__main__":
    main()
