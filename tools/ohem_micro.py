"""Timing of the OHEM cross entropy, forward + backward from the low-resolution class scores (19 classes, pitch 32), three ways in one
process, alternating, after a warm-up of every shape, with device events over windows of >= 300 ms.

  (a) plain   ops.upsample_cross_entropy: the fused cross entropy without mining (the floor: OHEM adds its selection to this)
  (b) ohem    ops.upsample_ohem_cross_entropy(thresh 0.7, min_kept 100 000): probability plane, radix select, masked target, then (a)
  (c) stock   what a caller's OHEM module gets on the stock path: ops.upsample_bilinear -> .float() -> softmax -> sort of every
              probability -> masked F.cross_entropy, backward through all of it (no host branch: the stock module adds one)

at 16 x 192 x 192 -> 768 x 768 in bfloat16 and 1 x 256 x 512 -> 1024 x 2048 in bfloat16 and float32.  The scores are 2.5 * randn + 3 on
the true class (a trained head: most pixels easy), so the run is in the thresh regime; `kth` repeats (b) with thresh 0, where every
select pass runs.

    python tools/ohem_micro.py [rounds]       # one JSON line
    python tools/ohem_micro.py --split [n]    # n calls of ops.ohem_target per case and regime, nothing else: for a kernel trace"""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import _lib, ops  # noqa: E402

C, PITCH, THRESH, MIN_KEPT = 19, 32, 0.7, 100000
SHAPES = [((16, 192, 192, 768, 768), torch.bfloat16), ((1, 256, 512, 1024, 2048), torch.bfloat16), ((1, 256, 512, 1024, 2048), torch.float32)]
WINDOW_MS = 300.0


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per call


def stock(P, y, size):
    """the chain the fused form replaces, with the rule's selection written in stock torch on the device"""
    logits = ops.upsample_bilinear(P, size, channels=C).float()
    valid = y != 255
    t = torch.where(valid, y, torch.zeros_like(y))
    p = torch.softmax(logits.detach(), 1).gather(1, t[:, None])[:, 0]
    p = torch.where(valid, p, torch.full_like(p, 2.0)).reshape(-1)
    q = torch.sort(p).values[MIN_KEPT - 1]
    theta = torch.clamp(q, min=THRESH)
    masked = torch.where(valid & (p.view_as(y) <= theta), y, torch.full_like(y, 255))
    return F.cross_entropy(logits, masked, ignore_index=255)


def make(shape, dtype, g, dev):
    B, Hi, Wi, H, W = shape
    y = torch.randint(0, C, (B, H, W), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.1] = 255
    low = F.interpolate(y[:, None].float(), size=(Hi, Wi), mode="nearest")[:, 0].long()
    P = torch.zeros(B, Hi, Wi, PITCH)
    P[..., :C] = torch.randn(B, Hi, Wi, C, generator=g) * 2.5 + 3.0 * F.one_hot(low.clamp(max=C - 1), C) * (low != 255)[..., None]
    return P.to(dev, dtype).permute(0, 3, 1, 2).requires_grad_(True), y.to(dev)


def micro(rounds):
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    cases = []
    for shape, dtype in SHAPES:
        P, y = make(shape, dtype, g, dev)
        s = shape[3:]

        def fb(f, P=P):
            P.grad = None
            f().backward()
        fns = {
            "plain": lambda P=P, y=y, s=s: fb(lambda: ops.upsample_cross_entropy(P, y, s, C)),
            "ohem": lambda P=P, y=y, s=s: fb(lambda: ops.upsample_ohem_cross_entropy(P, y, s, C, thresh=THRESH, min_kept=MIN_KEPT)),
            "kth": lambda P=P, y=y, s=s: fb(lambda: ops.upsample_ohem_cross_entropy(P, y, s, C, thresh=0.0, min_kept=MIN_KEPT)),
            "select": lambda P=P, y=y, s=s: ops.ohem_target(P, y, 255, THRESH, MIN_KEPT, size=s, channels=C),
            "stock": lambda P=P, y=y, s=s: fb(lambda: stock(P, y, s)),
        }
        state = ops.ohem_target(P, y, 255, THRESH, MIN_KEPT, size=s, channels=C, want_state=True)[1].tolist()
        cases.append((shape, dtype, fns, state))
    reps = {}
    for i, (shape, dtype, fns, _) in enumerate(cases):                         # warm-up of every shape, and the window lengths
        for k, fn in fns.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            reps[(i, k)] = max(5, int(WINDOW_MS * 1e3 / window(fn, 5)) + 1)
    out = []
    for i, (shape, dtype, fns, state) in enumerate(cases):
        t = {k: [] for k in fns}
        for _ in range(rounds):                                                # alternating
            for k, fn in fns.items():
                t[k].append(window(fn, reps[(i, k)]))
        npix = shape[0] * shape[3] * shape[4]
        row = {"shape": list(shape), "dtype": str(dtype).replace("torch.", ""), "valid": state[0], "kept": state[1], "mode": state[3],
               "extra_MB": round(npix * (4 + 8) / 1e6, 1), "stock_fp32_logits_MB": round(npix * C * 4 / 1e6, 1)}
        for k in fns:
            v = sorted(t[k])
            row[k] = {"us": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1), "reps": reps[(i, k)]}
        row["stock_over_ohem"] = round(row["stock"]["us"] / row["ohem"]["us"], 2)
        out.append(row)
    print(json.dumps({"op": "OHEM cross entropy, forward + backward from low-resolution scores", "classes": C, "pitch": PITCH,
                      "thresh": THRESH, "min_kept": MIN_KEPT, "device": torch.cuda.get_device_name(0), "rounds": rounds,
                      "window_ms": WINDOW_MS, "cases": out}))


def split(n):
    g = torch.Generator().manual_seed(0)
    for shape, dtype in SHAPES:
        P, y = make(shape, dtype, g, "cuda:0")
        for thresh in (THRESH, 0.0):
            for _ in range(n):
                ops.ohem_target(P, y, 255, thresh, MIN_KEPT, size=shape[3:], channels=C)
        torch.cuda.synchronize()


def main():
    if not torch.cuda.is_available():
        raise _lib.MrfpHipError("ohem_micro measures on the GPU: no device found")
    if "--split" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--split"]
        return split(int(rest[0]) if rest else 20)
    micro(int(sys.argv[1]) if len(sys.argv) > 1 else 5)


if __name__ == "__main__":
    main()
