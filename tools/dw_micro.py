"""Times every depthwise 3x3 launch shape of DeepMobileNetV3PlusD (OS16) and DeepMobileNetV3PlusD_OS8 at 16 x 768^2 bf16 through
the C ABI -- forward (with the fused BatchNorm statistics), dgrad, wgrad (slabs + fixed-order sum) -- and, beside each, stock
PyTorch-ROCm F.conv2d(groups=C) on a channels-last bf16 tensor of the same shape (forward, input gradient, weight gradient via
aten.convolution_backward).  Device-event timing, median of `--reps`; algorithmic bytes: fwd = read x + write y, dgrad = read dy +
write dx, wgrad = read x + read dy.  Prints one JSON line per shape and writes MRFP_OUT/dw_micro.json (default out/)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import _lib  # noqa: E402

SETTING = [[1, 16, 1, 1], [6, 24, 2, 2], [6, 32, 3, 2], [6, 64, 4, 2], [6, 96, 3, 1], [6, 160, 3, 2], [6, 320, 1, 1]]
LAYER_OF = {**{f: "layer0" for f in (0, 1)}, **{f: "layer1" for f in range(2, 7)}, **{f: "layer2" for f in range(7, 11)},
            **{f: "layer3" for f in range(11, 18)}}


def dw_shapes(S, variant):
    """(feature, C, H, W, stride, dil) of every depthwise convolution, DeepV3Plus dilation surgery applied."""
    dil_of = {"D": {"layer2": 2, "layer3": 4}, "D16": {"layer3": 2}}[variant]
    out, H, inp, f = [], (S + 1) // 2, 32, 0
    for t, c, n, s in SETTING:
        for i in range(n):
            f += 1
            st = s if i == 0 else 1
            hid = inp * t
            d = 1
            if st == 2 and LAYER_OF[f] in dil_of:
                st, d = 1, dil_of[LAYER_OF[f]]
            out.append((f, hid, H, H, st, d))
            H = (H - 1) // st + 1
            inp = c
    return out


def timed(fn, reps):
    ts = []
    for _ in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts = sorted(ts[2:])
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-stock", action="store_true")
    a = ap.parse_args()
    dev, B, st_ = "cuda", a.batch, _lib.stream
    seen, rows = set(), []
    for variant in ("D16", "D"):
        for (f, C, H, W, s, d) in dw_shapes(a.size, variant):
            key = (C, H, W, s, d)
            if key in seen:
                continue
            seen.add(key)
            Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
            x = torch.randn(B, H, W, C, device=dev, dtype=torch.bfloat16)
            dy = torch.randn(B, Ho, Wo, C, device=dev, dtype=torch.bfloat16)
            w = torch.randn(C, 1, 3, 3, device=dev) / 3
            y = torch.empty(B, Ho, Wo, C, device=dev, dtype=torch.bfloat16)
            dx = torch.empty_like(x)
            dw = torch.empty(C, 9, device=dev)
            nslab = int(_lib.lib().mrfp_dwconv_nslab(_lib.BF16, B, Ho, C))
            ws = torch.empty(B * nslab * 2 * C, device=dev)
            wws = torch.empty(int(_lib.lib().mrfp_dwconv_wgrad_ws_bytes(_lib.BF16, B, Ho, C)), device=dev, dtype=torch.uint8)
            p = lambda t: t.data_ptr()  # noqa: E731
            fwd = lambda: _lib.call("mrfp_dwconv_fwd", p(x), p(w), None, p(y), _lib.BF16, B, H, W, C, C, Ho, Wo, s, d, p(ws), st_())  # noqa: E731
            dgr = lambda: _lib.call("mrfp_dwconv_dgrad", p(dy), p(w), p(dx), _lib.BF16, B, H, W, C, C, Ho, Wo, s, d, st_())  # noqa: E731
            wgr = lambda: _lib.call("mrfp_dwconv_wgrad", p(x), p(dy), p(dw), p(wws), _lib.BF16, B, H, W, C, C, Ho, Wo, s, d, st_())  # noqa: E731
            r = {"variant": variant, "feature": f, "C": C, "H": H, "W": W, "stride": s, "dil": d,
                 "fwd_us": timed(fwd, a.reps), "dgrad_us": timed(dgr, a.reps), "wgrad_us": timed(wgr, a.reps)}
            bx, by = x.numel() * 2, y.numel() * 2
            r["fwd_TBs"] = (bx + by) / r["fwd_us"] / 1e6
            r["dgrad_TBs"] = (bx + by) / r["dgrad_us"] / 1e6
            r["wgrad_TBs"] = (bx + by) / r["wgrad_us"] / 1e6
            r["MB_moved_fwd"] = (bx + by) / 1e6
            if not a.no_stock:
                xs = x.permute(0, 3, 1, 2)                     # channels-last [B,C,H,W] view
                gys = dy.permute(0, 3, 1, 2)
                ws_ = w.to(torch.bfloat16)
                r["stock_fwd_us"] = timed(lambda: F.conv2d(xs, ws_, None, s, d, d, C), a.reps)
                cb = torch.ops.aten.convolution_backward
                r["stock_dgrad_us"] = timed(lambda: cb(gys, xs, ws_, None, [s, s], [d, d], [d, d], False, [0, 0], C,
                                                       [True, False, False]), a.reps)
                r["stock_wgrad_us"] = timed(lambda: cb(gys, xs, ws_, None, [s, s], [d, d], [d, d], False, [0, 0], C,
                                                       [False, True, False]), a.reps)
            print(json.dumps(r), flush=True)
            rows.append(r)
            del x, dy, y, dx, ws, wws
    out = os.environ.get("MRFP_OUT", "out")
    os.makedirs(out, exist_ok=True)
    json.dump(rows, open(os.path.join(out, "dw_micro.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
