"""Times the two test-time-augmentation kernels through the C ABI, next to stock PyTorch doing the same work on the same tensors.

    python tools/eval_micro.py [--out out/eval_micro.json] [--e2e]

Per shape (B x H x W, NC = 19, stride-4 source in a 32-channel padded buffer), dtype (bf16 / f32) and flip: device-event median of 10
calls after warm-up and >= 2 s of load.  Algorithmic bytes of prob_accum = read + write of acc and cnt (the source is 1/16 of a
plane); of acc_argmax_hist = read of acc, cnt and the int64 labels.  Yardstick: acc += w * softmax(interpolate(flip(logits))).
--e2e: harness.evaluate_tta (7 scales, flip, 768 x 768 windows) and harness.evaluate on 4 synthetic 1024 x 2048 images, ResNet-101
MRFP+ in bf16, seconds per image.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import _lib, synth  # noqa: E402
from mrfp_amd._lib import call, ptr, stream  # noqa: E402

NC, LD = 19, 32
SHAPES = [(1, 1024, 2048), (1, 768, 768), (16, 768, 768)]


def median_ms(fn, calls=10, load_s=2.0):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.time()
    while time.time() - t0 < load_s:           # clocks and caches in their loaded state before anything is read
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def kernels():
    rows = []
    for B, H, W in SHAPES:
        acc = torch.zeros(B, H, W, NC, device="cuda")
        cnt = torch.zeros(B, H, W, device="cuda")
        acc_nchw = torch.zeros(B, NC, H, W, device="cuda")          # stock torch's natural layout for the yardstick
        label = synth.synth_batch(1, H, W, seed=1)[1].expand(B, H, W).contiguous().cuda()
        hist = torch.zeros(NC, NC, dtype=torch.int64, device="cuda")
        hs, ws = H // 4, W // 4
        rmw = 2 * 4 * B * H * W * (NC + 1)
        for dtype in (torch.bfloat16, torch.float32):
            z = (3 * torch.randn(B, hs, ws, LD, device="cuda")).to(dtype).permute(0, 3, 1, 2)      # NHWC storage
            z_nchw = z[:, :NC].contiguous()
            for flip in (0, 1):
                def ours():
                    call("mrfp_prob_accum", ptr(z), _lib.dt(z), B, hs, ws, LD, ptr(acc), ptr(cnt), H, W, NC, 0, 0, H, W, flip, 1.0,
                         stream())

                def stock():
                    s = torch.flip(z_nchw, dims=(3,)) if flip else z_nchw
                    p = torch.softmax(F.interpolate(s.float(), size=(H, W), mode="bilinear", align_corners=True), dim=1)
                    acc_nchw.add_(p, alpha=1.0)
                    cnt.add_(1.0)
                t_o, t_s = median_ms(ours), median_ms(stock)
                rows.append({"kernel": "prob_accum", "shape": [B, H, W], "dtype": str(dtype).split(".")[1], "flip": flip,
                             "ms": t_o, "stock_ms": t_s, "bytes": rmw, "TBps": rmw / t_o / 1e9})
                print(json.dumps(rows[-1]), flush=True)

        def closing():
            call("mrfp_acc_argmax_hist", ptr(acc), ptr(cnt), ptr(label), B * H * W, NC, ptr(hist), None, None, stream())

        def closing_stock():
            pred = acc.argmax(dim=-1)
            m = (label >= 0) & (label < NC)
            hist.add_(torch.bincount(NC * label[m] + pred[m], minlength=NC * NC).view(NC, NC))
        nbytes = 4 * B * H * W * (NC + 1) + 8 * B * H * W
        t_o, t_s = median_ms(closing), median_ms(closing_stock)
        rows.append({"kernel": "acc_argmax_hist", "shape": [B, H, W], "ms": t_o, "stock_ms": t_s, "bytes": nbytes,
                     "TBps": nbytes / t_o / 1e9})
        print(json.dumps(rows[-1]), flush=True)
        del acc, cnt, acc_nchw
    return rows


def end_to_end():
    from mrfp_amd import deepv3, harness
    from mrfp_amd.config import cfg
    cfg.MODEL.ACT_DTYPE = torch.bfloat16
    model = deepv3.MRFPPlus(NC, trunk="resnet-101", criterion=torch.nn.CrossEntropyLoss(ignore_index=255))
    model.load_state_dict(synth.synth_state_dict(synth.spec_of(model.state_dict()), seed=0, residual_gain=0.3))
    model = model.cuda()
    batches = []
    for i in range(4):
        x, y = synth.synth_batch(1, 1024, 2048, seed=40 + i)
        batches.append((x.cuda(), y.cuda()))
    out = {}
    for name, fn in (("evaluate", lambda: harness.evaluate(model, batches)),
                     ("evaluate_tta", lambda: harness.evaluate_tta(model, batches, scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0),
                                                                   flip=True, window=(768, 768)))):
        fn()                                        # warm-up: weight packs, launch plans
        torch.cuda.synchronize()
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        out[name + "_s_per_image"] = (time.time() - t0) / len(batches)
        print(json.dumps({name + "_s_per_image": out[name + "_s_per_image"]}), flush=True)
    out["variants_per_image"] = len(harness.tta_variants(1024, 2048, (1024, 2048), (0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0), True,
                                                         (768, 768), None))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.environ.get("MRFP_OUT", "out"), "eval_micro.json"))
    ap.add_argument("--e2e", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_micro needs a GPU: a CPU timing says nothing about these kernels")
    res = {"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0), "kernels": kernels()}
    if a.e2e:
        res["end_to_end"] = end_to_end()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    slow = [r for r in res["kernels"] if r["ms"] > r["stock_ms"]]
    print("slower than stock on %d of %d rows" % (len(slow), len(res["kernels"])))
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
