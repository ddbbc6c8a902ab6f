"""Timing of the prediction path: two ways of getting the label map and the confusion histogram from the low-resolution class scores
(19 classes, pitch 32), in one process, alternating, after a warm-up of every shape, with device events over windows of >= 300 ms.

  (a) chain      ops.argmax_hist(ops.upsample_bilinear(P, size, channels=19).float(), labels, want_pred=True): the stock eval head
                 (unchanged code): writes [B,19,H,W] in the activation dtype, reads it, writes it as fp32, reads that
  (b) fused      ops.upsample_argmax(P, size, 19, labels): pred + hist in one launch
  (c) fused_all  the same with the confidence map and the validation loss switched on

at the two shapes users run, 16 x 192 x 192 -> 768 x 768 and 1 x 256 x 512 -> 1024 x 2048, in float32 and bfloat16.  Bytes are computed
from the shapes (what each path has to move, not what the caches made of it); GB/s = those bytes over the measured time.

    python tools/predict_micro.py [rounds]          # one JSON line
    python tools/predict_micro.py --model [n]       # harness.validate against harness.evaluate, MRFP+ ResNet-50 folded bf16, 1 x 3 x 1024 x 2048"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import _lib, ops  # noqa: E402

C, PITCH = 19, 32
SHAPES = [(16, 192, 192, 768, 768), (1, 256, 512, 1024, 2048)]
WINDOW_MS = 300.0


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per call


def path_bytes(B, Hi, Wi, H, W, es):
    npix, low = B * H * W, B * Hi * Wi * PITCH * es
    chain = low + npix * C * es * 2 + npix * C * 4 * 2 + npix * 8 + npix       # scores; logits written + read; fp32 copy written + read; labels; pred
    fused = low + npix * 8 + npix
    return chain, fused, fused + npix * 4                                      # (c) also writes the fp32 confidence


def micro(rounds):
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    cases = []
    for (B, Hi, Wi, H, W) in SHAPES:
        y = torch.randint(0, C, (B, H, W), generator=g)
        y[torch.rand(B, H, W, generator=g) < 0.1] = 255
        y = y.to(dev)
        for dtype in (torch.float32, torch.bfloat16):
            P = torch.zeros(B, Hi, Wi, PITCH)
            P[..., :C] = torch.randn(B, Hi, Wi, C, generator=g) * 4
            P = P.to(dev, dtype).permute(0, 3, 1, 2)
            acc = torch.zeros(2, dtype=torch.float64, device=dev)
            fns = {
                "chain": lambda P=P, y=y, s=(H, W): ops.argmax_hist(ops.upsample_bilinear(P, s, channels=C).float(), y, want_pred=True),
                "fused": lambda P=P, y=y, s=(H, W): ops.upsample_argmax(P, s, C, y),
                "fused_all": lambda P=P, y=y, s=(H, W), acc=acc: ops.upsample_argmax(P, s, C, y, want_conf=True, loss_acc=acc),
            }
            h_c, p_c = fns["chain"]()
            r = fns["fused"]()
            assert torch.equal(r.pred, p_c) and torch.equal(r.hist, h_c)       # faster and different is not faster
            cases.append(((B, Hi, Wi, H, W), dtype, fns))
    reps = {}
    for i, (shape, dtype, fns) in enumerate(cases):                            # warm-up of every shape, and the window lengths
        for k, fn in fns.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            reps[(i, k)] = max(5, int(WINDOW_MS * 1e3 / window(fn, 5)) + 1)
    out = []
    for i, (shape, dtype, fns) in enumerate(cases):
        t = {k: [] for k in fns}
        for _ in range(rounds):                                                # alternating
            for k, fn in fns.items():
                t[k].append(window(fn, reps[(i, k)]))
        es = torch.empty(0, dtype=dtype).element_size()
        byt = dict(zip(("chain", "fused", "fused_all"), path_bytes(*shape, es)))
        row = {"shape": list(shape), "dtype": str(dtype).replace("torch.", "")}
        for k in fns:
            v = sorted(t[k])
            med = v[len(v) // 2]
            row[k] = {"us": round(med, 1), "min": round(v[0], 1), "max": round(v[-1], 1), "reps": reps[(i, k)], "MB": round(byt[k] / 1e6, 1),
                      "GBps": round(byt[k] / (med * 1e-6) / 1e9, 1)}
        row["chain_over_fused"] = round(row["chain"]["us"] / row["fused"]["us"], 2)
        out.append(row)
    print(json.dumps({"op": "pred + hist from low-resolution scores", "classes": C, "pitch": PITCH, "device": torch.cuda.get_device_name(0),
                      "rounds": rounds, "window_ms": WINDOW_MS, "cases": out}))


def model_level(n):
    import contextlib
    import io
    import time
    from mrfp_amd import deepv3, harness, synth
    from mrfp_amd.config import cfg
    cfg.MODEL.ACT_DTYPE = torch.bfloat16
    with contextlib.redirect_stdout(io.StringIO()):
        m = deepv3.MRFPPlus(19, trunk="resnet-50", criterion=torch.nn.CrossEntropyLoss(ignore_index=255))
    m.load_state_dict(synth.synth_state_dict(synth.spec_of(m.state_dict()), seed=0))
    m = m.to("cuda:0")
    x, y = synth.synth_batch(1, 1024, 2048, seed=1)
    batches = [(x.to("cuda:0"), y.to("cuda:0"))] * n
    res = {}
    for _ in range(2):                                                         # the first pass of each is the warm-up
        for name, fn in (("evaluate", lambda: harness.evaluate(m, batches, fold=True)[0]),
                         ("validate", lambda: harness.validate(m, batches, fold=True)["hist"])):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = fn()                                                           # ends in a device -> host copy
            res[name] = ((time.perf_counter() - t0) / n * 1e3, h)
    assert (res["evaluate"][1] == res["validate"][1]).all()
    print(json.dumps({"op": "evaluate vs validate, MRFP+ ResNet-50, folded, bfloat16, 1x3x1024x2048", "images": n,
                      "evaluate_ms_per_image": round(res["evaluate"][0], 2), "validate_ms_per_image": round(res["validate"][0], 2)}))


def main():
    if not torch.cuda.is_available():
        raise _lib.MrfpHipError("predict_micro measures on the GPU: no device found")
    if "--model" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--model"]
        return model_level(int(rest[0]) if rest else 20)
    micro(int(sys.argv[1]) if len(sys.argv) > 1 else 5)


if __name__ == "__main__":
    main()
