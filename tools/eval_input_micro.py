"""Times the evaluation input path per sample: on the device, and the same work done the reference's way (numpy loops + PIL) on one
host core of the same machine.  profiles/eval_input.md is one run of

    timeout -k 10 600 python tools/eval_input_micro.py host && timeout -k 10 300 python tools/eval_input_micro.py lut && \
    timeout -k 10 300 python tools/eval_input_micro.py transforms && python tools/eval_input_micro.py report

Every step writes out/eval_input_<step>.json (MRFP_OUT names another directory); `report` joins them into the table of
profiles/eval_input.md (out/eval_input_table.md).
  host        encode_segmap-style in-place loops (35 passes) and the 66-pass copy loop on a uint8 map, numpy's ToTensor, and PIL's
              resize(BICUBIC) / resize(NEAREST) / expand / crop + ToTensor; one thread, median of 5; needs no GPU
  lut         mrfp_label_lut_u8 (out of place and in place), mrfp_label_encode_i64, and the in-tree yardstick for a uint8-in
              streaming pass, mrfp_u8hwc_to_f32chw, at 1024x2048 and 3000x4000: device-event median of single launches and of bursts of 20, bytes moved per second in a burst
  transforms  EvalTransform at 1024x2048; ResizeHeightCenterCropPad 3000x4000 -> 1536x1536 with warm tables (device events) and
              with cold tables (a new transform object per call: host table build + upload included, wall clock with a sync)
The device steps need a GPU: there is no fallback."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("MRFP_OUT", os.path.join(ROOT, "out"))
SIZES = [(1024, 2048), (3000, 4000)]
EVAL = 1536


def _save(step, rows):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "eval_input_%s.json" % step)
    json.dump(rows, open(path, "w"), indent=1)
    for r in rows:
        print(json.dumps(r))
    print(path)


def _maps(H, W, ids):
    rng = np.random.default_rng(H)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    blocks = rng.integers(0, ids, (H // 8 + 1, W // 8 + 1), dtype=np.uint8)          # 8x8 patches of one class, some noise on top
    lab = np.kron(blocks, np.ones((8, 8), np.uint8))[:H, :W].copy()
    noise = rng.random((H, W)) < 0.02
    lab[noise] = rng.integers(0, ids, int(noise.sum()), dtype=np.uint8)
    return img, lab


def _host_median(fn, reps=5):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def host():
    import torch
    torch.set_num_threads(1)
    from PIL import Image, ImageOps
    from mrfp_amd import input_pipeline as ip
    city = dict(void=[0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30, -1], valid=[i for i, v in enumerate(ip.label_encoder("Cityscapes").table[:34]) if v < 19])
    mapillary = {i: int(v) for i, v in enumerate(ip.label_encoder("Mapillary").table[:66])}
    rows = []
    for H, W in SIZES:
        img, lab = _maps(H, W, 34)

        def inplace_loops():
            m = lab.copy()
            for c in city["void"]:
                m[m == c] = 255
            for i, c in enumerate(city["valid"]):
                m[m == c] = i
            return m

        def copy_loop():
            out = lab.copy()
            for k, v in mapillary.items():
                out[lab == k] = v
            return out

        def to_tensor():
            a = torch.from_numpy(np.array(img).astype(np.float32).transpose((2, 0, 1))).float()
            b = torch.from_numpy(np.array(lab).astype(np.float32)).float()
            return a, b
        rows.append(dict(what="host in-place loops, 16 void + 19 valid passes", H=H, W=W, ms=_host_median(inplace_loops)))
        rows.append(dict(what="host copy loop, 66 passes", H=H, W=W, ms=_host_median(copy_loop)))
        rows.append(dict(what="host ToTensor (numpy astype + transpose)", H=H, W=W, ms=_host_median(to_tensor)))
    H, W = SIZES[1]
    img, lab = _maps(H, W, 66)
    pi, pl = Image.fromarray(img), Image.fromarray(lab)
    tf = ip.ResizeHeightCenterCropPad(EVAL)
    tw, pad_x, x1 = tf.geometry(W, H)

    def pil_val():
        a, b = pi.resize((tw, EVAL), Image.BICUBIC), pl.resize((tw, EVAL), Image.NEAREST)
        if pad_x:
            a, b = ImageOps.expand(a, border=(pad_x, 0, pad_x, 0), fill=0), ImageOps.expand(b, border=(pad_x, 0, pad_x, 0), fill=0)
        a, b = a.crop((x1, 0, x1 + EVAL, EVAL)), b.crop((x1, 0, x1 + EVAL, EVAL))
        return np.array(a).astype(np.float32).transpose((2, 0, 1)), np.array(b).astype(np.float32)
    rows.append(dict(what="host PIL resize(BICUBIC/NEAREST) + crop + ToTensor -> %d^2" % EVAL, H=H, W=W, ms=_host_median(pil_val)))
    _save("host", rows)


def _dev_median(fn, calls=20, load_s=1.0):
    import torch
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


def lut():
    import torch
    from mrfp_amd import input_pipeline as ip
    from mrfp_amd._lib import call, ptr, stream
    rows = []
    enc = ip.label_encoder("Mapillary")
    for H, W in SIZES:
        img, lab = _maps(H, W, 66)
        xi, xl = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
        o8, o64, of = torch.empty_like(xl), torch.empty(H, W, dtype=torch.int64, device="cuda"), torch.empty(3, H, W, device="cuda")
        scratch = xl.clone()
        n = H * W
        for what, fn, nbytes in (
                ("mrfp_label_lut_u8", lambda: enc(xl, out=o8), 2 * n),
                ("mrfp_label_lut_u8 in place", lambda: enc(scratch, out=scratch), 2 * n),
                ("mrfp_label_encode_i64", lambda: enc.to_int64(xl, out=o64), 9 * n),
                ("mrfp_u8hwc_to_f32chw (yardstick)", lambda: call("mrfp_u8hwc_to_f32chw", ptr(xi), ptr(of), H, W, stream()), 15 * n)):
            ms = _dev_median(fn)

            def burst(fn=fn):                   # 20 launches between one pair of events: the per-launch time without the pair's own floor
                for _ in range(20):
                    fn()
            ms20 = _dev_median(burst, calls=10, load_s=0.5) / 20
            rows.append(dict(what=what, H=H, W=W, ms=ms, ms_in_burst=ms20, bytes=nbytes, GBps=nbytes / ms20 / 1e6))
    _save("lut", rows)


def transforms():
    import torch
    from mrfp_amd import input_pipeline as ip
    rows = []
    H, W = SIZES[0]
    img, lab = _maps(H, W, 34)
    xi, xl = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
    oi, ol = torch.empty(3, H, W, device="cuda"), torch.empty(H, W, dtype=torch.int64, device="cuda")
    tf, enc = ip.EvalTransform(), ip.label_encoder("Cityscapes")
    rows.append(dict(what="EvalTransform + Cityscapes encoder", H=H, W=W, ms=_dev_median(lambda: tf(xi, xl, enc, oi, ol))))
    H, W = SIZES[1]
    img, lab = _maps(H, W, 66)
    xi, xl = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
    oi, ol = torch.empty(3, EVAL, EVAL, device="cuda"), torch.empty(EVAL, EVAL, dtype=torch.int64, device="cuda")
    enc = ip.label_encoder("Mapillary")
    warm = ip.ResizeHeightCenterCropPad(EVAL)
    rows.append(dict(what="ResizeHeightCenterCropPad(%d) + Mapillary encoder, warm tables" % EVAL, H=H, W=W,
                     ms=_dev_median(lambda: warm(xi, xl, enc, oi, ol))))
    ts = []
    for _ in range(7):                          # cold: the lru caches of the host tables emptied, a new object, wall clock to the sync
        ip._bicubic_tables.cache_clear()
        ip._nearest_table.cache_clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ip.ResizeHeightCenterCropPad(EVAL)(xi, xl, enc, oi, ol)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    rows.append(dict(what="ResizeHeightCenterCropPad(%d) + Mapillary encoder, cold tables (wall clock)" % EVAL, H=H, W=W,
                     ms=sorted(ts)[len(ts) // 2]))
    t0 = time.perf_counter()
    for _ in range(20):
        warm(xi, xl, enc, oi, ol)
    torch.cuda.synchronize()
    rows.append(dict(what="the same, warm tables (wall clock, 20 calls back to back)", H=H, W=W, ms=(time.perf_counter() - t0) * 1e3 / 20))
    _save("transforms", rows)


def report():
    rows = []
    for step in ("host", "lut", "transforms"):
        rows += json.load(open(os.path.join(OUT, "eval_input_%s.json" % step)))
    lines = ["| what | H x W | ms per sample | ms in a burst of 20 | GB/s (burst) |", "|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d x %d | %.3f | %s | %s |" % (r["what"], r["H"], r["W"], r["ms"], "%.4f" % r["ms_in_burst"] if "ms_in_burst" in r else "",
                                                       "%.0f" % r["GBps"] if "GBps" in r else ""))
    path = os.path.join(OUT, "eval_input_table.md")
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(path)


if __name__ == "__main__":
    {"host": host, "lut": lut, "transforms": transforms, "report": report}[sys.argv[1]]()
