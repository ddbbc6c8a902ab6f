"""Timing of the frequency filters (HPF / LPF / PHOT, csrc/freq.hip) on a batch, and of the Resize / Crop training compositions
per image against the same PIL calls on one host core.    python tools/freq_micro.py [B H W reps]

Filters: device events around `reps` calls after a warm-up, per call; the algorithmic FLOP and byte counts are computed here from
the shapes (band filter: two band-limited DFT passes over every pixel; PHOT: the line FFTs' 5 N log2 N per transform and the
88 bytes per pixel the three passes move)."""
import json
import math
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import input_pipeline as ip  # noqa: E402


def time_call(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def filters(B, H, W, reps):
    x = torch.randint(0, 256, (B, 3, H, W), device="cuda").float()
    out = torch.empty_like(x)
    planes, npix = 3 * B, B * H * W
    nk = min(16, W // 2) + 1
    band_flop = planes * H * W * 2 * nk * 2 * 2          # forward rows + output pass: 2 nk real columns, one FMA = 2 FLOP each
    phot_flop = 2 * 2 * B * 5 * H * W * math.log2(H * W)  # two 2-D transforms (channel sum, z), forward + inverse
    res = {"batch": [B, 3, H, W]}
    for name, fn, flop, nbytes in (("hpf", lambda: ip.hpf(x, out=out), band_flop, 2 * 4 * 3 * npix + 4 * 3 * npix),
                                   ("lpf", lambda: ip.lpf(x, out=out), band_flop, 2 * 4 * 3 * npix + 4 * 3 * npix),
                                   ("phot", lambda: ip.phot(x, out=out), phot_flop, 88 * npix)):
        ms = time_call(fn, reps)
        res[name] = {"us_per_batch": round(ms * 1e3, 1), "gflop": round(flop / 1e9, 2), "tflops": round(flop / ms / 1e9, 2),
                     "gb": round(nbytes / 1e9, 3), "tb_per_s": round(nbytes / ms / 1e9, 2)}
    return res


def transforms(reps):
    try:
        from PIL import Image
    except ImportError:
        Image = None
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    res = {}
    rng = np.random.default_rng(0)
    for name, (H, W), t in (("resize 1024x2048 -> 768x768 (Foggy / BDD / Synthia)", (1024, 2048), ip.ResizeTransform(768, 768)),
                            ("crop 1024x2048 -> 768x768 (Mapillary)", (1024, 2048), ip.CropTransform(768, 768))):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        lab = rng.integers(0, 19, (H, W), dtype=np.uint8)
        r, nr = random.Random(0), np.random.RandomState(0)
        draws = [t.draw(W, H, r, nr) for _ in range(reps)]
        xi, xl = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
        oi = torch.empty((3, 768, 768), device="cuda")
        ol = torch.empty((768, 768), dtype=torch.int64, device="cuda")
        for d in draws[:3]:
            t(xi, xl, d, oi, ol)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for d in draws:
            t(xi, xl, d, oi, ol)
        torch.cuda.synchronize()
        gpu_ms = (time.perf_counter() - t0) / reps * 1e3
        row = {"gpu_ms_per_image": round(gpu_ms, 3), "gpu_images_per_s": round(1e3 / gpu_ms, 1)}
        if Image is not None:
            import make_golden_input_resize as mg
            pi, pl = Image.fromarray(img), Image.fromarray(lab)
            t0 = time.perf_counter()
            for d in draws:
                if isinstance(t, ip.ResizeTransform):
                    mg.resize_pil(pi, pl, size=(t.size1, t.size2), flip=d.flip, jitter=d.jitter, blur=d.blur)
                else:
                    mg.crop_pil(pi, pl, base_size=t.base_size, crop_size=t.crop_size, crop=d.crop, flip=d.flip, jitter=d.jitter,
                                blur=d.blur)
            row["pil_ms_per_image_one_core"] = round((time.perf_counter() - t0) / reps * 1e3, 2)
        else:
            row["pil_ms_per_image_one_core"] = "not measured (no Pillow)"
        res[name] = row
    return res


def main():
    a = [int(v) for v in sys.argv[1:]]
    B, H, W, reps = (a + [16, 768, 768, 20][len(a):])[:4]
    print(json.dumps({"filters": filters(B, H, W, reps), "transforms": transforms(reps)}))


if __name__ == "__main__":
    main()
