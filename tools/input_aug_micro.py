"""Timing of ScaleCropTransform (with rotation) and FixScaleCropTransform on the GPU against the same PIL / numpy calls on one
host core (the sibling of tools/input_micro.py).    python tools/input_aug_micro.py [H W crop reps]"""
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import input_aug_common as iac  # noqa: E402  (the PIL call sequences of the classes)
from mrfp_amd.input_pipeline import FixScaleCropTransform, ScaleCropTransform  # noqa: E402


def _time(fn, items, reps_over=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps_over):
        for it in items:
            fn(it)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (len(items) * reps_over) * 1e3


def main():
    a = [int(v) for v in sys.argv[1:]]
    H, W, crop, reps = (a + [1024, 2048, 768, 20][len(a):])[:4]
    torch.set_num_threads(1)
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    lab = rng.integers(0, 19, (H, W), dtype=np.uint8)
    xi, xl = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
    out_i = torch.empty(3, crop, crop, device="cuda")
    out_l = torch.empty(crop, crop, dtype=torch.int64, device="cuda")
    results = []

    kw = dict(fill=255, rotate_degree=10, jitter=True, contrast=True, normalize=iac.IMAGENET)
    tt = ScaleCropTransform(crop, crop, **kw)
    r, nr = random.Random(0), np.random.RandomState(0)
    draws = [tt.draw(W, H, r, nr) for _ in range(reps)]
    for d in draws[:3]:
        tt(xi, xl, d, out_i, out_l)
    cold = _time(lambda d: tt(xi, xl, d, out_i, out_l), draws[3:])     # every draw has a new scaled size: tables built + uploaded
    warm = _time(lambda d: tt(xi, xl, d, out_i, out_l), draws)         # tables cached
    pil = _time(lambda d: iac.scale_crop_pil(img, lab, **iac.draw_kwargs(d), crop_size=crop, fill=255, contrast=True,
                                             normalize=iac.IMAGENET), draws)
    results.append({"op": "ScaleCropTransform (flip, ColorJitter and blur on half the draws each, rotation within 10 degrees, bilinear "
                          "rescale, pad, crop, Contrast, Normalize, ToTensor)", "source": [H, W], "crop": crop,
                    "mean_short_size": round(float(np.mean([min(d.scaled) for d in draws])), 1), "gpu_ms_per_image": round(warm, 3),
                    "gpu_ms_per_image_new_tables": round(cold, 3), "pil_ms_per_image_one_core": round(pil, 2)})

    rot_only = ScaleCropTransform(crop, crop, rotate_degree=10)
    d0 = [rot_only.draw(W, H, random.Random(i)) for i in range(reps)]
    for d in d0:
        rot_only(xi, xl, d, out_i, out_l)
    warm = _time(lambda d: rot_only(xi, xl, d, out_i, out_l), d0)
    pil = _time(lambda d: iac.scale_crop_pil(img, lab, **iac.draw_kwargs(d), crop_size=crop), d0)
    results.append({"op": "ScaleCropTransform (flip, rotation, rescale, pad, crop, blur on half the draws, ToTensor)", "source": [H, W],
                    "crop": crop, "gpu_ms_per_image": round(warm, 3), "pil_ms_per_image_one_core": round(pil, 2)})

    ft = FixScaleCropTransform(crop, contrast=True, normalize=iac.IMAGENET)
    for _ in range(3):
        ft(xi, xl, None, out_i, out_l)
    warm = _time(lambda _: ft(xi, xl, None, out_i, out_l), list(range(reps)))
    pil = _time(lambda _: iac.fix_scale_crop_pil(img, lab, crop, True, iac.IMAGENET), list(range(reps)))
    results.append({"op": "FixScaleCropTransform (bilinear rescale of the kept columns and rows, centre crop, Contrast, Normalize, ToTensor)",
                    "source": [H, W], "crop": crop, "gpu_ms_per_image": round(warm, 3), "pil_ms_per_image_one_core": round(pil, 2)})
    for res in results:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
