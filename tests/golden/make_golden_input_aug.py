"""Golden vectors of the augmentation compositions: outputs of the PIL calls of the reference's classes for a small hashed image
and fixed draws (Pillow 12.2.0, numpy for Normalize).

    python tests/golden/make_golden_input_aug.py   ->  tests/golden/input_aug.npz  (inputs + expected outputs)

Train cases (tests/input_aug_common.py::GOLDEN_TRAIN; the call sequence is scale_crop_pil there, cited line by line):
RandomHorizontalFlip (dataloaders.py:139-150) -> ColorJitter (:596-660) -> RandomRotate (:153-165: img.rotate(angle, BILINEAR),
mask.rotate(angle, NEAREST), no fillcolor) -> RandomScaleCrop (:180-214: resize BILINEAR / NEAREST, ImageOps.expand with
border=(0, 0, padw, padh) when short_size < crop_size, crop) -> RandomGaussianBlur (:168-177) -> Contrast (:83-93) -> Normalize
(:95-115) -> ToTensor (:118-136).  The reference never composes these classes itself: the order is this build's.
Eval cases (GOLDEN_EVAL; fix_scale_crop_pil): FixScaleCrop (:439-465) -> Contrast -> Normalize -> ToTensor.
Images are stored as float32 (Normalize leaves no integers), labels as uint8."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import input_aug_common as iac  # noqa: E402


def main():
    img, lab = iac.golden_source()
    out = {"img": img, "lab": lab}
    for i, case in enumerate(iac.GOLDEN_TRAIN):
        im, lb = iac.scale_crop_pil(img, lab, crop_size=iac.GOLDEN_CROP, **case)
        out["train_img_%d" % i], out["train_lab_%d" % i] = im, lb.astype(np.uint8)        # labels: integers 0..255
    for i, case in enumerate(iac.GOLDEN_EVAL):
        si, sl = iac.golden_source(case["w"], case["h"])
        im, lb = iac.fix_scale_crop_pil(si, sl, iac.GOLDEN_CROP, case["contrast"], case["normalize"])
        out["eval_src_img_%d" % i], out["eval_src_lab_%d" % i] = si, sl
        out["eval_img_%d" % i], out["eval_lab_%d" % i] = im, lb.astype(np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "input_aug.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
