"""Golden vectors of the Resize and Crop training compositions: outputs of the reference's own sequence of PIL calls for a small
seeded image and fixed draws (Pillow 12.2.0).

    python tests/golden/make_golden_input_resize.py   ->  tests/golden/input_resize.npz  (inputs + expected outputs)

Resize composition (Foggy Cityscapes main.py:319-330, BDD100k :499-507, Synthia :592-603): RandomHorizontalFlip -> ColorJitter ->
Resize(size1, size2) (dataloaders.py:467-482: img.resize((size1, size2), BILINEAR), mask.resize(..., NEAREST); PIL reads the pair
as (width, height)) -> RandomGaussianBlur -> ToTensor.
Crop composition (Mapillary main.py:764-773): RandomHorizontalFlip -> ColorJitter -> RandomCrop_p(base_size, crop_size)
(dataloaders.py:216-234: crop (x0, y0, x0 + crop_size, y0 + base_size)) -> RandomGaussianBlur -> ToTensor."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import input_oracle as io  # noqa: E402

J1 = [("hue", -0.21), ("contrast", 1.13), ("brightness", 0.62), ("saturation", 0.9)]
J2 = [("saturation", 1.2), ("brightness", 1.5), ("hue", 0.3), ("contrast", 0.8)]
# (size1, size2) = (width, height) of the Resize step; the source image is 30 x 40 (H x W)
RESIZE = [
    dict(size=(56, 44), flip=False, jitter=None, blur=None),          # up-scaling, non-square
    dict(size=(56, 44), flip=True, jitter=J1, blur=0.61),
    dict(size=(24, 18), flip=True, jitter=J2, blur=None),             # down-scaling
    dict(size=(24, 18), flip=False, jitter=None, blur=0.05),
    dict(size=(40, 30), flip=True, jitter=None, blur=0.37),           # unchanged size: a copy (mirrored)
    dict(size=(40, 21), flip=False, jitter=J1, blur=None),            # only the height changes: one pass
    dict(size=(17, 30), flip=True, jitter=None, blur=None),           # only the width changes
]
# (base_size, crop_size): base_size tall, crop_size wide
CROP_SIZE = (20, 28)
CROP = [
    dict(crop=(0, 0), flip=False, jitter=None, blur=None),
    dict(crop=(12, 10), flip=True, jitter=J2, blur=0.83),
    dict(crop=(5, 3), flip=True, jitter=None, blur=None),
    dict(crop=(7, 9), flip=False, jitter=J1, blur=0.2),
]


def _flip_jitter(img, mask, flip, jitter):
    from PIL import Image
    if flip:                                                             # dataloaders.py:145-147
        img, mask = img.transpose(Image.FLIP_LEFT_RIGHT), mask.transpose(Image.FLIP_LEFT_RIGHT)
    for op, factor in (jitter or []):                                    # ColorJitter :596-660
        img = io.jitter_pil(img, op, factor)
    return img, mask


def _blur_totensor(img, mask, blur):
    if blur is not None:                                                 # RandomGaussianBlur :172-174
        from PIL import ImageFilter
        img = img.filter(ImageFilter.GaussianBlur(radius=blur))
    return np.array(img).astype(np.float32).transpose((2, 0, 1)), np.array(mask).astype(np.float32)   # ToTensor :128-133


def resize_pil(img, mask, *, size, flip, jitter, blur):
    """The reference's PIL calls of the Resize composition for one draw: PIL images in -> (float32 [3,h,w], float32 [h,w])."""
    from PIL import Image
    img, mask = _flip_jitter(img, mask, flip, jitter)
    img, mask = img.resize(size, Image.BILINEAR), mask.resize(size, Image.NEAREST)      # :479-480
    return _blur_totensor(img, mask, blur)


def crop_pil(img, mask, *, base_size, crop_size, crop, flip, jitter, blur):
    """The reference's PIL calls of the Crop composition for one draw."""
    img, mask = _flip_jitter(img, mask, flip, jitter)
    x0, y0 = crop
    box = (x0, y0, x0 + crop_size, y0 + base_size)                       # :229-231
    img, mask = img.crop(box), mask.crop(box)
    return _blur_totensor(img, mask, blur)


def source():
    rng = np.random.default_rng(2025)
    img = rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)
    img[:3] = img[:3, :, :1]                   # grey pixels
    lab = rng.integers(0, 19, (30, 40), dtype=np.uint8)
    lab[rng.random((30, 40)) < 0.05] = 255
    return img, lab


def main():
    from PIL import Image
    img, lab = source()
    out = {"img": img, "lab": lab}
    for i, d in enumerate(RESIZE):
        im, lb = resize_pil(Image.fromarray(img), Image.fromarray(lab), **d)
        out["resize_img_%d" % i], out["resize_lab_%d" % i] = im.astype(np.uint8), lb.astype(np.uint8)   # exact: integers 0..255
    for i, d in enumerate(CROP):
        im, lb = crop_pil(Image.fromarray(img), Image.fromarray(lab), base_size=CROP_SIZE[0], crop_size=CROP_SIZE[1], **d)
        out["crop_img_%d" % i], out["crop_lab_%d" % i] = im.astype(np.uint8), lb.astype(np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "input_resize.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
