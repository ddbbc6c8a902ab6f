"""Numpy restatements of the augmentation half of the input path (mrfp_amd/input_pipeline.py: rotate, contrast,
ScaleCropTransform, FixScaleCropTransform; csrc/input.hip: affine_u8, u8hwc_to_f32chw_norm), the samples and the cases that
tests/test_input_aug_cpu.py, tests/test_input_aug_golden.py, tests/test_input_aug_gpu.py and
tests/golden/make_golden_input_aug.py share.  Resize, blend and blur come from oracle/input_oracle.py.

The arithmetic inside Image.rotate is restated from the published algorithm of the third-party dependency Pillow (pinned here:
12.2.0; Image.py rotate; src/libImaging/Geometry.c affine_transform, bilinear_filter32RGB, affine_fixed, ImagingTransformAffine)
and pinned against PIL itself in tests/test_input_aug_cpu.py."""
import math
import os

import numpy as np

from oracle import input_oracle as io

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "input_aug.npz")

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))       # main.py:140
SHAPES = ((37, 53), (64, 64), (130, 70), (257, 511))            # H x W: odd, square (the 90 / 270 transposes), tall, > one block row
ANGLES = (7.3, -13.9, 45, 90, 270, 179.99, 180, 0, 360, 367.3, -0.001, 123.456)


def sample(w: int, h: int, seed: int = 0):
    """-> (uint8 [h,w,3] image, uint8 [h,w] label map with the values 0..18 and 255) from integer arithmetic alone (no random
    generator whose stream could differ between numpy versions)."""
    y, x = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")

    def mix(c):
        v = (y * np.uint64(7919) + x * np.uint64(104729) + np.uint64(c * 1299709 + seed * 15485863 + 12345)) * np.uint64(2654435761)
        v ^= v >> np.uint64(15)
        v = (v * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
        return v ^ (v >> np.uint64(13))
    img = np.stack([(mix(c) & np.uint64(255)).astype(np.uint8) for c in range(3)], -1)
    # smooth ramps under the noise on half of the image: bilinear fractions then meet both flat and busy neighbourhoods
    ramp = ((x * np.uint64(3) + y * np.uint64(5)) & np.uint64(255)).astype(np.uint8)
    img[:, : w // 2] = (img[:, : w // 2] >> 3) + (ramp[:, : w // 2, None] >> 1)
    m = mix(3)
    lab = ((m >> np.uint64(8)) % np.uint64(19)).astype(np.uint8)
    lab[(m & np.uint64(31)) == 0] = 255
    return np.ascontiguousarray(img), np.ascontiguousarray(lab)


# ---- Image.rotate ------------------------------------------------------------------------------------------------------------
def rotate_matrix(w: int, h: int, angle: float):
    """Image.rotate's dispatch and matrix -> ("copy" | "rot90" | "rot180" | "rot270" | "affine", [m0..m5] or None)."""
    angle = angle % 360.0
    if angle == 0:
        return "copy", None
    if angle == 180:
        return "rot180", None
    if angle in (90, 270) and w == h:
        return ("rot90" if angle == 90 else "rot270"), None
    center = (w / 2, h / 2)
    angle = -math.radians(angle)
    matrix = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
              round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    x, y = -center[0] - 0, -center[1] - 0
    a, b, c, d, e, f = matrix
    matrix[2], matrix[5] = a * x + b * y + c, d * x + e * y + f
    matrix[2] += center[0]
    matrix[5] += center[1]
    return "affine", matrix


def fixed_range_ok(w: int, h: int, m) -> bool:
    """ImagingTransformAffine's check_fixed on the four corners: the NEAREST transform stays in 16.16 fixed point."""
    return all(abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0
               for x, y in ((0, 0), (w, h), (0, h), (w, 0)))


def affine_bilinear(img: np.ndarray, m) -> np.ndarray:
    """ImagingGenericTransform(affine_transform, bilinear_filter32RGB), fill 0: uint8 [H,W,3] -> the same shape."""
    H, W = img.shape[:2]
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    xc, yc = x + 0.5, y + 0.5
    xin = m[0] * xc + m[1] * yc + m[2]
    yin = m[3] * xc + m[4] * yc + m[5]
    inside = ~((xin < 0.0) | (xin >= W) | (yin < 0.0) | (yin >= H))
    xin, yin = xin - 0.5, yin - 0.5
    fx, fy = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)       # FLOOR: floor below 0, truncation above
    dx, dy = (xin - fx)[..., None], (yin - fy)[..., None]
    x0, x1 = np.clip(fx, 0, W - 1), np.clip(fx + 1, 0, W - 1)
    y0 = np.clip(fy, 0, H - 1)
    src = img.astype(np.float64)
    a, b = src[y0, x0], src[y0, x1]
    v1 = a + (b - a) * dx
    has2 = ((fy + 1 >= 0) & (fy + 1 < H))[..., None]
    y1 = np.clip(fy + 1, 0, H - 1)
    e, f = src[y1, x0], src[y1, x1]
    v2 = np.where(has2, e + (f - e) * dx, v1)
    out = (v1 + (v2 - v1) * dy).astype(np.int64).astype(np.uint8)                 # (UINT8)v: truncation
    return np.where(inside[..., None], out, 0).astype(np.uint8)


def affine_fixed(lab: np.ndarray, m) -> np.ndarray:
    """Geometry.c affine_fixed (NEAREST), fill 0: uint8 [H,W] -> the same shape."""
    H, W = lab.shape
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    a0, a1, a3, a4 = fix(m[0]), fix(m[1]), fix(m[3]), fix(m[4])
    a2 = fix(m[2] + m[0] * 0.5 + m[1] * 0.5)
    a5 = fix(m[5] + m[3] * 0.5 + m[4] * 0.5)
    x, y = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    xin, yin = (a2 + a1 * y + a0 * x) >> 16, (a5 + a4 * y + a3 * x) >> 16
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    return np.where(inside, lab[np.clip(yin, 0, H - 1), np.clip(xin, 0, W - 1)], 0).astype(np.uint8)


def rotate_numpy(img: np.ndarray, lab: np.ndarray, angle: float):
    """img.rotate(angle, BILINEAR), mask.rotate(angle, NEAREST) on arrays."""
    H, W = lab.shape
    kind, m = rotate_matrix(W, H, angle)
    if kind == "copy":
        return img.copy(), lab.copy()
    if kind != "affine":
        k = {"rot90": 1, "rot180": 2, "rot270": 3}[kind]
        return np.ascontiguousarray(np.rot90(img, k)), np.ascontiguousarray(np.rot90(lab, k))
    assert fixed_range_ok(W, H, m)
    return affine_bilinear(img, m), affine_fixed(lab, m)


# ---- RandomScaleCrop / FixScaleCrop / Normalize ----------------------------------------------------------------------------------
def scale_crop_geometry(w: int, h: int, short_size: int, crop_size: int):
    """RandomScaleCrop -> ((ow, oh), (padw, padh))."""
    if h > w:
        ow = short_size
        oh = int(1.0 * h * ow / w)
    else:
        oh = short_size
        ow = int(1.0 * w * oh / h)
    padw = padh = 0
    if short_size < crop_size:
        padh = crop_size - oh if oh < crop_size else 0
        padw = crop_size - ow if ow < crop_size else 0
    return (ow, oh), (padw, padh)


def _resize_pair(img, lab, ow, oh):
    H, W = lab.shape
    return io.resample_u8(np.ascontiguousarray(img), ow, oh, "bilinear"), lab[io.nearest_table(H, oh)][:, io.nearest_table(W, ow)]


def random_scale_crop_numpy(img, lab, scaled, pad, crop_xy, crop_size: int, fill: int = 0):
    (ow, oh), (padw, padh), (x1, y1) = scaled, pad, crop_xy
    img, lab = _resize_pair(img, lab, ow, oh)
    if padw or padh:                                                  # right and bottom only
        img = np.pad(img, ((0, padh), (0, padw), (0, 0)), constant_values=0)
        lab = np.pad(lab, ((0, padh), (0, padw)), constant_values=fill)
    t = crop_size
    return img[y1:y1 + t, x1:x1 + t], lab[y1:y1 + t, x1:x1 + t]


def fix_scale_crop_geometry(w: int, h: int, crop_size: int):
    if w > h:
        oh = crop_size
        ow = int(1.0 * w * oh / h)
    else:
        ow = crop_size
        oh = int(1.0 * h * ow / w)
    return ow, oh, int(round((ow - crop_size) / 2.)), int(round((oh - crop_size) / 2.))


def fix_scale_crop_numpy(img, lab, crop_size: int):
    H, W = lab.shape
    ow, oh, x1, y1 = fix_scale_crop_geometry(W, H, crop_size)
    img, lab = _resize_pair(img, lab, ow, oh)
    t = crop_size
    return img[y1:y1 + t, x1:x1 + t], lab[y1:y1 + t, x1:x1 + t]


def normalize_numpy(img_u8: np.ndarray, mean, std) -> np.ndarray:
    """Normalize with the precision of every step written out: the division by the Python scalar 255.0 stays in float32; mean
    and std are tuples, which numpy takes as float64 arrays, so `-=` and `/=` compute in float64 and round into the float32
    array.  uint8 [H,W,3] -> float32 [H,W,3]."""
    v = img_u8.astype(np.float32) / np.float32(255.0)
    v = (v.astype(np.float64) - np.asarray(mean, np.float64)).astype(np.float32)
    return (v.astype(np.float64) / np.asarray(std, np.float64)).astype(np.float32)


def normalize_reference(img_u8: np.ndarray, mean, std) -> np.ndarray:
    """The statements of Normalize.__call__ as numpy runs them."""
    img = np.array(img_u8).astype(np.float32)
    img /= 255.0
    img -= mean
    img /= std
    return img


def finish_numpy(img_u8, lab_u8, blur=None, contrast=False, normalize=None):
    """RandomGaussianBlur -> Contrast -> Normalize -> ToTensor on arrays -> (float32 [3,H,W], int64 [H,W])."""
    if blur is not None and blur != 0:
        img_u8 = io.gaussian_blur_u8(np.ascontiguousarray(img_u8), blur)
    if contrast:
        img_u8 = io.jitter_u8(np.ascontiguousarray(img_u8), "contrast", 2.0)
    out = img_u8.astype(np.float32) if normalize is None else normalize_numpy(img_u8, *normalize)
    return np.ascontiguousarray(out.transpose(2, 0, 1)), np.ascontiguousarray(lab_u8).astype(np.int64)


def scale_crop_numpy(img, lab, *, flip, jitter, degrees, scaled, pad, crop, blur, crop_size, fill=0, contrast=False,
                     normalize=None):
    """ScaleCropTransform from the restated arithmetic alone."""
    if flip:
        img, lab = img[:, ::-1], lab[:, ::-1]
    for op, factor in (jitter or []):
        img = io.jitter_u8(np.ascontiguousarray(img), op, factor)
    if degrees is not None:
        img, lab = rotate_numpy(np.ascontiguousarray(img), np.ascontiguousarray(lab), degrees)
    img, lab = random_scale_crop_numpy(img, lab, scaled, pad, crop, crop_size, fill)
    return finish_numpy(img, lab, blur, contrast, normalize)


def fix_scale_crop_transform_numpy(img, lab, crop_size, contrast=False, normalize=None, table=None):
    img, lab = fix_scale_crop_numpy(img, lab if table is None else table[lab], crop_size)
    return finish_numpy(img, lab, None, contrast, normalize)


# ---- the same steps by PIL, in the order of the classes ------------------------------------------------------------------------------
def rotate_pil(img_u8, lab_u8, angle):
    from PIL import Image
    return (np.array(Image.fromarray(img_u8).rotate(angle, Image.BILINEAR)), np.array(Image.fromarray(lab_u8).rotate(angle, Image.NEAREST)))


def finish_pil(img, mask, blur=None, contrast=False, normalize=None):
    """RandomGaussianBlur (dataloaders.py:172-174) -> Contrast (:90-91) -> Normalize (:108-112) -> ToTensor (:128-130)."""
    from PIL import ImageEnhance, ImageFilter
    if blur is not None:
        img = img.filter(ImageFilter.GaussianBlur(radius=blur))
    if contrast:
        img = np.array(ImageEnhance.Contrast(img).enhance(2.0))
    if normalize is not None:
        img = normalize_reference(np.array(img), *normalize)
    return np.array(img).astype(np.float32).transpose((2, 0, 1)), np.array(mask).astype(np.float32)


def scale_crop_pil(img_u8, lab_u8, *, flip, jitter, degrees, scaled, pad, crop, blur, crop_size, fill=0, contrast=False,
                   normalize=None):
    """The PIL calls of RandomHorizontalFlip, ColorJitter, RandomRotate and RandomScaleCrop with the draws given, then finish_pil."""
    from PIL import Image, ImageOps
    img, mask = Image.fromarray(img_u8), Image.fromarray(lab_u8)
    if flip:                                                                     # :145-147
        img, mask = img.transpose(Image.FLIP_LEFT_RIGHT), mask.transpose(Image.FLIP_LEFT_RIGHT)
    for op, factor in (jitter or []):                                            # :596-660
        img = io.jitter_pil(img, op, factor)
    if degrees is not None:                                                      # :161-162
        img, mask = img.rotate(degrees, Image.BILINEAR), mask.rotate(degrees, Image.NEAREST)
    img, mask = img.resize(scaled, Image.BILINEAR), mask.resize(scaled, Image.NEAREST)       # :198-199
    padw, padh = pad
    if padw or padh:                                                             # :204-205
        img = ImageOps.expand(img, border=(0, 0, padw, padh), fill=0)
        mask = ImageOps.expand(mask, border=(0, 0, padw, padh), fill=fill)
    x1, y1 = crop
    box = (x1, y1, x1 + crop_size, y1 + crop_size)                               # :210-211
    return finish_pil(img.crop(box), mask.crop(box), blur, contrast, normalize)


def fix_scale_crop_pil(img_u8, lab_u8, crop_size, contrast=False, normalize=None, table=None):
    """FixScaleCrop (:446-462), then finish_pil; the label is encoded first, as the reference's __getitem__ does."""
    from PIL import Image
    img, mask = Image.fromarray(img_u8), Image.fromarray(lab_u8 if table is None else table[lab_u8])
    w, h = img.size
    ow, oh, x1, y1 = fix_scale_crop_geometry(w, h, crop_size)
    img, mask = img.resize((ow, oh), Image.BILINEAR), mask.resize((ow, oh), Image.NEAREST)
    box = (x1, y1, x1 + crop_size, y1 + crop_size)
    return finish_pil(img.crop(box), mask.crop(box), None, contrast, normalize)


def draw_kwargs(d) -> dict:
    """A ScaleCropDraw as the keyword arguments of scale_crop_numpy / scale_crop_pil."""
    return dict(flip=d.flip, jitter=d.jitter, degrees=d.degrees, scaled=d.scaled, pad=d.pad, crop=d.crop, blur=d.blur)


# ---- the recorded cases (tests/golden/input_aug.npz): a 30 x 40 (H x W) source, crop_size 24 ----------------------------------------
GOLDEN_CROP = 24
J1 = [("hue", -0.21), ("contrast", 1.13), ("brightness", 0.62), ("saturation", 0.9)]
GOLDEN_TRAIN = (
    # short_size 18 < 24: (ow, oh) = (24, 18), padded at the bottom by 6
    dict(flip=False, jitter=None, degrees=None, scaled=(24, 18), pad=(0, 6), crop=(0, 0), blur=None),
    dict(flip=True, jitter=None, degrees=None, scaled=(24, 18), pad=(0, 6), crop=(0, 0), blur=0.37, fill=255),
    # short_size 30: no padding
    dict(flip=False, jitter=None, degrees=None, scaled=(40, 30), pad=(0, 0), crop=(9, 4), blur=None),
    dict(flip=True, jitter=J1, degrees=-11.7, scaled=(53, 40), pad=(0, 0), crop=(20, 13), blur=None),          # rotation + jitter
    dict(flip=False, jitter=None, degrees=8.25, scaled=(32, 24), pad=(0, 0), crop=(5, 0), blur=0.61),           # rotation + blur
    dict(flip=True, jitter=None, degrees=180.0, scaled=(40, 30), pad=(0, 0), crop=(16, 6), blur=None),          # the 180 transpose
    dict(flip=False, jitter=None, degrees=-360.0, scaled=(48, 36), pad=(0, 0), crop=(3, 12), blur=None),        # angle % 360 == 0: a copy
    dict(flip=True, jitter=None, degrees=90.0, scaled=(20, 15), pad=(4, 9), crop=(0, 0), blur=0.9, fill=255),   # 90 on a non-square image: affine
    dict(flip=False, jitter=J1, degrees=3.0, scaled=(26, 20), pad=(0, 4), crop=(2, 0), blur=None, contrast=True, normalize=IMAGENET),
)
GOLDEN_EVAL = (
    dict(w=40, h=30, contrast=True, normalize=IMAGENET),        # w > h: (ow, oh) = (32, 24), x1 = 4
    dict(w=30, h=40, contrast=True, normalize=IMAGENET),        # h > w: (24, 32), y1 = 4
    dict(w=37, h=30, contrast=False, normalize=None),           # ow = 29: x1 = round(2.5) = 2, half to even
)


def golden_source(w: int = 40, h: int = 30):
    return sample(w, h, seed=2025)


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(FIXTURE) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture
