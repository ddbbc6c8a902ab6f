"""The reference's training transforms (main.py:409-419 transform_tr and the Resize / Crop compositions of its other training
sets) on the GPU, bit-exact with their PIL calls, and its frequency filters HPF / LPF / PHOT (dataloaders.py:24-79).

ResizeTransform (main.py:319-330, 499-507, 592-603) and CropTransform (main.py:764-773) reuse the kernels below: Pillow's BILINEAR
tables for the resampler, the assemble kernel with no padding, and the same flip, jitter and blur steps as TrainTransform.
hpf / lpf / phot (csrc/freq.hip) take the ToTensor layout float32 [3,H,W] or [B,3,H,W].
rotate / contrast, ScaleCropTransform, FixScaleCropTransform and CropTransform.p2 are the classes main.py keeps commented or never
composes (RandomRotate, RandomScaleCrop, RandomCrop_p2, FixScaleCrop, Contrast, Normalize): Image.rotate is csrc/input.hip's
affine_u8, Normalize is fused into the ToTensor store, the rest reuses the kernels below.

Reference: main.py:409-419 `transform_tr` = RandomHorizontalFlip -> ColorJitter -> RandomSizeAndCrop(crop_size,
crop_nopad=False, ignore_index=255) -> Resize(crop_size) -> RandomGaussianBlur -> ToTensor (dataloaders.py).  This module
does flip, ColorJitter, the BICUBIC / NEAREST rescale, the ImageOps.expand padding, the crop, the Gaussian blur and ToTensor on the device: uint8 image
and label map in, float32 [3,H,W] (0..255) and int64 [H,W] out, byte for byte what PIL produces (tests/test_input_gpu.py).
RandomGaussianBlur (:168-177) is included: its radius is random.random() < 1, for which ImageFilter.GaussianBlur is three
horizontal + three vertical passes of a 3-tap fixed-point box blur.  ColorJitter (dataloaders.py:596-660) is included: PIL's
ImageEnhance blends (Blend.c float arithmetic) and the RGB -> HSV -> RGB round trip of adjust_hue (Convert.c), per pixel,
the contrast mean reduced on the device; the Resize step is the identity here (the crop already has crop_size) and PIL
returns a copy for it.  One deviation is stated in oracle/input_oracle.py::hue_shift: `np.uint8(hue_factor * 255)` of a
negative factor is taken with the wrap-around of the numpy 1.x the reference pins.

The fixed-point coefficient tables of Pillow's resampler are built on the host exactly as Pillow builds them
(src/libImaging/Resample.c, double precision) and cached per (source size, destination size); the kernels
(csrc/input.hip) do the integer arithmetic."""
from __future__ import annotations

import math
import random as _random
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream

PRECISION_BITS = 32 - 8 - 2


def _bicubic_vec(x: np.ndarray) -> np.ndarray:
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _bilinear_vec(x: np.ndarray) -> np.ndarray:
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


_FILTERS = {"bicubic": (_bicubic_vec, 2.0), "bilinear": (_bilinear_vec, 1.0)}


@lru_cache(maxsize=256)
def _bicubic_tables(in_size: int, out_size: int):
    """Pillow precompute_coeffs(BICUBIC) + normalize_coeffs_8bpc -> (bounds int32 [out,2], coefs int32 [out,ksize])."""
    return _resample_tables(in_size, out_size, "bicubic")


@lru_cache(maxsize=256)
def _bilinear_tables(in_size: int, out_size: int):
    """Pillow precompute_coeffs(BILINEAR) + normalize_coeffs_8bpc: the image half of dataloaders.py:467-482 Resize."""
    return _resample_tables(in_size, out_size, "bilinear")


def _resample_tables(in_size: int, out_size: int, filt: str):
    """Pillow precompute_coeffs + normalize_coeffs_8bpc for `filt` -> (bounds int32 [out,2], coefs int32 [out,ksize]).
    Vectorised over the destination index with the same IEEE double operations in the same order as Pillow's scalar loop
    (the weight sum is a sequential cumsum, not numpy's pairwise sum); checked entry by entry against the scalar
    restatement in oracle/input_oracle.py::resample_tables (tests/test_input_cpu.py, tests/test_input_resize_cpu.py)."""
    fn, sup = _FILTERS[filt]
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = sup * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xx = np.arange(out_size, dtype=np.float64)
    center = 0.0 + (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)            # (int) truncates; the argument is > -1
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    t = np.arange(ksize, dtype=np.float64)[None, :]
    live = np.arange(ksize)[None, :] < xmax[:, None]
    w = np.where(live, fn((t + xmin[:, None] - center[:, None] + 0.5) * ss), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                                           # sequential adds, trailing zeros change nothing
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    one = float(1 << PRECISION_BITS)
    coefs = np.where(w < 0, -0.5 + w * one, 0.5 + w * one).astype(np.int32)     # C (int) cast: truncation
    coefs = np.where(live, coefs, 0).astype(np.int32)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    return bounds, np.ascontiguousarray(coefs)


@lru_cache(maxsize=256)
def _nearest_table(in_size: int, out_size: int) -> np.ndarray:
    """ImagingScaleAffine: xo = a/2, xin = (int)xo, xo += a (accumulated in double: a sequential cumsum)."""
    a = float(in_size) / out_size
    steps = np.full(out_size, a, dtype=np.float64)
    steps[0] = 0.0 + a * 0.5
    xo = np.cumsum(steps)
    return np.where(xo < 0.0, -1, xo.astype(np.int64)).astype(np.int32)


def _blur_weights(radius: float):
    """ImageFilter.GaussianBlur(radius) -> the (ww, fw) 24-bit weights of its three box-blur passes per axis, derived as
    Pillow derives them (BoxBlur.c _gaussian_blur_radius in C float arithmetic, then ww = (UINT32)(2^24 / (2 r + 1)),
    fw = (2^24 - (2 int(r) + 1) ww) / 2).  Only box radii below 1 (every radius = random.random() gives one)."""
    f32 = np.float32
    r = f32(radius)
    sigma2 = f32(f32(r * r) / f32(3))
    L = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * sigma2)))
    a = f32(a / f32(f32(6) * f32(sigma2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    fr = f32(l + a)
    if int(fr) != 0:
        raise _lib.MrfpHipError("GaussianBlur radius %r gives a box radius >= 1: only the reference's range [0, 1) is built" % radius)
    ww = int(f32(f32(1 << 24) / f32(fr * f32(2) + f32(1))))
    fw = ((1 << 24) - ww) // 2
    return ww, fw


_JITTER_OPS = {"brightness": 0, "contrast": 1, "saturation": 2, "hue": 3}


@dataclass
class Draw:
    flip: bool
    jitter: Optional[list]             # ColorJitter: [(op, factor), ...] in application order when its gate fired, else None
    scaled: Tuple[int, int]            # (w, h) after RandomSizeAndCrop's rescale
    pad: Tuple[int, int]               # (pad_w, pad_h) of ImageOps.expand on every side
    crop: Tuple[int, int]              # (x1, y1) in the padded image
    blur: Optional[float]              # GaussianBlur radius when its gate fired
    centroid: Optional[Tuple[int, int]] = None     # (c_x, c_y) the crop step was given (mirrored, scaled), None: a plain crop


def _draw_jitter(rng, np_rng, j) -> Optional[list]:
    """ColorJitter's draws (dataloaders.py:655 gate; when it fires, get_params :622-643: four uniform factors from numpy's global
    stream, then np.random.shuffle of the four transforms) -> [(op, factor), ...] in application order, or None."""
    if rng.random() < 0.5:
        ops = [("brightness", float(np_rng.uniform(max(0, 1 - j["brightness"]), 1 + j["brightness"]))),
               ("contrast", float(np_rng.uniform(max(0, 1 - j["contrast"]), 1 + j["contrast"]))),
               ("saturation", float(np_rng.uniform(max(0, 1 - j["saturation"]), 1 + j["saturation"]))),
               ("hue", float(np_rng.uniform(-j["hue"], j["hue"])))]
        np_rng.shuffle(ops)                                # consumes the stream as shuffling the four Lambdas does
        return ops
    return None


def _draw_blur(rng) -> Optional[float]:
    """RandomGaussianBlur (dataloaders.py:172-174): gate, then the radius."""
    return rng.random() if rng.random() < 0.5 else None


def _check_pair(name: str, img_u8: torch.Tensor, lab_u8: torch.Tensor):
    if not (img_u8.is_cuda and lab_u8.is_cuda and img_u8.dtype == torch.uint8 and lab_u8.dtype == torch.uint8):
        raise _lib.MrfpHipError("%s: uint8 CUDA tensors expected (there is no CPU path)" % name)
    H, W, C = img_u8.shape
    if C != 3 or tuple(lab_u8.shape) != (H, W):
        raise _lib.MrfpHipError("%s: image [H,W,3] and label [H,W] expected" % name)
    return H, W, img_u8.contiguous(), lab_u8.contiguous()


def _jitter(cur: torch.Tensor, jitter) -> torch.Tensor:
    """ColorJitter on the original-size image (per-pixel: commutes with the flip)."""
    if not jitter:
        return cur
    npix = cur.shape[0] * cur.shape[1]
    ws = torch.empty(16, dtype=torch.uint8, device=cur.device)
    for op, factor in jitter:
        nxt = torch.empty_like(cur)
        shift = int(factor * 255) & 255 if op == "hue" else 0
        call("mrfp_jitter_u8", ptr(cur), ptr(nxt), npix, _JITTER_OPS[op], float(factor), shift, ptr(ws), stream())
        cur = nxt
    return cur


def _resample(cur: torch.Tensor, H: int, W: int, sh: int, sw: int, xtab, ytab, flip: bool) -> torch.Tensor:
    """img.resize((sw, sh)) of the (unflipped) uint8 [H,W,3] image, mirrored when `flip`: xtab / ytab = (bounds, coefs, ksize)."""
    dev = cur.device
    if sw != W or flip:         # horizontal pass first (Pillow ImagingResample), reading the source mirrored when flipped
        # (at sw == W the coefficients are exactly (0, 1, 0): the pass is then a plain mirrored copy)
        bx, kx, ksx = xtab
        tmp = torch.empty((H, sw, 3), dtype=torch.uint8, device=dev)
        call("mrfp_resample_u8", ptr(cur), ptr(tmp), H, W, H, sw, 3, ptr(bx), ptr(kx), ksx, 0, int(flip), stream())
        cur = tmp
    if sh != H:
        by, ky, ksy = ytab
        tmp = torch.empty((sh, sw, 3), dtype=torch.uint8, device=dev)
        call("mrfp_resample_u8", ptr(cur), ptr(tmp), H, sw, sh, sw, 3, ptr(by), ptr(ky), ksy, 1, 0, stream())
        cur = tmp
    return cur


def _out_slot(t: Optional[torch.Tensor], shape, dtype, dev, what: str) -> torch.Tensor:
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not (t.is_cuda and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
        raise _lib.MrfpHipError("%s: contiguous %s CUDA tensor of shape %s expected, got %s %s" % (what, dtype, tuple(shape), t.dtype,
                                                                                                tuple(t.shape)))
    return t


def _assemble(cur: torch.Tensor, lab_u8: torch.Tensor, ty, tx, sh: int, sw: int, d: "Draw", Hc: int, Wc: int, ignore: int,
              out_img: Optional[torch.Tensor], out_lab: Optional[torch.Tensor]):
    """Pad + crop + (RandomGaussianBlur) + ToTensor of the scaled image `cur` [sh,sw,3]; the label is read from the ORIGINAL map
    through Pillow's nearest-neighbour tables ty [sh], tx [sw] (mirrored when d.flip) -> (float32 [3,Hc,Wc], int64 [Hc,Wc])."""
    H, W = lab_u8.shape
    dev = cur.device
    out_img = _out_slot(out_img, (3, Hc, Wc), torch.float32, dev, "out_img")
    out_lab = _out_slot(out_lab, (Hc, Wc), torch.int64, dev, "out_lab")
    blur = d.blur is not None and d.blur != 0.0          # PIL returns a copy for radius 0
    crop_u8 = torch.empty((Hc, Wc, 3), dtype=torch.uint8, device=dev) if blur else None
    call("mrfp_input_assemble", ptr(cur), ptr(lab_u8), ptr(ty), ptr(tx), sh, sw, H, W, int(d.flip), d.pad[0], d.pad[1],
         d.crop[0], d.crop[1], Hc, Wc, int(ignore), ptr(out_img), ptr(crop_u8), ptr(out_lab), stream())
    if blur:                                              # RandomGaussianBlur (dataloaders.py:168-177), then ToTensor
        ww, fw = _blur_weights(d.blur)
        a, b = crop_u8, torch.empty_like(crop_u8)
        for vertical in (0, 0, 0, 1, 1, 1):               # ImagingBoxBlur: three passes along x, then three along y
            call("mrfp_box_blur3_u8", ptr(a), ptr(b), Hc, Wc, 3, ww, fw, vertical, stream())
            a, b = b, a
        call("mrfp_u8hwc_to_f32chw", ptr(a), ptr(out_img), Hc, Wc, stream())
    return out_img, out_lab


def _cached(cache: dict, key, build):
    t = cache.get(key)
    if t is None:
        t = build()
        if len(cache) > 64:
            cache.clear()
        cache[key] = t
    return t


def _dev(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


class TrainTransform:
    """transform_tr of the reference (main.py:409-419) on the device."""

    def __init__(self, crop_size: int, scale_min: float = 0.5, scale_max: float = 2.0, ignore_index: int = 255):
        self.crop_size, self.scale_min, self.scale_max, self.ignore_index = int(crop_size), scale_min, scale_max, ignore_index
        self._dev_tables = {}

    JITTER = dict(brightness=0.5, hue=0.3, contrast=0.2, saturation=0.2)      # main.py:412

    def draw(self, w: int, h: int, rng=_random, np_rng=np.random, centroid=None) -> Draw:
        """Consumes python's `random` stream in the reference's order (dataloaders.py:145, 655, 421, 327-331, 172-174) and,
        when the ColorJitter gate fires, numpy's global stream as get_params does (:622-643: four uniform factors, then
        np.random.shuffle of the four transforms).
        centroid = (c_x, c_y), a point of the w x h source the crop has to cover (class-uniform sampling):
        RandomSizeAndCrop scales it as it scales the size, [int(c * scale_amt) for c in centroid] (:424-425), and RandomCrop draws
        x1 = randint(c_x - t, c_x), y1 = randint(c_y - t, c_y), each clipped to the padded image (:313-322) -- two randint calls
        whenever the crop is not the early return, also where the plain path draws none.  Kept as the reference has it: the
        centroid is NOT moved by ImageOps.expand's padding, and the interval is [c - t, c], so x1 <= c_x <= x1 + t (closed).
        This build's own rule: transform_tr flips before it crops and hands no centroid on, so when the flip fired the crop step
        gets w - 1 - c_x."""
        flip = rng.random() < 0.5
        jitter = _draw_jitter(rng, np_rng, self.JITTER)
        scale_amt = 1.0 * rng.uniform(self.scale_min, self.scale_max)
        sw, sh = int(w * scale_amt), int(h * scale_amt)
        if centroid is not None:
            c_x, c_y = centroid
            centroid = tuple(int(c * scale_amt) for c in ((w - 1 - c_x if flip else c_x), c_y))
        t = self.crop_size
        pad_w = pad_h = 0
        x1 = y1 = 0
        if not (sw == t and sh == t):
            pad_h = (t - sh) // 2 + 1 if t > sh else 0
            pad_w = (t - sw) // 2 + 1 if t > sw else 0
            W2, H2 = sw + 2 * pad_w, sh + 2 * pad_h
            if centroid is not None:
                x1 = min(W2 - t, max(0, rng.randint(centroid[0] - t, centroid[0])))
                y1 = min(H2 - t, max(0, rng.randint(centroid[1] - t, centroid[1])))
            else:
                x1 = 0 if W2 == t else rng.randint(0, W2 - t)
                y1 = 0 if H2 == t else rng.randint(0, H2 - t)
        blur = _draw_blur(rng)
        return Draw(flip, jitter, (sw, sh), (pad_w, pad_h), (x1, y1), blur, centroid)

    def _tables(self, dev, H, W, sh, sw):
        key = (str(dev), H, W, sh, sw)
        t = self._dev_tables.get(key)
        if t is None:
            bx, kx = _bicubic_tables(W, sw)
            by, ky = _bicubic_tables(H, sh)
            t = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
                      (bx, kx, by, ky, _nearest_table(W, sw), _nearest_table(H, sh))) + (kx.shape[1], ky.shape[1])
            if len(self._dev_tables) > 64:
                self._dev_tables.clear()
            self._dev_tables[key] = t
        return t

    def __call__(self, img_u8: torch.Tensor, lab_u8: torch.Tensor, d: Draw, out_img: Optional[torch.Tensor] = None,
                 out_lab: Optional[torch.Tensor] = None):
        """img_u8: uint8 [H,W,3], lab_u8: uint8 [H,W], both on the GPU -> (float32 [3,T,T], int64 [T,T])."""
        H, W, img_u8, lab_u8 = _check_pair("TrainTransform", img_u8, lab_u8)
        sw, sh = d.scaled
        bx, kx, by, ky, tx, ty, ksx, ksy = self._tables(img_u8.device, H, W, sh, sw)
        cur = _jitter(img_u8, d.jitter)
        cur = _resample(cur, H, W, sh, sw, (bx, kx, ksx), (by, ky, ksy), d.flip)
        return _assemble(cur, lab_u8, ty, tx, sh, sw, d, self.crop_size, self.crop_size, self.ignore_index, out_img, out_lab)


class ResizeTransform:
    """The Resize composition of the reference (Foggy Cityscapes main.py:319-330, BDD100k :499-507, Synthia :592-603):
    RandomHorizontalFlip -> ColorJitter -> Resize(size1, size2) -> RandomGaussianBlur -> ToTensor, on the device.
    Resize (dataloaders.py:467-482) hands (size1, size2) to PIL as (width, height) (the `# (h, w)` comment there is wrong):
    BILINEAR for the image, NEAREST for the label.  Output: float32 [3,size2,size1] (0..255) and int64 [size2,size1]."""

    JITTER = TrainTransform.JITTER

    def __init__(self, size1: int, size2: int):
        self.size1, self.size2 = int(size1), int(size2)
        self._dev_tables = {}

    def draw(self, w: int, h: int, rng=_random, np_rng=np.random) -> Draw:
        """python's `random`: flip, jitter gate, blur gate (+ radius); numpy's stream as ColorJitter.get_params when its gate
        fires.  (w, h), the source size, draws nothing here: it is taken for the same signature as TrainTransform.draw."""
        flip = rng.random() < 0.5
        jitter = _draw_jitter(rng, np_rng, self.JITTER)
        blur = _draw_blur(rng)
        return Draw(flip, jitter, (self.size1, self.size2), (0, 0), (0, 0), blur)

    def __call__(self, img_u8: torch.Tensor, lab_u8: torch.Tensor, d: Draw, out_img: Optional[torch.Tensor] = None,
                 out_lab: Optional[torch.Tensor] = None):
        """img_u8: uint8 [H,W,3], lab_u8: uint8 [H,W], both on the GPU -> (float32 [3,size2,size1], int64 [size2,size1]);
        out_img / out_lab: slots to write into (e.g. one sample of a batch)."""
        H, W, img_u8, lab_u8 = _check_pair("ResizeTransform", img_u8, lab_u8)
        sw, sh = self.size1, self.size2
        dev = img_u8.device
        bx, kx, by, ky, tx, ty = _cached(self._dev_tables, (str(dev), H, W), lambda: _dev(
            dev, *_bilinear_tables(W, sw), *_bilinear_tables(H, sh), _nearest_table(W, sw), _nearest_table(H, sh)))
        cur = _jitter(img_u8, d.jitter)
        cur = _resample(cur, H, W, sh, sw, (bx, kx, kx.shape[1]), (by, ky, ky.shape[1]), d.flip)
        return _assemble(cur, lab_u8, ty, tx, sh, sw, Draw(d.flip, d.jitter, (sw, sh), (0, 0), (0, 0), d.blur), sh, sw, 255,
                         out_img, out_lab)


class CropTransform:
    """The Crop composition of the reference (Mapillary, main.py:764-773): RandomHorizontalFlip -> ColorJitter ->
    RandomCrop_p(base_size, crop_size) -> RandomGaussianBlur -> ToTensor, on the device.  RandomCrop_p (dataloaders.py:216-234)
    crops `crop_size` wide and `base_size` tall at x0 = randint(0, w - crop_size), y0 = randint(0, h - base_size), drawn
    unconditionally (an image smaller than the crop raises ValueError in draw(), as it does there).
    Output: float32 [3,base_size,crop_size] (0..255) and int64 [base_size,crop_size]."""

    JITTER = TrainTransform.JITTER

    def __init__(self, base_size: int, crop_size: int):
        self.base_size, self.crop_size = int(base_size), int(crop_size)
        self._dev_tables = {}

    @classmethod
    def p2(cls, crop_w: int, crop_h: int) -> "CropTransform":
        """The same composition around RandomCrop_p2(crop_sizew, crop_sizeh) (dataloaders.py:236-255): RandomCrop_p with the
        width named first -- x0 = randint(0, w - crop_w), then y0 = randint(0, h - crop_h).  Output [3,crop_h,crop_w]."""
        return cls(crop_h, crop_w)

    def draw(self, w: int, h: int, rng=_random, np_rng=np.random) -> Draw:
        """python's `random`: flip, jitter gate, randint x0, randint y0, blur gate (+ radius); numpy's stream as
        ColorJitter.get_params when its gate fires."""
        flip = rng.random() < 0.5
        jitter = _draw_jitter(rng, np_rng, self.JITTER)
        x0 = rng.randint(0, w - self.crop_size)
        y0 = rng.randint(0, h - self.base_size)
        blur = _draw_blur(rng)
        return Draw(flip, jitter, (w, h), (0, 0), (x0, y0), blur)

    def __call__(self, img_u8: torch.Tensor, lab_u8: torch.Tensor, d: Draw, out_img: Optional[torch.Tensor] = None,
                 out_lab: Optional[torch.Tensor] = None):
        """img_u8: uint8 [H,W,3], lab_u8: uint8 [H,W], both on the GPU -> (float32 [3,base_size,crop_size],
        int64 [base_size,crop_size]); out_img / out_lab: slots to write into."""
        H, W, img_u8, lab_u8 = _check_pair("CropTransform", img_u8, lab_u8)
        x0, y0 = d.crop
        if not (0 <= x0 <= W - self.crop_size and 0 <= y0 <= H - self.base_size):
            raise _lib.MrfpHipError("CropTransform: a %dx%d crop at (%d, %d) leaves the %dx%d image" % (
                self.crop_size, self.base_size, x0, y0, W, H))
        dev = img_u8.device
        # identity tables: the flip is a mirrored copy through the resampler (coefficients exactly (0, 1, 0)), the label is read
        # through the identity nearest-neighbour tables, mirrored by the assemble kernel
        bx, kx, tx, ty = _cached(self._dev_tables, (str(dev), H, W), lambda: _dev(
            dev, *_bilinear_tables(W, W), _nearest_table(W, W), _nearest_table(H, H)))
        cur = _jitter(img_u8, d.jitter)
        cur = _resample(cur, H, W, H, W, (bx, kx, kx.shape[1]), None, d.flip)
        return _assemble(cur, lab_u8, ty, tx, H, W, Draw(d.flip, d.jitter, (W, H), (0, 0), (x0, y0), d.blur), self.base_size,
                         self.crop_size, 255, out_img, out_lab)


# ---- RandomRotate, RandomScaleCrop, FixScaleCrop, Contrast, Normalize (dataloaders.py:83-115, 153-165, 180-214, 439-465) -------
# Quirks of the reference that are kept as they are:
#   * RandomRotate passes no fillcolor: the corners a rotation uncovers are 0 in the image AND in the label -- class 0 (road),
#     not the ignore index;
#   * RandomScaleCrop pads on the right and at the bottom only (the content stays in the top-left corner), and only when
#     short_size < crop_size; the label padding is `fill`, whose default is 0;
#   * the reference never puts these classes into one Compose: the ORDER of ScaleCropTransform is this build's (the classic
#     DeepLab train composition dataloaders.py descends from), every step equals its class.
ROT_AFFINE, ROT_COPY, ROT_90, ROT_180, ROT_270 = 0, 1, 2, 3, 4        # the `mode` of mrfp_affine_u8


def rotate_plan(w: int, h: int, degrees: float):
    """Image.rotate(degrees) of a w x h image without expand / center / translate -> (mode, (m0..m5)): Pillow's dispatch to a copy
    or an exact transpose, else the matrix of its affine transform, with the same IEEE operations in the same order
    (Image.py: angle % 360.0, -math.radians, cos / sin rounded to 15 places, the centre (w / 2, h / 2) taken through the matrix and
    added back).  Raises MrfpHipError when a corner of the image maps to 32768 or beyond: Pillow's NEAREST transform then leaves
    the 16.16 fixed-point path (Geometry.c ImagingTransformAffine), and its double fallback is not built."""
    angle = degrees % 360.0
    if angle == 0:
        return ROT_COPY, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    if angle == 180:
        return ROT_180, (-1.0, 0.0, float(w), 0.0, -1.0, float(h))
    if angle in (90, 270) and w == h:
        return (ROT_90 if angle == 90 else ROT_270), (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    cx, cy = w / 2, h / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    x, y = -cx - 0, -cy - 0
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    for px, py in ((0, 0), (w, h), (0, h), (w, 0)):
        if not (abs(px * m[0] + py * m[1] + m[2]) < 32768.0 and abs(px * m[3] + py * m[4] + m[5]) < 32768.0):
            raise _lib.MrfpHipError("rotate: a corner of the %dx%d image leaves the 16.16 fixed-point range of Pillow's NEAREST "
                                    "transform (|coordinate| < 32768) at %r degrees" % (w, h, degrees))
    return ROT_AFFINE, tuple(m)


def _rotate(name: str, img_u8: torch.Tensor, lab_u8: torch.Tensor, degrees: float, flip: bool):
    """(flip, then) rotate: contiguous uint8 [H,W,3] / [H,W] on the device -> new tensors of the same shapes."""
    H, W = lab_u8.shape
    mode, m = rotate_plan(W, H, degrees)
    if mode == ROT_COPY and not flip:
        return img_u8, lab_u8                                # nothing downstream writes into its input
    out_img, out_lab = torch.empty_like(img_u8), torch.empty_like(lab_u8)
    call("mrfp_affine_u8", ptr(img_u8), ptr(lab_u8), ptr(out_img), ptr(out_lab), H, W, mode, int(flip), *m, stream())
    return out_img, out_lab


def rotate(img_u8: torch.Tensor, lab_u8: torch.Tensor, degrees: float):
    """RandomRotate's two calls (dataloaders.py:161-162): img.rotate(degrees, BILINEAR), mask.rotate(degrees, NEAREST), byte for
    byte.  uint8 [H,W,3] and [H,W] on the GPU -> the rotated pair (same shapes; uncovered corners are 0 in both)."""
    H, W, img_u8, lab_u8 = _check_pair("rotate", img_u8, lab_u8)
    out_img, out_lab = _rotate("rotate", img_u8, lab_u8, float(degrees), False)
    if out_img is img_u8:
        out_img, out_lab = img_u8.clone(), lab_u8.clone()    # Image.copy()
    return out_img, out_lab


def contrast(img_u8: torch.Tensor, factor: float = 2.0) -> torch.Tensor:
    """Contrast (dataloaders.py:83-93): ImageEnhance.Contrast(img).enhance(2.0), byte for byte -- the blend of every byte with
    the rounded mean of the L image, clipped (the contrast op of mrfp_jitter_u8).  uint8 [H,W,3] on the GPU -> the same."""
    if not (isinstance(img_u8, torch.Tensor) and img_u8.is_cuda and img_u8.dtype == torch.uint8 and img_u8.dim() == 3
            and img_u8.shape[2] == 3 and img_u8.numel() > 0):
        raise _lib.MrfpHipError("contrast: a uint8 CUDA tensor [H,W,3] expected (there is no CPU path)")
    return _jitter(img_u8.contiguous(), [("contrast", float(factor))])


def _normalize_arg(name: str, normalize):
    """normalize=(mean, std), three numbers each (the arguments of Normalize) -> six Python floats, or None."""
    if normalize is None:
        return None
    try:
        mean, std = normalize
        six = tuple(float(v) for v in mean) + tuple(float(v) for v in std)
    except (TypeError, ValueError):
        six = ()
    if len(six) != 6 or not all(math.isfinite(v) for v in six) or 0.0 in six[3:]:
        raise ValueError("%s: normalize=(mean, std) with three finite numbers each and no zero std expected" % name)
    return six


def _to_tensor(crop_u8: torch.Tensor, out_img: torch.Tensor, normalize):
    """(Normalize ->) ToTensor of a uint8 [Hc,Wc,3] image into out_img float32 [3,Hc,Wc]."""
    Hc, Wc = crop_u8.shape[0], crop_u8.shape[1]
    if normalize is None:
        call("mrfp_u8hwc_to_f32chw", ptr(crop_u8), ptr(out_img), Hc, Wc, stream())
    else:
        call("mrfp_u8hwc_to_f32chw_norm", ptr(crop_u8), ptr(out_img), Hc, Wc, *normalize, stream())


def _assemble_post(cur: torch.Tensor, lab_u8: torch.Tensor, ty, tx, sh: int, sw: int, flip: bool, pad, crop, Hc: int, Wc: int,
                   fill: int, blur, contrast_on: bool, normalize, out_img, out_lab):
    """Pad on the right / at the bottom + crop of the scaled image `cur` [sh,sw,3], then RandomGaussianBlur, Contrast, Normalize,
    ToTensor as asked.  mrfp_input_assemble pads both sides by (pad_x, pad_y): with the crop origin moved by the same amount its
    left / top border is never read, which leaves the one-sided padding of RandomScaleCrop."""
    H, W = lab_u8.shape
    dev = cur.device
    out_img = _out_slot(out_img, (3, Hc, Wc), torch.float32, dev, "out_img")
    out_lab = _out_slot(out_lab, (Hc, Wc), torch.int64, dev, "out_lab")
    blur_on = blur is not None and blur != 0.0               # PIL returns a copy for radius 0
    staged = blur_on or contrast_on or normalize is not None
    crop_u8 = torch.empty((Hc, Wc, 3), dtype=torch.uint8, device=dev) if staged else None
    call("mrfp_input_assemble", ptr(cur), ptr(lab_u8), ptr(ty), ptr(tx), sh, sw, H, W, int(flip), pad[0], pad[1],
         crop[0] + pad[0], crop[1] + pad[1], Hc, Wc, int(fill), ptr(out_img), ptr(crop_u8), ptr(out_lab), stream())
    if not staged:
        return out_img, out_lab
    if blur_on:                                              # RandomGaussianBlur (dataloaders.py:168-177)
        ww, fw = _blur_weights(blur)
        a, b = crop_u8, torch.empty_like(crop_u8)
        for vertical in (0, 0, 0, 1, 1, 1):
            call("mrfp_box_blur3_u8", ptr(a), ptr(b), Hc, Wc, 3, ww, fw, vertical, stream())
            a, b = b, a
        crop_u8 = a
    if contrast_on:                                          # Contrast (dataloaders.py:83-93)
        crop_u8 = _jitter(crop_u8, [("contrast", 2.0)])
    _to_tensor(crop_u8, out_img, normalize)
    return out_img, out_lab


@dataclass
class ScaleCropDraw:
    flip: bool
    jitter: Optional[list]             # ColorJitter: [(op, factor), ...] when asked and its gate fired, else None
    degrees: Optional[float]           # RandomRotate's angle, None without rotation
    scaled: Tuple[int, int]            # (ow, oh) of RandomScaleCrop's resize
    pad: Tuple[int, int]               # (padw, padh): right and bottom only
    crop: Tuple[int, int]              # (x1, y1) in the padded image
    blur: Optional[float]              # GaussianBlur radius when its gate fired


class ScaleCropTransform:
    """The classic DeepLab train composition from the classes of dataloaders.py, on the device:
    RandomHorizontalFlip (:139-150) -> ColorJitter (:596-660, when jitter=True, with the constants of the other compositions) ->
    RandomRotate(rotate_degree) (:153-165, when given) -> RandomScaleCrop(base_size, crop_size, fill) (:180-214) ->
    RandomGaussianBlur (:168-177) -> Contrast (:83-93, when contrast=True) -> Normalize(*normalize) (:95-115, when given) ->
    ToTensor (:118-136).  The reference never composes these itself: this ORDER is build-defined; every step is byte for byte
    (Normalize: bit for bit) what its class computes.
    RandomScaleCrop: short_size = randint(int(base_size * 0.5), int(base_size * 2.0)) becomes the short edge, the long one is
    int(1.0 * long * short_size / short); BILINEAR for the image, NEAREST for the label; when short_size < crop_size the result is
    padded on the RIGHT and at the BOTTOM only (image 0, label `fill`, default 0 as the class has it); then a crop_size square at
    x1 = randint(0, w - crop_size), y1 = randint(0, h - crop_size).  RandomRotate leaves uncovered corners 0 in image and label
    (class 0: the reference passes no fillcolor).  Output: float32 [3,crop_size,crop_size] (0..255 without normalize) and int64
    [crop_size,crop_size]."""

    JITTER = TrainTransform.JITTER

    def __init__(self, base_size: int, crop_size: int, fill: int = 0, rotate_degree: Optional[float] = None, jitter: bool = False,
                 contrast: bool = False, normalize=None):
        self.base_size, self.crop_size, self.fill = int(base_size), int(crop_size), int(fill)
        if self.crop_size <= 0 or int(self.base_size * 0.5) <= 0 or not 0 <= self.fill <= 255:
            raise ValueError("ScaleCropTransform: base_size >= 2, crop_size > 0 and fill in 0..255 expected")
        self.rotate_degree, self.jitter, self.contrast = rotate_degree, bool(jitter), bool(contrast)
        self.normalize = _normalize_arg("ScaleCropTransform", normalize)
        self._dev_tables = {}

    def draw(self, w: int, h: int, rng=_random, np_rng=np.random) -> ScaleCropDraw:
        """Consumes python's `random` in the order of the composition: flip gate (:145); with jitter=True the ColorJitter gate
        (:655) and, when it fires, numpy's stream as get_params does; with a rotate_degree uniform(-degree, degree) (:160);
        randint for short_size (:190), x1, y1 (:208-209); the blur gate and its radius (:172-174)."""
        flip = rng.random() < 0.5
        jitter = _draw_jitter(rng, np_rng, self.JITTER) if self.jitter else None
        degrees = rng.uniform(-1 * self.rotate_degree, self.rotate_degree) if self.rotate_degree is not None else None
        short_size = rng.randint(int(self.base_size * 0.5), int(self.base_size * 2.0))
        if h > w:
            ow = short_size
            oh = int(1.0 * h * ow / w)
        else:
            oh = short_size
            ow = int(1.0 * w * oh / h)
        padw = padh = 0
        t = self.crop_size
        if short_size < t:
            padh = t - oh if oh < t else 0
            padw = t - ow if ow < t else 0
        x1 = rng.randint(0, ow + padw - t)
        y1 = rng.randint(0, oh + padh - t)
        blur = _draw_blur(rng)
        return ScaleCropDraw(flip, jitter, degrees, (ow, oh), (padw, padh), (x1, y1), blur)

    def __call__(self, img_u8: torch.Tensor, lab_u8: torch.Tensor, d: ScaleCropDraw, out_img: Optional[torch.Tensor] = None,
                 out_lab: Optional[torch.Tensor] = None):
        """img_u8: uint8 [H,W,3], lab_u8: uint8 [H,W], both on the GPU -> (float32 [3,T,T], int64 [T,T]); out_img / out_lab: slots
        to write into.  The rotated label is materialised as uint8 and read through the nearest-neighbour tables."""
        H, W, img_u8, lab_u8 = _check_pair("ScaleCropTransform", img_u8, lab_u8)
        t = self.crop_size
        (sw, sh), (padw, padh), (x1, y1) = d.scaled, d.pad, d.crop
        if not (sw > 0 and sh > 0 and padw >= 0 and padh >= 0 and 0 <= x1 <= sw + padw - t and 0 <= y1 <= sh + padh - t):
            raise _lib.MrfpHipError("ScaleCropTransform: a %d crop at (%d, %d) leaves the %dx%d image padded by (%d, %d)" % (
                t, x1, y1, sw, sh, padw, padh))
        dev = img_u8.device
        bx, kx, by, ky, tx, ty = _cached(self._dev_tables, (str(dev), H, W, sh, sw), lambda: _dev(
            dev, *_bilinear_tables(W, sw), *_bilinear_tables(H, sh), _nearest_table(W, sw), _nearest_table(H, sh)))
        cur = _jitter(img_u8, d.jitter)                      # per pixel: commutes with the flip
        flip = d.flip
        if d.degrees is not None:                            # the rotation reads the source mirrored: the flip is done with it
            cur, lab_u8 = _rotate("ScaleCropTransform", cur, lab_u8, d.degrees, flip)
            flip = False
        cur = _resample(cur, H, W, sh, sw, (bx, kx, kx.shape[1]), (by, ky, ky.shape[1]), flip)
        return _assemble_post(cur, lab_u8, ty, tx, sh, sw, flip, (padw, padh), (x1, y1), t, t, self.fill, d.blur, self.contrast,
                              self.normalize, out_img, out_lab)


class FixScaleCropTransform:
    """The evaluation composition FixScaleCrop(crop_size) -> Contrast (when contrast=True) -> Normalize(*normalize) (when given)
    -> ToTensor (dataloaders.py:439-465, 83-115, 118-136; the lines commented in every transform_val of main.py) on the device.
    FixScaleCrop: the short edge goes to crop_size (w > h: oh = crop_size, ow = int(1.0 * w * oh / h); else the other way round),
    BILINEAR for the image and NEAREST for the label; the centre crop starts at int(round((ow - crop_size) / 2.)),
    int(round((oh - crop_size) / 2.)) -- Python's round-half-even.  Only the columns and rows the crop keeps are resampled.
    Called as the other evaluation transforms (harness.eval_batches): `encoder` encodes the label first, as the reference's
    __getitem__ does.  Output: float32 [3,crop_size,crop_size] and int64 [crop_size,crop_size]."""

    def __init__(self, crop_size: int, contrast: bool = False, normalize=None):
        self.crop_size, self.contrast = int(crop_size), bool(contrast)
        if self.crop_size <= 0:
            raise ValueError("FixScaleCropTransform: crop_size > 0 expected")
        self.normalize = _normalize_arg("FixScaleCropTransform", normalize)
        self._dev_tables = {}

    def geometry(self, w: int, h: int):
        """-> (ow, oh, x1, y1) of a w x h source: the scaled size and the crop origin in it."""
        t = self.crop_size
        if w > h:
            oh = t
            ow = int(1.0 * w * oh / h)
        else:
            ow = t
            oh = int(1.0 * h * ow / w)
        return ow, oh, int(round((ow - t) / 2.)), int(round((oh - t) / 2.))

    def __call__(self, img_u8: torch.Tensor, lab_u8: torch.Tensor, encoder: Optional[LabelEncoder] = None,
                 out_img: Optional[torch.Tensor] = None, out_lab: Optional[torch.Tensor] = None):
        H, W, img_u8, lab_u8 = _check_pair("FixScaleCropTransform", img_u8, lab_u8)
        dev, t = img_u8.device, self.crop_size

        def build():
            ow, oh, x1, y1 = self.geometry(W, H)
            bx, kx = _bilinear_tables(W, ow)
            by, ky = _bilinear_tables(H, oh)
            return _dev(dev, bx[x1:x1 + t], kx[x1:x1 + t], by[y1:y1 + t], ky[y1:y1 + t], _nearest_table(W, ow)[x1:x1 + t],
                        _nearest_table(H, oh)[y1:y1 + t]) + (ow, oh)
        bx, kx, by, ky, tx, ty, ow, oh = _cached(self._dev_tables, (str(dev), H, W), build)
        cur = img_u8
        if ow != W or t != W:       # the kept columns' rows of Pillow's tables (at ow == W PIL copies: the coefficients are (0, 1, 0))
            tmp = torch.empty((H, t, 3), dtype=torch.uint8, device=dev)
            call("mrfp_resample_u8", ptr(cur), ptr(tmp), H, W, H, t, 3, ptr(bx), ptr(kx), kx.shape[1], 0, 0, stream())
            cur = tmp
        if oh != H or t != H:
            tmp = torch.empty((t, t, 3), dtype=torch.uint8, device=dev)
            call("mrfp_resample_u8", ptr(cur), ptr(tmp), H, t, t, t, 3, ptr(by), ptr(ky), ky.shape[1], 1, 0, stream())
            cur = tmp
        if encoder is not None:
            lab_u8 = encoder(lab_u8)
        return _assemble_post(cur, lab_u8, ty, tx, t, t, False, (0, 0), (0, 0), t, t, 0, None, self.contrast, self.normalize,
                              out_img, out_lab)


# ---- frequency filters (dataloaders.py:24-79; csrc/freq.hip) --------------------------------------------------------------
@lru_cache(maxsize=32)
def _twiddles(n: int, device_str: str) -> torch.Tensor:
    """exp(-2 pi i t/n), t < n, built in double, stored as float32 (re, im) pairs."""
    t = np.arange(n, dtype=np.float64)
    tab = np.stack([np.cos(2 * np.pi * t / n), -np.sin(2 * np.pi * t / n)], 1).astype(np.float32)
    return torch.from_numpy(tab).to(device_str)


def _freq_args(name: str, x, out):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() in (3, 4) and x.shape[-3] == 3
            and x.numel() > 0):
        raise _lib.MrfpHipError("%s: a float32 CUDA tensor [3,H,W] or [B,3,H,W] expected, got %s" % (
            name, "%s %s %s" % (x.dtype, tuple(x.shape), x.device) if isinstance(x, torch.Tensor) else type(x).__name__))
    x = x.contiguous()
    B = 1 if x.dim() == 3 else x.shape[0]
    H, W = x.shape[-2], x.shape[-1]
    out = _out_slot(out, tuple(x.shape), torch.float32, x.device, name + ": out")
    dev = str(x.device)
    return x, out, B, H, W, _twiddles(H, dev), _twiddles(W, dev)


def _band(name: str, x, radius: float, out, high: bool):
    x, out, B, H, W, twH, twW = _freq_args(name, x, out)
    nb = int(_lib.lib().mrfp_band_filter_ws_bytes(B, H, W, float(radius)))
    if nb < 0:
        raise _lib.MrfpHipError("%s: radius %r on %dx%d images is not supported (0 <= radius < 33, H, W < 65536)" % (name, radius, H, W))
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    call("mrfp_band_filter", ptr(x), ptr(out), ptr(ws), ptr(twH), ptr(twW), B, H, W, float(radius), int(high), stream())
    return out


def hpf(x: torch.Tensor, radius: float = 16.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """HPF (dataloaders.py:24-45) on the ToTensor layout: x - Re(IDFT2(F * [fy^2 + fx^2 <= radius^2])) per channel plane.
    x: float32 CUDA [3,H,W] or [B,3,H,W] (any H, W) -> the same shape."""
    return _band("hpf", x, radius, out, True)


def lpf(x: torch.Tensor, radius: float = 16.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LPF (dataloaders.py:59-79): Re(IDFT2(F * [fy^2 + fx^2 < radius^2])) per channel plane (strict: the bins at distance
    exactly `radius` are removed by both filters, so hpf + lpf != x)."""
    return _band("lpf", x, radius, out, False)


def phot(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PHOT (dataloaders.py:47-57): Re(ifftn(F / |F|)) * 5 * 255 over the 3-D (H,W,3) spectrum.  H and W of the form
    2^a 3^b 5^c, <= 4096.  A zero bin gives NaN everywhere, as numpy does: a grey image (R = G = B) returns all NaN."""
    x, out, B, H, W, twH, twW = _freq_args("phot", x, out)
    nb = int(_lib.lib().mrfp_phot_ws_bytes(B, H, W))
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    call("mrfp_phot", ptr(x), ptr(out), ptr(ws), ptr(twH), ptr(twW), B, H, W, stream())
    return out


# ---- evaluation input path: label encoding, ToTensor-only validation, Mapillary's validation transform ----------------------
# Quirks of the reference that are kept as they are (DESIGN.md section 8 has the same list for users):
#   * encode_segmap rewrites the map in place, class id by class id: ids named in neither list stay what they are (Cityscapes
#     ids >= 34), and the -1 of the void lists never matches a uint8;
#   * BDD100kSegmentation defines encode_segmap but never calls it (its label files hold train ids): its table is the identity;
#   * Synthia starts from an all-255 map, Mapillary from a copy: unmapped ids are 255 there and unchanged here (ids >= 66);
#   * CenterCropPad pads the FULL deficit on both sides, takes its crop origin from the width before padding (a narrow image is
#     not centred, and the crop leaves the padded image on the left), and main.py:779 keeps its default ignore_index = 0:
#     padded label pixels are class 0 (road), not 255.
class LabelEncoder:
    """A label encoding of the reference as one 256-entry table, applied on the device (csrc/input.hip: label_lut_u8,
    label_encode_i64).  The reference rewrites the uint8 label map with one masked numpy pass per class id; the table is what
    those passes, replayed in the reference's statement order on arange(256), leave behind -- so the quirks of the in-place
    chain come out by construction instead of being restated.
      LabelEncoder.from_lists(void_classes, valid_classes, ignore_index): encode_segmap (main.py:106-112): in place, the voids
        first, then the valids in list order, valid_classes[i] -> i;
      LabelEncoder.from_map({id: train_id}, default): the copy-based loops; default None leaves unmapped ids unchanged
        (Mapillary, main.py:742-745), an int fills them (255 for Synthia, main.py:561-563)."""

    def __init__(self, table):
        table = np.asarray(table)
        if table.shape != (256,) or table.min() < 0 or table.max() > 255:
            raise ValueError("LabelEncoder: a table of 256 values in 0..255 expected")
        self.table = np.ascontiguousarray(table.astype(np.uint8))
        self.table.setflags(write=False)
        self._dev_tables = {}

    @classmethod
    def from_lists(cls, void_classes, valid_classes, ignore_index: int = 255) -> "LabelEncoder":
        t = np.arange(256, dtype=np.int64)           # wider than the map so that -1 compares as it does against a uint8: never equal
        for c in void_classes:
            t[t == c] = ignore_index
        for i, c in enumerate(valid_classes):
            t[t == c] = i
        return cls(t)

    @classmethod
    def from_map(cls, class_map: dict, default: Optional[int] = None) -> "LabelEncoder":
        src = np.arange(256, dtype=np.int64)
        t = src.copy() if default is None else np.full(256, default, dtype=np.int64)
        for k, v in class_map.items():
            t[src == k] = v
        return cls(t)

    def device_table(self, dev) -> torch.Tensor:
        return _cached(self._dev_tables, str(dev), lambda: _dev(dev, self.table.copy())[0])

    def inverse(self, fill: int = 0) -> "LabelEncoder":
        """The way back from train ids to the dataset's own ids, as a new LabelEncoder: inv[t] = the smallest id i with
        table[i] == t, for every t != 255 some id maps to; every other entry (255 included) is `fill`.  For the Cityscapes preset:
        0 -> 7, 1 -> 8, ... 18 -> 33, 255 -> fill.  Build-defined (the reference has no inverse); a many-to-one encoding such as
        Mapillary's returns the smallest of the ids that share a train id."""
        fill = int(fill)
        if not 0 <= fill <= 255:
            raise ValueError("LabelEncoder.inverse: fill must be in 0..255, got %r" % (fill,))
        inv = np.full(256, fill, dtype=np.int64)
        for i in range(255, -1, -1):                 # descending: the smallest id is written last
            t = int(self.table[i])
            if t != 255:
                inv[t] = i
        return LabelEncoder(inv)

    def _arg(self, name: str, lab_u8: torch.Tensor) -> torch.Tensor:
        if not (isinstance(lab_u8, torch.Tensor) and lab_u8.is_cuda and lab_u8.dtype == torch.uint8):
            raise _lib.MrfpHipError("LabelEncoder%s: a uint8 CUDA tensor expected (there is no CPU path)" % name)
        return lab_u8.contiguous()

    def __call__(self, lab_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 label map of any shape -> the encoded uint8 map (out may be lab_u8 itself: in place)."""
        lab_u8 = self._arg("", lab_u8)
        out = _out_slot(out, tuple(lab_u8.shape), torch.uint8, lab_u8.device, "LabelEncoder: out")
        if lab_u8.numel():                                   # (an empty tensor has no address to hand over)
            call("mrfp_label_lut_u8", ptr(lab_u8), ptr(out), lab_u8.numel(), ptr(self.device_table(lab_u8.device)), stream())
        return out

    def to_int64(self, lab_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 label map -> the encoded map as int64 (what ToTensor hands the loss / the histogram), in one pass."""
        lab_u8 = self._arg(".to_int64", lab_u8)
        return _to_int64(lab_u8, self.device_table(lab_u8.device), out, "LabelEncoder.to_int64: out")


def _to_int64(lab_u8: torch.Tensor, table: Optional[torch.Tensor], out: Optional[torch.Tensor], what: str) -> torch.Tensor:
    out = _out_slot(out, tuple(lab_u8.shape), torch.int64, lab_u8.device, what)
    if lab_u8.numel():
        call("mrfp_label_encode_i64", ptr(lab_u8), ptr(table), ptr(out), lab_u8.numel(), stream())
    return out


class RelaxedBoundaryTarget:
    """The reference's RelaxedBoundaryLossToTensor (transforms/transforms.py:75-124) on the device: an int64 label map [H,W] or
    [B,H,W] -> the relaxed target as int32 words of the same shape (csrc/relax.hip, mrfp_relax_labels): bit c =
    class c occurs within `border` pixels, bit num_classes = ignore or the outside of the image does.  border / strict_classes None:
    cfg.BORDER_WINDOW / cfg.STRICTBORDERCLASS, read at call time as the reference's transform reads them.  The reference's
    REDUCE_BORDER_ITER branch is not built.  to_multihot(words) gives the reference's uint8 [C+1,H,W] layout."""

    def __init__(self, num_classes, ignore_id=255, border=None, strict_classes=None):
        self.num_classes, self.ignore_id = int(num_classes), int(ignore_id)
        if 0 <= self.ignore_id < self.num_classes:
            raise ValueError("RelaxedBoundaryTarget: ignore_id %d is a class of 0..%d" % (self.ignore_id, self.num_classes - 1))
        self.border, self.strict_classes = border, strict_classes

    def __call__(self, label: torch.Tensor) -> torch.Tensor:
        from . import ops
        from .config import cfg
        border = cfg.BORDER_WINDOW if self.border is None else self.border
        strict = cfg.STRICTBORDERCLASS if self.strict_classes is None else self.strict_classes
        if not (isinstance(label, torch.Tensor) and label.dim() in (2, 3)):
            raise _lib.MrfpHipError("RelaxedBoundaryTarget: an int64 label map [H,W] or [B,H,W] expected")
        words = ops.relax_labels(label if label.dim() == 3 else label.unsqueeze(0), self.num_classes, border, strict)
        return words if label.dim() == 3 else words[0]

    def to_multihot(self, words: torch.Tensor) -> torch.Tensor:
        """int32 words [H,W] / [B,H,W] -> uint8 [C+1,H,W] / [B,C+1,H,W], plane c = bit c (for callers that want the reference's bytes;
        the loss takes the words)."""
        bits = torch.arange(self.num_classes + 1, dtype=torch.int32, device=words.device).view(-1, 1, 1)
        return ((words.unsqueeze(-3) >> bits) & 1).to(torch.uint8)


# Label ids of the 19 evaluation classes, in train-id order (road, sidewalk, building, wall, fence, pole, traffic light, traffic
# sign, vegetation, terrain, sky, person, rider, car, truck, bus, train, motorcycle, bicycle), per label set.
_CITYSCAPES_IDS = (7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33)      # Cityscapes labelIds; GTAV shares them
_SYNTHIA_IDS = (3, 4, 2, 21, 5, 7, 15, 9, 6, 16, 1, 10, 17, 8, 18, 19, 20, 12, 11)               # SYNTHIA-RAND-CITYSCAPES
_MAPILLARY_IDS = ((13, 24, 41), (2, 15), (17,), (6,), (3,), (45, 47), (48,), (50,), (30,), (29,), (27,), (19,), (20, 21, 22), (55,),
                  (61,), (54,), (58,), (57,), (52,))                                              # Mapillary Vistas v1.2 (66 ids)


def _preset_table(groups, nvoid: Optional[int], default: Optional[int] = None) -> np.ndarray:
    """ids 0..nvoid-1 that belong to no class -> 255, every other unmapped id `default` (None: unchanged); groups[i] -> i."""
    t = np.arange(256) if default is None else np.full(256, default)
    if nvoid:
        t[:nvoid] = 255
    for i, g in enumerate(groups):
        t[list(g) if isinstance(g, tuple) else g] = i
    return t


_PRESETS = {
    # encode_segmap with the Cityscapes lists (main.py:69-70, 161-162, 257-258): labelIds 0..33; 34 and above are in neither list
    "Cityscapes": lambda: _preset_table(_CITYSCAPES_IDS, 34),
    "RainyCityscapes": lambda: _preset_table(_CITYSCAPES_IDS, 34),
    "Foggy_Cityscapes": lambda: _preset_table(_CITYSCAPES_IDS, 34),
    "GTAV": lambda: _preset_table(_CITYSCAPES_IDS, 35),                # main.py:358 adds 34 to the voids
    # main.py:470-471: the *_train_id.png files go to the transform as they are; the encode_segmap of that class (whose valid
    # list :448 differs, as the comment at :70 says) is never called
    "BDD100k": lambda: _preset_table((), None),
    "Synthia": lambda: _preset_table(_SYNTHIA_IDS, None, 255),         # main.py:561-563: an all-255 map, the 19 ids written in
    "Mapillary": lambda: _preset_table(_MAPILLARY_IDS, 66),            # main.py:635-726, 742-745: 66 ids, a copy for the rest
}


def label_encoder(name: str) -> LabelEncoder:
    """The label encoding of one dataset class of the reference's main.py, by the reference's class name
    (CityscapesSegmentation, RainyCityscapesSegmentation, Foggy_CityscapesSegmentation, GTAVSegmentation, BDD100kSegmentation,
    SynthiaSegmentation, MapillarySegmentation; the `Segmentation` suffix may be left out)."""
    key = name[:-len("Segmentation")] if name.endswith("Segmentation") else name
    if key not in _PRESETS:
        raise KeyError("label_encoder: %r is none of %s" % (name, ", ".join(k + "Segmentation" for k in _PRESETS)))
    return LabelEncoder(_PRESETS[key]())


class EvalTransform:
    """The ToTensor-only validation sample (main.py:134-144 and the transform_val of every dataset class but Mapillary;
    dataloaders.py:118-136): uint8 [H,W,3] image and uint8 [H,W] label map on the GPU -> float32 [3,H,W] (0..255, no /255) and
    int64 [H,W], the label encoded by `encoder` in the same pass (the reference encodes in __getitem__, before the transform)."""

    def __call__(self, img_u8: torch.Tensor, lab_u8: torch.Tensor, encoder: Optional[LabelEncoder] = None,
                 out_img: Optional[torch.Tensor] = None, out_lab: Optional[torch.Tensor] = None):
        H, W, img_u8, lab_u8 = _check_pair("EvalTransform", img_u8, lab_u8)
        dev = img_u8.device
        out_img = _out_slot(out_img, (3, H, W), torch.float32, dev, "out_img")
        call("mrfp_u8hwc_to_f32chw", ptr(img_u8), ptr(out_img), H, W, stream())
        table = encoder.device_table(dev) if encoder is not None else None
        return out_img, _to_int64(lab_u8, table, out_lab, "out_lab")


class ResizeHeightCenterCropPad:
    """Mapillary's validation composition (main.py:775-783): ResizeHeight(eval_size) -> CenterCropPad(eval_size) -> ToTensor
    (dataloaders.py:339-394, 118-136) on the device, byte for byte what PIL gives, the reference's behaviour kept as it is:
      * target_w = int(w / h * eval_size), in floating point as written; BICUBIC for the image, NEAREST for the label;
      * a narrow result (target_w < eval_size) is padded by the FULL deficit on BOTH sides, and the crop origin
        int(round((target_w - eval_size) / 2.)) (Python's round-half-even) is taken from the width BEFORE padding: it is then
        negative, the crop leaves the padded image on the left (those pixels are 0 in image and label, as Image.crop gives) and
        the content is not centred -- 12 wide at eval_size 16: 2 outside columns, 4 pad columns, the first 10 content columns;
      * padded label pixels take `ignore_index`, whose default is 0 as CenterCropPad's is; main.py:779 does not override it, so
        in the reference's Mapillary evaluation the padding counts as class 0 (road).  That is mirrored, not corrected: pass
        ignore_index=255 for padding the loss and the histogram ignore.
    Only the columns that survive the crop are resampled (a wide image loses target_w - eval_size columns before the horizontal
    pass instead of after it).  `encoder`: the table is applied while the assemble kernel reads the label -- raw dataset ids in,
    train ids out, no intermediate map.  Output: float32 [3,eval_size,eval_size] (0..255) and int64 [eval_size,eval_size]."""

    def __init__(self, eval_size: int, ignore_index: int = 0):
        self.eval_size, self.ignore_index = int(eval_size), int(ignore_index)
        if self.eval_size <= 0 or not 0 <= self.ignore_index <= 255:
            raise ValueError("ResizeHeightCenterCropPad: eval_size > 0 and ignore_index in 0..255 expected")
        self._dev_tables = {}

    def geometry(self, w: int, h: int):
        """-> (target_w, pad_x, x1) of a w x h source: the scaled width, ImageOps.expand's border on each side and the crop
        origin in the padded image (vertically the scaled image has eval_size rows: no padding, origin 0)."""
        t = self.eval_size
        tw = int(w / h * t)
        if tw <= 0:
            raise _lib.MrfpHipError("ResizeHeightCenterCropPad: a %dx%d image scales to width 0 (PIL refuses it too)" % (w, h))
        return tw, (t - tw if tw < t else 0), int(round((tw - t) / 2.))

    def _tables(self, dev, H: int, W: int):
        def build():
            t = self.eval_size
            tw, pad_x, x1 = self.geometry(W, H)
            c0, c1 = (x1, x1 + t) if tw >= t else (0, tw)          # the scaled columns the crop keeps (no padding when tw >= t)
            bx, kx = _bicubic_tables(W, tw)
            by, ky = _bicubic_tables(H, t)
            tabs = _dev(dev, bx[c0:c1], kx[c0:c1], by, ky, _nearest_table(W, tw)[c0:c1], _nearest_table(H, t))
            return tabs + (kx.shape[1], ky.shape[1], tw, c1 - c0, pad_x, x1 - c0 if tw >= t else x1)
        return _cached(self._dev_tables, (str(dev), H, W), build)

    def __call__(self, img_u8: torch.Tensor, lab_u8: torch.Tensor, encoder: Optional[LabelEncoder] = None,
                 out_img: Optional[torch.Tensor] = None, out_lab: Optional[torch.Tensor] = None):
        H, W, img_u8, lab_u8 = _check_pair("ResizeHeightCenterCropPad", img_u8, lab_u8)
        dev, t = img_u8.device, self.eval_size
        bx, kx, by, ky, tx, ty, ksx, ksy, tw, ncol, pad_x, x1 = self._tables(dev, H, W)
        out_img = _out_slot(out_img, (3, t, t), torch.float32, dev, "out_img")
        out_lab = _out_slot(out_lab, (t, t), torch.int64, dev, "out_lab")
        cur = img_u8
        if tw != W or ncol != W:    # horizontal pass over the kept columns only: their rows of Pillow's tables (at tw == W, where
            # PIL returns a copy, the coefficients are exactly (0, 1, 0, 0): the pass then copies the kept columns)
            tmp = torch.empty((H, ncol, 3), dtype=torch.uint8, device=dev)
            call("mrfp_resample_u8", ptr(cur), ptr(tmp), H, W, H, ncol, 3, ptr(bx), ptr(kx), ksx, 0, 0, stream())
            cur = tmp
        if t != H:
            tmp = torch.empty((t, ncol, 3), dtype=torch.uint8, device=dev)
            call("mrfp_resample_u8", ptr(cur), ptr(tmp), H, ncol, t, ncol, 3, ptr(by), ptr(ky), ksy, 1, 0, stream())
            cur = tmp
        table = encoder.device_table(dev) if encoder is not None else None
        call("mrfp_eval_assemble", ptr(cur), ptr(lab_u8), ptr(ty), ptr(tx), t, ncol, H, W, pad_x, 0, x1, 0, t, t, self.ignore_index,
             ptr(table), ptr(out_img), ptr(out_lab), stream())
        return out_img, out_lab


# ---- class-uniform sampling (reference config.py:53-64 CLASS_UNIFORM_PCT; csrc/sample.hip) ----------------
# The reference carries the consumer half -- RandomCrop / RandomSizeAndCrop take a centroid (dataloaders.py:280-337, 407-434;
# TrainTransform.draw(centroid=) above) -- and not the producer (`uniform.py` of the DeepLabV3+ lineage): the rule of
# mrfp_tile_class_sums (include/mrfp_hip.h) and of ClassUniformSampler.epoch is therefore build-defined.
def _label_table(table, dev) -> Optional[torch.Tensor]:
    if table is None:
        return None
    if isinstance(table, LabelEncoder):
        return table.device_table(dev)
    if not (isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.uint8 and tuple(table.shape) == (256,)
            and table.is_contiguous()):
        raise _lib.MrfpHipError("tile_class_centroids: table must be a LabelEncoder or its 256-entry uint8 CUDA tensor")
    return table


def tile_class_centroids(lab_u8: torch.Tensor, num_classes: int, tile: int = 1024, table=None, partial_tiles: bool = False):
    """Per image tile and class: pixel count, coordinate sums and integer centroid, in one pass over uint8 label maps on the device.
    lab_u8: uint8 CUDA [H,W] or [B,H,W]; table: a LabelEncoder or its 256-entry uint8 device tensor, applied as the labels are read (the
    published id2trainid step).  -> (sums int64 [B,nty,ntx,C,3] = n, sum(x - x0), sum(y - y0); cent int32 [B,nty,ntx,C,2] = cx, cy in
    image coordinates, -1, -1 where the class has no pixel in the tile).  partial_tiles=False is the published rule (whole tiles only: the
    ragged right and bottom strips are never looked at, an image smaller than a tile is refused); True counts the ragged tiles too."""
    if not (isinstance(lab_u8, torch.Tensor) and lab_u8.is_cuda and lab_u8.dtype == torch.uint8 and lab_u8.dim() in (2, 3)
            and lab_u8.numel() > 0):
        raise _lib.MrfpHipError("tile_class_centroids: lab_u8 must be a non-empty uint8 CUDA tensor [H,W] or [B,H,W] (there is no CPU "
                                "path), got %s" % ("%s %s %s" % (lab_u8.dtype, tuple(lab_u8.shape), lab_u8.device)
                                                   if isinstance(lab_u8, torch.Tensor) else type(lab_u8).__name__))
    C, tile, partial = int(num_classes), int(tile), int(bool(partial_tiles))
    lab_u8 = lab_u8.contiguous()
    B = 1 if lab_u8.dim() == 2 else lab_u8.shape[0]
    H, W = lab_u8.shape[-2], lab_u8.shape[-1]
    dev = lab_u8.device
    table = _label_table(table, dev)
    count = _lib.lib().mrfp_tile_count
    nty, ntx = max(int(count(H, tile, partial)), 0), max(int(count(W, tile, partial)), 0)      # (the entry refuses what is wrong, by name)
    sums = _out_slot(None, (B, nty, ntx, max(C, 0), 3), torch.int64, dev, "sums")
    cent = _out_slot(None, (B, nty, ntx, max(C, 0), 2), torch.int32, dev, "cent")
    call("mrfp_tile_class_sums", ptr(lab_u8), ptr(table), B, H, W, C, tile, partial, ptr(sums), ptr(cent), stream())
    return sums, cent


class ClassCentroids:
    """The centroid table of a training set: by_class[c] = [(image_index, (cx, cy)), ...], one entry per (image, tile) in which class c
    occurs, in (image, tile-row, tile-column) order.  tile=None reads cfg.CLASS_UNIFORM_TILE when maps are added; encoder: the
    LabelEncoder the raw label ids go through first.  This is preprocessing, once per training set, not the training step:
    add() makes one device -> host copy of the small centroid table per call."""

    def __init__(self, num_classes: int, tile: Optional[int] = None, partial_tiles: bool = False, encoder: Optional[LabelEncoder] = None):
        self.num_classes, self.tile, self.partial_tiles, self.encoder = int(num_classes), tile, bool(partial_tiles), encoder
        if not 1 <= self.num_classes <= 256:
            raise ValueError("ClassCentroids: num_classes must be in 1..256, got %r" % (num_classes,))
        self.by_class = [[] for _ in range(self.num_classes)]

    def add(self, first_index: int, lab_u8: torch.Tensor):
        """One label map [H,W], or a batch [B,H,W] of equal-sized ones that are images first_index .. first_index + B - 1."""
        from .config import cfg
        tile = cfg.CLASS_UNIFORM_TILE if self.tile is None else self.tile
        _, cent = tile_class_centroids(lab_u8, self.num_classes, tile, self.encoder, self.partial_tiles)
        host = cent.cpu().numpy()                            # [B,nty,ntx,C,2]
        b, ty, tx, c = np.nonzero(host[..., 0] >= 0)         # row-major: (image, tile-row, tile-column) order within a class
        for bi, yi, xi, ci in zip(b.tolist(), ty.tolist(), tx.tolist(), c.tolist()):
            cx, cy = host[bi, yi, xi, ci].tolist()
            self.by_class[ci].append((int(first_index) + bi, (cx, cy)))

    def state_dict(self):
        """Plain lists and ints (JSON-able, as the published form caches its centroid files)."""
        return {"num_classes": self.num_classes, "tile": self.tile, "partial_tiles": self.partial_tiles,
                "by_class": [[[i, [cx, cy]] for i, (cx, cy) in lst] for lst in self.by_class]}

    def load_state_dict(self, sd):
        if int(sd["num_classes"]) != self.num_classes or len(sd["by_class"]) != self.num_classes:
            raise ValueError("ClassCentroids: the state holds %r classes, this table %d" % (sd["num_classes"], self.num_classes))
        self.tile, self.partial_tiles = sd["tile"], bool(sd["partial_tiles"])
        self.by_class = [[(int(i), (int(c[0]), int(c[1]))) for i, c in lst] for lst in sd["by_class"]]


class ClassUniformSampler:
    """An epoch that draws every class equally often (cfg.CLASS_UNIFORM_PCT; build-defined).
    per_class = int(n_images * pct / C), n_rand = n_images - per_class * C.  pick(alist, k): idx = arange(len); np_rng.shuffle(idx);
    [alist[idx[i % len]] for i in range(k)] -- a short list wraps around.  epoch(): pick(range(n_images), n_rand) as
    (index, None, None), then for c ascending pick(by_class[c], per_class) as (index, centroid, c) for every class that has an entry
    (a class that is nowhere adds nothing: the epoch is shorter), then one np_rng.shuffle(items) when `shuffle`.  pct = 0 is a
    permutation of the images.  centroids: a ClassCentroids or its by_class list; pct=None reads cfg.CLASS_UNIFORM_PCT per epoch."""

    def __init__(self, n_images: int, centroids, pct: Optional[float] = None):
        self.n_images = int(n_images)
        self.by_class = centroids.by_class if isinstance(centroids, ClassCentroids) else list(centroids)
        if self.n_images < 1 or not self.by_class:
            raise ValueError("ClassUniformSampler: n_images >= 1 and at least one class expected")
        if pct is not None and not 0.0 <= float(pct) <= 1.0:
            raise ValueError("ClassUniformSampler: pct must be in [0, 1], got %r" % (pct,))
        self.pct = pct

    @staticmethod
    def pick(alist, k: int, np_rng=np.random):
        idx = np.arange(len(alist))
        np_rng.shuffle(idx)
        return [alist[int(idx[i % len(alist)])] for i in range(k)]

    def epoch(self, np_rng=np.random, shuffle: bool = True):
        """-> [(index, centroid | None, class_id | None), ...]"""
        from .config import cfg
        pct = float(cfg.CLASS_UNIFORM_PCT if self.pct is None else self.pct)
        C = len(self.by_class)
        per_class = int(self.n_images * pct / C)
        n_rand = self.n_images - per_class * C
        items = [(i, None, None) for i in self.pick(range(self.n_images), n_rand, np_rng)]
        for c, entries in enumerate(self.by_class):
            if entries:
                items += [(i, cen, c) for i, cen in self.pick(entries, per_class, np_rng)]
        if shuffle:
            np_rng.shuffle(items)
        return items

    @staticmethod
    def shard(items, rank: int, world: int):
        """items[rank::world], cut to len(items) // world: every rank builds the same epoch from the same seed and takes its share."""
        return items[rank::world][:len(items) // world]
