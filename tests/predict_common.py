"""Shared by test_predict_cpu.py, test_predict_gpu.py and test_predict_golden.py: the seeded inputs of the prediction path
(ops.upsample_argmax, include/mrfp_hip.h: mrfp_upsample_argmax), the fp32 numpy restatement of the kernel's interpolation -- an
operation-for-operation copy of csrc/loss_common.hpp::up_logits, rounded to the storage type as the kernel rounds -- and the fp64
evaluation of the same interpolation that decides which pixels an fp64 comparison may look at."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "predict.npz")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
# relative loss bounds of the training kernels with the same arithmetic (tests/test_loss_gpu.py, tests/test_relaxed_gpu.py)
LOSS_TOL = {F32: 1e-5, BF16: 2e-3, F16: 2e-3}
IGNORE = 255

# (name, B, Hi, Wi, H, W, C, ld); ld None: the smallest legal pitch (C rounded up to the 16-byte chunk of the dtype)
SMALL_CASES = [
    ("c19_ld32", 2, 5, 7, 17, 26, 19, 32),
    ("c3_minpitch", 2, 9, 6, 33, 21, 3, None),
    ("c21_ld24", 2, 6, 5, 24, 20, 21, 24),
    ("c33_ld64", 1, 4, 4, 9, 9, 33, 64),
    ("identity", 1, 6, 6, 6, 6, 19, 32),
    ("src1x1", 2, 1, 1, 4, 4, 19, 32),
    ("src3x1", 1, 3, 1, 3, 9, 19, 32),
]
# capped grids: a workgroup walks several trips (1 x 768^2: 2048 workgroups x 1.1 trips; 3 x 456^2: 682 per image x 1.2)
CAPPED_CASES = [
    ("cap_768", 1, 192, 192, 768, 768, 19, 32),
    ("cap_3x456", 3, 24, 24, 456, 456, 19, 32),
]
CASES = SMALL_CASES + CAPPED_CASES
# pixels whose two largest fp64 scores are closer than this are left out of an fp64 comparison ...
GAP = {F32: lambda top: np.full_like(top, 2e-3), BF16: lambda top: 2.0 ** -7 * np.abs(top), F16: lambda top: 2.0 ** -10 * np.abs(top)}
# ... and no more than this share of a case's pixels may be (conditions on the inputs, asserted on the CPU)
GAP_CAP = {F32: 0.01, BF16: 0.05, F16: 0.01}


def dname(d):
    return str(d).replace("torch.", "")


def pitch(case, dtype):
    ld = case[7]
    if ld is None:
        epc = 16 // torch.empty(0, dtype=dtype).element_size()
        ld = (case[6] + epc - 1) // epc * epc
    return ld


@functools.lru_cache(maxsize=None)
def scores(name, dtype):
    """-> host tensor [B,Hi,Wi,ld] of `dtype`: 4 * randn class scores rounded to the dtype; the pad channels c >= C hold 1e30 (the
    largest finite value in float16) and must never show."""
    case = next(c for c in CASES if c[0] == name)
    _, B, Hi, Wi, H, W, C, _ = case
    ld = pitch(case, dtype)
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 7 * DTYPES.index(dtype))
    z = (4.0 * torch.randn(B, Hi, Wi, ld, generator=g)).to(dtype)
    z[..., C:] = 65504.0 if dtype == F16 else 1e30
    return z


def to_device(z, dev):
    """host [B,Hi,Wi,ld] -> logical [B,ld,Hi,Wi] over the same NHWC storage on the device"""
    return z.to(dev).permute(0, 3, 1, 2)


def labels(name, B, H, W, C):
    """int64 [B,H,W]: uniform classes, ~10 % 255, and some -1, C and 200 (all ignored)."""
    g = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    y = torch.randint(0, C, (B, H, W), generator=g)
    r = torch.rand(B, H, W, generator=g)
    y[r < 0.10] = IGNORE
    y[(r >= 0.10) & (r < 0.13)] = -1
    y[(r >= 0.13) & (r < 0.16)] = C
    y[(r >= 0.16) & (r < 0.19)] = 200
    return y


def _taps(n_in, n_out):
    """up_scale + the tap arithmetic of up_logits along one axis, in float32"""
    s = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    f = s * np.arange(n_out, dtype=np.float32)
    i0 = f.astype(np.int32)
    i1 = i0 + (i0 < n_in - 1)
    l1 = f - i0.astype(np.float32)
    l0 = np.float32(1.0) - l1
    return i0, i1, l0, l1


def restated_z(z, C, H, W):
    """The kernel's z in float32 numpy: z [B,Hi,Wi,ld] host tensor of the storage dtype -> float32 [B,H,W,C], every operation in
    float32 in up_logits' order (numpy contracts nothing, as -ffp-contract=off), then rounded to the storage dtype and widened."""
    dtype = z.dtype
    x = z[..., :C].float().numpy()
    Hi, Wi = x.shape[1:3]
    h0, h1, lh0, lh1 = _taps(Hi, H)
    w0, w1, lw0, lw1 = _taps(Wi, W)
    lh0, lh1 = lh0[None, :, None, None], lh1[None, :, None, None]
    lw0, lw1 = lw0[None, None, :, None], lw1[None, None, :, None]
    a, b = x[:, h0][:, :, w0], x[:, h0][:, :, w1]
    c, d = x[:, h1][:, :, w0], x[:, h1][:, :, w1]
    out = lh0 * (lw0 * a + lw1 * b) + lh1 * (lw0 * c + lw1 * d)
    assert out.dtype == np.float32
    return torch.from_numpy(out).to(dtype).float().numpy()


def fp64_z(z, C, H, W):
    """the same interpolation evaluated in float64 by torch -> float64 [B,H,W,C]"""
    x = z[..., :C].double().permute(0, 3, 1, 2)
    return F.interpolate(x, size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy()


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """-> (restated float32 z [B,H,W,C], fp64 arg-max [B,H,W], decidable mask [B,H,W]) of one case; computed once per process."""
    _, B, Hi, Wi, H, W, C, _ = next(c for c in CASES if c[0] == name)
    z = scores(name, dtype)
    z64 = fp64_z(z, C, H, W)
    if C > 1:
        top = np.partition(z64, C - 2, axis=-1)[..., C - 2:]
        decidable = (top[..., 1] - top[..., 0]) >= GAP[dtype](top[..., 1])
    else:
        decidable = np.ones(z64.shape[:3], dtype=bool)
    return restated_z(z, C, H, W), np.argmax(z64, axis=-1), decidable


def np_hist(pred, label, C):
    """hist[t, p] over the labels in 0..C-1, as metrics.fast_hist"""
    pred, label = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(label).reshape(-1)
    k = (label >= 0) & (label < C)
    return np.bincount(C * label[k] + pred[k], minlength=C * C).reshape(C, C)


def fp64_loss_sums(zf, label, C, ignore=IGNORE):
    """(sum nll, valid pixels) of the plain cross entropy in float64; zf: [B,H,W,C] scores (any float type), label int64 [B,H,W]"""
    z = torch.as_tensor(np.asarray(zf), dtype=torch.float64).reshape(-1, C)
    y = torch.as_tensor(np.asarray(label)).reshape(-1)
    valid = (y >= 0) & (y < C) & (y != ignore)
    if int(valid.sum()) == 0:
        return 0.0, 0
    return float(F.cross_entropy(z[valid], y[valid], reduction="sum")), int(valid.sum())


def np_colorize(pred, table, image=None, a=256):
    """uint8 palette look-up / integer blend in numpy"""
    col = np.asarray(table)[np.asarray(pred).astype(np.int64)].astype(np.int64)
    if image is None:
        return col.astype(np.uint8)
    return ((a * col + (256 - a) * np.asarray(image).astype(np.int64) + 128) >> 8).astype(np.uint8)
