"""numpy restatement of the reference's frequency filters (dataloaders.py:24-79 HPF / LPF / PHOT) on the ToTensor layout
[..., 3, H, W], float64.  Checked against the reference classes' own outputs (tests/golden/freq_filters.npz) in
tests/test_input_freq_cpu.py; the GPU operators (mrfp_amd/input_pipeline.py::hpf / lpf / phot) are checked against it.

* fftshift puts frequency 0 at index n//2, so shifted index i is frequency i - n//2 (the reference's centre int(n/2)).
* HPF zeroes fy^2 + fx^2 <= r^2, LPF keeps fy^2 + fx^2 < r^2 (strict only there).  The mask is constant along the channel
  axis, so both are a 2-D filter per channel: HPF = x - Re(IDFT2(F * band<=)), LPF = Re(IDFT2(F * band<)).
* PHOT = Re(ifftn(F / |F|)) * 5 * 255 over the 3-D spectrum (channel axis included); a zero bin gives NaN."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "freq_filters.npz")


def band(H: int, W: int, radius: float, strict: bool) -> np.ndarray:
    """The band in the unshifted (np.fft) layout."""
    fy = (np.arange(H) - H // 2)[:, None]
    fx = (np.arange(W) - W // 2)[None, :]
    d2 = fy * fy + fx * fx
    m = d2 < radius * radius if strict else d2 <= radius * radius
    return np.fft.ifftshift(m)


def low(x: np.ndarray, radius: float, strict: bool) -> np.ndarray:
    x = np.asarray(x, np.float64)
    F = np.fft.fft2(x, axes=(-2, -1))
    return np.fft.ifft2(F * band(x.shape[-2], x.shape[-1], radius, strict), axes=(-2, -1)).real


def hpf(x: np.ndarray, radius: float = 16.0) -> np.ndarray:
    return np.asarray(x, np.float64) - low(x, radius, False)


def lpf(x: np.ndarray, radius: float = 16.0) -> np.ndarray:
    return low(x, radius, True)


def phot(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, np.float64)
    axes = (-3, -2, -1)
    F = np.fft.fftn(x, axes=axes)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.fft.ifftn(F / np.abs(F), axes=axes).real * 5 * 255


def chw(img_hwc: np.ndarray) -> np.ndarray:
    """ToTensor's layout: uint8 [H,W,3] -> float32 [3,H,W] holding the same integers."""
    return np.ascontiguousarray(img_hwc.astype(np.float32).transpose(2, 0, 1))
