"""HPF / LPF / PHOT on the GPU (csrc/freq.hip, mrfp_amd/input_pipeline.py::hpf / lpf / phot) against the reference classes'
recorded outputs (tests/golden/freq_filters.npz) and the float64 numpy restatement (tests/freq_common.py)."""
import numpy as np
import pytest
import torch

import freq_common as fc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ip():
    from mrfp_amd import input_pipeline as ip
    return ip


def _rand_chw(H, W, seed, B=None):
    rng = np.random.default_rng(seed)
    shape = (3, H, W) if B is None else (B, 3, H, W)
    return rng.integers(0, 256, shape).astype(np.float32)


def _check_band(got, want, what):
    err = float(np.abs(got.astype(np.float64) - want).max())
    assert err <= 5e-3, (what, err)


def _check_phot(got, want, what):
    scale = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    assert err <= 1e-4 * scale, (what, err, scale)


@pytest.mark.parametrize("case", ["even", "odd", "tiny", "grey"])
def test_filters_match_reference_classes(case):
    ip = _ip()
    G = np.load(fc.GOLDEN)
    x = torch.from_numpy(fc.chw(G[case + "_img"])).to(DEV)
    for name, fn in (("hpf", ip.hpf), ("lpf", ip.lpf), ("phot", ip.phot)):
        want = G["%s_%s" % (case, name)].transpose(2, 0, 1).astype(np.float64)
        got = fn(x).cpu().numpy()
        assert got.shape == want.shape and got.dtype == np.float32
        if case == "grey" and name == "phot":
            assert np.isnan(want).all() and np.isnan(got).all()
            continue
        (_check_phot if name == "phot" else _check_band)(got, want, (case, name))


@pytest.mark.parametrize("H,W", [(768, 768), (64, 96), (45, 75), (24, 20)])
def test_filters_match_restatement(H, W):
    ip = _ip()
    x = _rand_chw(H, W, H * 1000 + W)
    xd = torch.from_numpy(x).to(DEV)
    _check_band(ip.hpf(xd).cpu().numpy(), fc.hpf(x), ("hpf", H, W))
    _check_band(ip.lpf(xd).cpu().numpy(), fc.lpf(x), ("lpf", H, W))
    _check_phot(ip.phot(xd).cpu().numpy(), fc.phot(x), ("phot", H, W))


def test_other_radii():
    ip = _ip()
    x = _rand_chw(96, 80, 11)
    xd = torch.from_numpy(x).to(DEV)
    for r in (0.0, 3.5, 16.0, 20.0, 32.5):
        _check_band(ip.hpf(xd, radius=r).cpu().numpy(), fc.hpf(x, r), ("hpf", r))
        _check_band(ip.lpf(xd, radius=r).cpu().numpy(), fc.lpf(x, r), ("lpf", r))


def test_batched_equals_per_image():
    ip = _ip()
    for H, W in [(64, 96), (45, 75)]:
        x = torch.from_numpy(_rand_chw(H, W, 7, B=4)).to(DEV)
        for fn in (ip.hpf, ip.lpf, ip.phot):
            yb = fn(x)
            assert yb.shape == x.shape
            for b in range(4):
                assert torch.equal(yb[b], fn(x[b])), (fn.__name__, H, W, b)


def test_any_size_band_and_phot_length_error():
    """77 x 64: the band filters take any size; PHOT refuses a line length with a prime factor other than 2, 3, 5."""
    from mrfp_amd import _lib
    ip = _ip()
    x = _rand_chw(77, 64, 5)
    xd = torch.from_numpy(x).to(DEV)
    _check_band(ip.hpf(xd).cpu().numpy(), fc.hpf(x), "hpf 77x64")
    _check_band(ip.lpf(xd).cpu().numpy(), fc.lpf(x), "lpf 77x64")
    with pytest.raises(_lib.MrfpHipError, match="77"):
        ip.phot(xd)
    with pytest.raises(_lib.MrfpHipError, match="4608"):
        ip.phot(torch.zeros(3, 8, 4608, device=DEV))


def test_bitwise_reproducible_and_out_slots():
    ip = _ip()
    xd = torch.from_numpy(_rand_chw(768, 768, 1, B=2)).to(DEV)
    for fn in (ip.hpf, ip.lpf, ip.phot):
        a, b = fn(xd), fn(xd)
        assert torch.equal(a, b), fn.__name__
        out = torch.empty_like(xd)
        assert fn(xd, out=out) is out and torch.equal(out, a)
    y = xd.clone()
    ip.hpf(y, out=y)                                                   # in place
    assert torch.equal(y, ip.hpf(xd))


def test_refuses_bad_inputs():
    from mrfp_amd import _lib
    ip = _ip()
    for bad in (torch.zeros(3, 8, 8), torch.zeros(3, 8, 8, device=DEV, dtype=torch.float64), torch.zeros(4, 8, 8, device=DEV),
                torch.zeros(8, 8, device=DEV), torch.zeros(1, 2, 3, 8, 8, device=DEV)):
        for fn in (ip.hpf, ip.lpf, ip.phot):
            with pytest.raises(_lib.MrfpHipError):
                fn(bad)
    with pytest.raises(_lib.MrfpHipError):
        ip.hpf(torch.zeros(3, 8, 8, device=DEV), out=torch.zeros(3, 8, 9, device=DEV))
    with pytest.raises(_lib.MrfpHipError):
        ip.hpf(torch.zeros(3, 8, 8, device=DEV), radius=40.0)
