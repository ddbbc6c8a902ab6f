"""No-GPU checks of the frequency filters and of the Resize / Crop training compositions: the numpy restatement of HPF / LPF /
PHOT (tests/freq_common.py) against the reference classes' recorded outputs, the draw order of ResizeTransform / CropTransform,
and Pillow's BILINEAR tables against their scalar restatement."""
import random

import numpy as np
import pytest

import freq_common as fc
from oracle import input_oracle as io


@pytest.mark.parametrize("case", ["even", "odd", "tiny", "grey"])
def test_numpy_restatement_equals_reference_classes(case):
    G = np.load(fc.GOLDEN)
    x = fc.chw(G[case + "_img"])
    for name, fn in (("hpf", fc.hpf), ("lpf", fc.lpf), ("phot", fc.phot)):
        want = G["%s_%s" % (case, name)].transpose(2, 0, 1)
        got = fn(x)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (case, name)
        fin = ~np.isnan(want)
        np.testing.assert_allclose(got[fin], want[fin], rtol=0, atol=1e-4, err_msg="%s %s" % (case, name))
    if case == "grey":
        assert np.isnan(G["grey_phot"]).all()                # the reference's behaviour on R = G = B: all NaN
    if case == "tiny":
        assert np.abs(G["tiny_hpf"]).max() < 1e-3            # the band covers every frequency of a 24 x 20 image but four


def test_band_edges():
    """The four bins at distance exactly r: removed by HPF (<=) and not kept by LPF (<); signed range for even n."""
    m_le, m_lt = fc.band(64, 64, 16, False), fc.band(64, 64, 16, True)
    assert m_le[16, 0] and not m_lt[16, 0] and m_le[0, 48] and not m_lt[0, 48]
    assert m_le.sum() - m_lt.sum() == 4                   # (0, +-16), (+-16, 0): 256 is a sum of two squares only as 0 + 256
    m = fc.band(8, 8, 16, True)                           # clipped to [-4, 3]: 64 bins
    assert m.all()


def _jitter_draws(np_rng, j):
    ops = [("brightness", float(np_rng.uniform(max(0, 1 - j["brightness"]), 1 + j["brightness"]))),
           ("contrast", float(np_rng.uniform(max(0, 1 - j["contrast"]), 1 + j["contrast"]))),
           ("saturation", float(np_rng.uniform(max(0, 1 - j["saturation"]), 1 + j["saturation"]))),
           ("hue", float(np_rng.uniform(-j["hue"], j["hue"])))]
    np_rng.shuffle(ops)
    return ops


def test_resize_draw_order():
    """flip random(); jitter gate random() (+ numpy's four uniforms and shuffle); blur gate random() (+ radius)."""
    from mrfp_amd.input_pipeline import ResizeTransform
    t = ResizeTransform(768, 512)
    r, nr = random.Random(3), np.random.RandomState(3)
    r2, nr2 = random.Random(3), np.random.RandomState(3)
    seen = set()
    for _ in range(40):
        d = t.draw(1024, 2048, r, nr)
        flip = r2.random() < 0.5
        jitter = _jitter_draws(nr2, t.JITTER) if r2.random() < 0.5 else None
        blur = r2.random() if r2.random() < 0.5 else None
        assert (d.flip, d.jitter, d.blur, d.scaled, d.pad, d.crop) == (flip, jitter, blur, (768, 512), (0, 0), (0, 0))
        seen.add((flip, jitter is None, blur is None))
    assert len(seen) == 8
    assert r.random() == r2.random() and nr.uniform() == nr2.uniform()


def test_crop_draw_order():
    """As the Resize composition, with RandomCrop_p's randint(0, w - crop_size), randint(0, h - base_size) between the jitter
    and the blur -- both drawn unconditionally."""
    from mrfp_amd.input_pipeline import CropTransform
    t = CropTransform(96, 128)
    r, nr = random.Random(5), np.random.RandomState(5)
    r2, nr2 = random.Random(5), np.random.RandomState(5)
    for _ in range(40):
        d = t.draw(300, 200, r, nr)
        flip = r2.random() < 0.5
        jitter = _jitter_draws(nr2, t.JITTER) if r2.random() < 0.5 else None
        x0, y0 = r2.randint(0, 300 - 128), r2.randint(0, 200 - 96)
        blur = r2.random() if r2.random() < 0.5 else None
        assert (d.flip, d.jitter, d.crop, d.blur, d.scaled, d.pad) == (flip, jitter, (x0, y0), blur, (300, 200), (0, 0))
    assert r.random() == r2.random()
    d = CropTransform(96, 128).draw(128, 96, random.Random(0))    # exact fit: randint(0, 0) still consumes the stream
    assert d.crop == (0, 0)
    with pytest.raises(ValueError):                                # smaller than the crop: randint's empty range, as the reference
        CropTransform(96, 128).draw(127, 200, random.Random(0))


def test_bilinear_tables_match_pillow_restatement():
    from mrfp_amd import input_pipeline as ip
    for a, b in [(40, 56), (40, 24), (30, 44), (30, 18), (1024, 768), (2048, 768), (720, 1280), (7, 7), (5, 1), (1, 9)]:
        bp, kp = ip._bilinear_tables(a, b)
        bo, ko = io.resample_tables(a, b, "bilinear")
        assert np.array_equal(bp, bo) and np.array_equal(kp, ko), (a, b)
