"""Class-uniform sampling without a GPU: the tile rule against scipy, the sampler, TrainTransform.draw(centroid=) against its
restatement and against records of the reference's own classes, and the host-side refusals of the two new entry points."""
import ctypes
import json
import random

import numpy as np
import pytest
import torch

import class_uniform_common as cu
from mrfp_amd import _lib, build
from mrfp_amd import input_pipeline as ip


@pytest.fixture(scope="module")
def cdll():
    build.build()
    return _lib.lib()


# ---- the rule: n, sum x, sum y and integer division == int(center_of_mass) + offset ------------------------------------------------
def test_the_integer_rule_equals_scipy_center_of_mass_on_random_patches():
    g = np.random.default_rng(5)
    mismatches = checked = 0
    for k in range(300):
        h, w = int(g.integers(1, 40)), int(g.integers(1, 40))
        C = int(g.integers(1, 6))
        # blocky maps (as label maps are) for half of the patches, noise for the rest
        if k % 2:
            patch = g.integers(0, C + 1, (h, w), dtype=np.uint8)
        else:
            patch = np.repeat(np.repeat(g.integers(0, C + 1, ((h + 4) // 5, (w + 4) // 5), dtype=np.uint8), 5, 0), 5, 1)[:h, :w]
        _, cent = cu.tile_sums_np(patch, C, max(h, w), partial=True)
        for c in range(C):
            if (patch == c).any():
                checked += 1
                mismatches += tuple(cent[0, 0, 0, c]) != cu.scipy_centroid(patch, c)
            else:
                assert tuple(cent[0, 0, 0, c]) == (-1, -1)
    assert checked > 600 and mismatches == 0, (checked, mismatches)


def test_single_pixel_classes_tile_offsets_and_the_long_strip():
    lab = np.full((12, 12), 255, dtype=np.uint8)
    lab[0, 0], lab[3, 7], lab[11, 11], lab[8, 4] = 0, 1, 2, 3
    sums, cent = cu.tile_sums_np(lab, 4, 4)
    for c, (y, x) in enumerate(((0, 0), (3, 7), (11, 11), (8, 4))):
        ty, tx = y // 4, x // 4
        assert tuple(cent[0, ty, tx, c]) == (x, y) == cu.scipy_centroid(lab[ty * 4:ty * 4 + 4, tx * 4:tx * 4 + 4], c, tx * 4, ty * 4)
        assert sums[0, ty, tx, c].tolist() == [1, x % 4, y % 4] and int(sums[..., c, 0].sum()) == 1
    strip = np.zeros((3, 65536), dtype=np.uint8)                     # sum x = 3 * 65535 * 65536 / 2 > 2^32
    sums, cent = cu.tile_sums_np(strip, 1, 65536, partial=True)
    assert sums[0, 0, 0, 0].tolist() == [3 * 65536, 6442352640, 65536 * 3] and sums[0, 0, 0, 0, 1] > 2 ** 32
    assert tuple(cent[0, 0, 0, 0]) == (32767, 1) == cu.scipy_centroid(strip, 0)


def test_whole_tiles_only_unless_partial_and_the_table_comes_first():
    lab = cu.ragged_map()
    sums, cent = cu.tile_sums_np(lab, 5, 4)
    assert sums.shape == (2, 3, 5, 5, 3) and int(sums[..., 4, 0].sum()) == 0 and (cent[..., 4, :] == -1).all()
    psums, pcent = cu.tile_sums_np(lab, 5, 4, partial=True)
    assert psums.shape == (2, 4, 6, 5, 3) and int(psums[..., 4, 0].sum()) == 2 * (21 + 12)
    assert np.array_equal(psums[:, :3, :5], sums)                     # the whole tiles are the same tiles
    assert int(psums[..., 0].sum()) == int((lab < 5).sum())           # 7 and 255 belong to nothing
    table = np.arange(256, dtype=np.uint8)
    table[7], table[0] = 0, 255
    tsums, _ = cu.tile_sums_np(lab, 5, 4, table=table, partial=True)
    assert int(tsums[..., 0, 0].sum()) == int((lab == 7).sum())
    assert cu.tile_count(13, 4, False) == 3 and cu.tile_count(13, 4, True) == 4 and cu.tile_count(3, 4, False) == 0


def test_the_vectorised_restatement_equals_the_loop():
    g = np.random.default_rng(9)
    lab = g.choice(np.array([0, 1, 2, 9, 255], dtype=np.uint8), size=(2, 11, 19))
    table = g.integers(0, 256, 256).astype(np.uint8)
    for partial in (False, True):
        for tab in (None, table):
            a, b = cu.tile_sums_np(lab, 3, 2, tab, partial), cu.tile_sums_big_np(lab, 3, 2, tab, partial)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the sampler -----------------------------------------------------------------------------------------------------------------
def _by_class():
    return [[(0, (5, 5)), (3, (9, 1))], [], [(2, (0, 0))], [(i, (i, 2 * i)) for i in range(7)], []]


def test_epoch_length_class_counts_and_wrap_around():
    by_class = _by_class()
    n = 23
    s = ip.ClassUniformSampler(n, by_class, pct=0.7)
    items = s.epoch(np.random.RandomState(1))
    per_class = int(n * 0.7 / 5)
    n_rand = n - per_class * 5
    assert per_class == 3 and len(items) == n_rand + per_class * 3          # classes 1 and 4 are nowhere: the epoch is shorter
    for c in (0, 2, 3):
        got = [it for it in items if it[2] == c]
        assert len(got) == per_class and all((i, cen) in by_class[c] for i, cen, _ in got)
    assert not [it for it in items if it[2] in (1, 4)]
    plain = [it for it in items if it[2] is None]
    assert len(plain) == n_rand and all(cen is None and 0 <= i < n for i, cen, _ in plain) and len({i for i, _, _ in plain}) == n_rand
    picked = ip.ClassUniformSampler.pick(by_class[2], 4, np.random.RandomState(0))          # a one-entry list wraps around
    assert picked == [by_class[2][0]] * 4
    picked = ip.ClassUniformSampler.pick(by_class[0], 5, np.random.RandomState(0))
    assert picked[0] == picked[2] == picked[4] and picked[1] == picked[3] and set(picked) == set(by_class[0])


def test_epoch_equals_the_restatement_and_repeats_with_the_seed():
    by_class = _by_class()
    for pct in (0.0, 0.25, 0.7, 1.0):
        for shuffle in (True, False):
            a = ip.ClassUniformSampler(40, by_class, pct).epoch(np.random.RandomState(7), shuffle)
            b, _, _ = cu.epoch_np(40, by_class, pct, np.random.RandomState(7), shuffle)
            assert a == b
            assert a == ip.ClassUniformSampler(40, by_class, pct).epoch(np.random.RandomState(7), shuffle)
    assert (ip.ClassUniformSampler(40, by_class, 0.7).epoch(np.random.RandomState(7))
            != ip.ClassUniformSampler(40, by_class, 0.7).epoch(np.random.RandomState(8)))


def test_pct_zero_is_a_permutation_and_pct_none_reads_the_config():
    from mrfp_amd.config import cfg
    assert cfg.CLASS_UNIFORM_PCT == 0.0 and cfg.CLASS_UNIFORM_TILE == 1024
    items = ip.ClassUniformSampler(17, _by_class()).epoch(np.random.RandomState(3))
    assert sorted(i for i, _, _ in items) == list(range(17)) and all(cen is None and c is None for _, cen, c in items)
    assert [i for i, _, _ in items] != list(range(17))
    with pytest.raises(ValueError, match="pct"):
        ip.ClassUniformSampler(17, _by_class(), pct=1.5)


def test_shards_are_disjoint_and_equally_long():
    items = ip.ClassUniformSampler(50, _by_class(), 0.5).epoch(np.random.RandomState(2))
    tagged = list(enumerate(items))
    shards = [ip.ClassUniformSampler.shard(tagged, r, 4) for r in range(4)]
    assert all(len(s) == len(items) // 4 for s in shards)
    seen = [k for s in shards for k, _ in s]
    assert len(set(seen)) == len(seen)
    assert shards[1][0] == tagged[1] and shards[1][1] == tagged[5]


def test_class_centroids_state_is_json_and_loads_back():
    cc = ip.ClassCentroids(5)
    cc.by_class = _by_class()
    sd = json.loads(json.dumps(cc.state_dict()))
    other = ip.ClassCentroids(5, tile=64)
    other.load_state_dict(sd)
    assert other.by_class == cc.by_class and other.tile is None and other.partial_tiles is False
    with pytest.raises(ValueError):
        ip.ClassCentroids(4).load_state_dict(sd)
    assert ip.ClassUniformSampler(9, other, 1.0).by_class is other.by_class


# ---- the draw --------------------------------------------------------------------------------------------------------------------
def test_draw_with_a_centroid_covers_it_stays_inside_and_follows_the_restatement():
    T = 32
    tt = ip.TrainTransform(T)
    g = random.Random(12)
    nopad = both = early = 0
    for k in range(2000):
        w, h = g.randint(20, 90), g.randint(20, 90)
        cen = (g.randint(0, w - 1), g.randint(0, h - 1))
        seed = 1000 + k
        rng, np_rng = random.Random(seed), np.random.RandomState(seed)
        d = tt.draw(w, h, rng, np_rng, centroid=cen)
        rng2, np_rng2 = random.Random(seed), np.random.RandomState(seed)
        want = cu.centroid_draw(T, 0.5, 2.0, w, h, rng2, np_rng2, cen)
        assert cu.draw_tuple(d) == want[:6] and d.centroid == want[6]
        assert rng.getstate() == rng2.getstate()                             # the `random` stream stands where the restatement's does
        assert np_rng.get_state()[2] == np_rng2.get_state()[2] and np.array_equal(np_rng.get_state()[1], np_rng2.get_state()[1])
        (sw, sh), (pw, ph), (x1, y1), (cx, cy) = d.scaled, d.pad, d.crop, d.centroid
        assert 0 <= x1 <= sw + 2 * pw - T and 0 <= y1 <= sh + 2 * ph - T      # the crop stays inside the padded image
        if (sw, sh) == (T, T):
            early += 1
            continue
        if pw == 0:
            assert x1 <= cx <= x1 + T
        if ph == 0:
            assert y1 <= cy <= y1 + T
        nopad += pw == 0 and ph == 0
        both += pw > 0 and ph > 0
    assert nopad > 500 and both > 20


def test_centroid_none_gives_exactly_the_parents_draws():
    T = 32
    tt = ip.TrainTransform(T)
    g = random.Random(13)
    for k in range(2000):
        w, h = g.randint(20, 90), g.randint(20, 90)
        seed = 5000 + k
        rng, np_rng = random.Random(seed), np.random.RandomState(seed)
        d = tt.draw(w, h, rng, np_rng)
        rng2, np_rng2 = random.Random(seed), np.random.RandomState(seed)
        assert cu.draw_tuple(d) == cu.parent_draw(T, 0.5, 2.0, w, h, rng2, np_rng2) and d.centroid is None
        assert rng.getstate() == rng2.getstate() and np.array_equal(np_rng.get_state()[1], np_rng2.get_state()[1])
    assert ip.Draw(False, None, (1, 1), (0, 0), (0, 0), None).centroid is None        # positional construction keeps working


def test_the_early_return_draws_nothing_and_the_plain_path_may_draw_fewer():
    tt = ip.TrainTransform(16, 1.0, 1.0)

    class Counting(random.Random):
        calls = 0

        def randint(self, a, b):
            Counting.calls += 1
            return super().randint(a, b)
    d = tt.draw(16, 16, Counting(1), np.random.RandomState(1), centroid=(3, 4))
    assert Counting.calls == 0 and d.crop == (0, 0) and d.pad == (0, 0)
    tt.draw(16, 40, Counting(1), np.random.RandomState(1))                   # W2 == T: the plain path draws y1 only
    assert Counting.calls == 1
    tt.draw(16, 40, Counting(1), np.random.RandomState(1), centroid=(3, 4))  # two, always
    assert Counting.calls == 3


def test_draw_reproduces_every_record_of_the_reference():
    z = cu.load_golden()
    rec, keys = z["records"], z["record_keys"].tolist()
    assert keys == ["flip", "sw", "sh", "pad_w", "pad_h", "x1", "y1", "nrandint"] and len(rec) == len(cu.golden_templates()) == 40
    templates = cu.golden_templates()
    for i, (si, smin, smax, cen) in enumerate(templates):
        assert z["params"][i].tolist() == [si, cen[0], cen[1]] and z["scales"][i].tolist() == [smin, smax]
        w, h = cu.GOLDEN_SIZES[si]
        seed = int(z["seeds"][i])
        rng, np_rng = random.Random(seed), np.random.RandomState(seed)
        d = ip.TrainTransform(cu.GOLDEN_CROP, smin, smax).draw(w, h, rng, np_rng, centroid=cen)
        flip, sw, sh, pw, ph, x1, y1, nr = rec[i].tolist()
        assert (int(d.flip), d.scaled, d.pad, d.crop) == (flip, (sw, sh), (pw, ph), (x1, y1)), i
        assert rng.random() == float(z["probes"][i]), i                       # the stream position behind the whole pipeline
    early = rec[:, 7] == 0
    px, py = rec[:, 3] > 0, rec[:, 4] > 0
    assert early.any() and (px & py).any() and (px ^ py).any() and set(rec[:, 0].tolist()) == {0, 1}
    cens = {(int(p[0]), int(p[1]), int(p[2])) for p in z["params"]}
    assert any(c[1] == 0 for c in cens) and any(c[1] == cu.GOLDEN_SIZES[c[0]][0] - 1 for c in cens)
    import os
    assert os.path.getsize(cu.GOLDEN) < 100 * 1024


# ---- the boundary ----------------------------------------------------------------------------------------------------------------
def test_every_argument_has_a_name_and_the_host_refuses_by_name(cdll):
    protos = _lib.parse_header()
    assert _lib.ARG_NAMES["mrfp_tile_count"] == ["size", "tile", "partial"]
    assert _lib.ARG_NAMES["mrfp_tile_class_sums"] == ["lab", "table", "B", "H", "W", "C", "tile", "partial", "sums", "cent", "stream"]
    assert protos["mrfp_tile_count"][0] is ctypes.c_int64 and len(protos["mrfp_tile_class_sums"][1]) == 11
    assert cdll.mrfp_tile_count(1052, 1024, 0) == 1 and cdll.mrfp_tile_count(1914, 1024, 0) == 1 and cdll.mrfp_tile_count(1914, 1024, 1) == 2
    assert cdll.mrfp_tile_count(1000, 1024, 0) == 0 and cdll.mrfp_tile_count(8, 0, 0) == -1
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255                          # nothing is launched: a host address will do
    good = dict(lab=p, table=None, B=2, H=13, W=21, C=5, tile=4, partial=0, sums=p, cent=p, stream=None)

    def refused(**kw):
        args = dict(good, **kw)
        rc = cdll.mrfp_tile_class_sums(*[args[n] for n in _lib.ARG_NAMES["mrfp_tile_class_sums"]])
        assert rc == -1
        return cdll.mrfp_last_error().decode()
    assert "C = 0 is outside 1..256" in refused(C=0)
    assert "C = 257 is outside 1..256" in refused(C=257)
    assert "tile = 0 is outside 1..65536" in refused(tile=0)
    assert "tile = 65537 is outside 1..65536" in refused(tile=65537)
    assert "no tile" in refused(tile=16) and "no tile" in refused(H=3)
    assert "H, W < 2^31" in refused(W=1 << 31, partial=1)
    assert "reaches 2^31" in refused(B=1 << 20, H=1 << 12, W=1 << 12, tile=1, C=2)
    assert "null argument" in refused(lab=None) and "null argument" in refused(cent=None)


def test_python_refuses_what_is_not_a_uint8_device_map():
    with pytest.raises(_lib.MrfpHipError, match="uint8 CUDA tensor"):
        ip.tile_class_centroids(torch.zeros(8, 8, dtype=torch.uint8), 5, 4)          # a CPU tensor: there is no CPU path
    with pytest.raises(_lib.MrfpHipError, match="uint8 CUDA tensor"):
        ip.tile_class_centroids(torch.zeros(8, 8, dtype=torch.int64), 5, 4)
    with pytest.raises(_lib.MrfpHipError, match="uint8 CUDA tensor"):
        ip.tile_class_centroids(np.zeros((8, 8), dtype=np.uint8), 5, 4)
    with pytest.raises(ValueError, match="num_classes"):
        ip.ClassCentroids(0)
