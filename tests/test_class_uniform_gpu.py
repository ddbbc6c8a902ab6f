"""Class-uniform sampling on the device: mrfp_tile_class_sums against the numpy restatement, exactly (tests/class_uniform_common.py),
TrainTransform with draw(centroid=) against the bytes the reference's own classes produced, and the whole chain ClassCentroids ->
ClassUniformSampler -> harness.train_batches."""
import random

import numpy as np
import pytest
import torch

import class_uniform_common as cu
import poison_common as pc
from mrfp_amd import _lib, harness
from mrfp_amd import input_pipeline as ip

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _check(lab, C, tile, table=None, partial=False, ref=cu.tile_sums_np, dev_lab=None):
    """The operator on `lab` (numpy uint8 [B,H,W]; dev_lab: the device tensor to hand over instead of a plain copy) == ref, exactly."""
    want_sums, want_cent = ref(lab, C, tile, table, partial)
    x = torch.from_numpy(lab).to(DEV) if dev_lab is None else dev_lab
    t = torch.from_numpy(table).to(DEV) if table is not None else None
    sums, cent = ip.tile_class_centroids(x, C, tile, t, partial)
    assert sums.dtype == torch.int64 and cent.dtype == torch.int32
    assert tuple(sums.shape) == want_sums.shape and tuple(cent.shape) == want_cent.shape
    got_sums, got_cent = sums.cpu().numpy(), cent.cpu().numpy()
    bad = np.argwhere(got_sums != want_sums)
    assert len(bad) == 0, "sums differ at %d places, first [b, ty, tx, c, k] = %s: %d vs %d" % (
        len(bad), bad[0].tolist(), got_sums[tuple(bad[0])], want_sums[tuple(bad[0])])
    assert np.array_equal(got_cent, want_cent)
    return sums, cent


def test_whole_tiles_only_the_ragged_strips_are_never_looked_at():
    lab = cu.ragged_map()                                             # B=2, 13 x 21, tile 4: 3 x 5 whole tiles
    sums, cent = _check(lab, 5, 4)
    assert tuple(sums.shape) == (2, 3, 5, 5, 3)
    assert int(sums[..., 4, 0].sum()) == 0 and bool((cent[..., 4, :] == -1).all())        # class 4 lives in row 12 and column 20 only


def test_partial_tiles_count_the_ragged_ones():
    lab = cu.ragged_map()
    sums, _ = _check(lab, 5, 4, partial=True)                         # 4 x 6 tiles
    assert tuple(sums.shape) == (2, 4, 6, 5, 3) and int(sums[..., 4, 0].sum()) == 2 * (21 + 12)


def test_rows_no_vector_load_is_aligned_to_and_a_map_one_byte_into_its_buffer():
    lab = cu.ragged_map()
    buf = torch.zeros(lab.size + 17, dtype=torch.uint8, device=DEV)
    for off in (1, 16):                                               # W = 21: no row but the first starts on a 16-byte boundary
        view = buf[off:off + lab.size].view(lab.shape)
        view.copy_(torch.from_numpy(lab))
        assert view.data_ptr() % 16 == off % 16 and view.is_contiguous()
        _check(lab, 5, 4, partial=True, dev_lab=view)
    g = np.random.default_rng(3)
    wide = g.integers(0, 6, (2, 40, 64), dtype=np.uint8)             # pitch and tile multiples of 16, the base not
    buf = torch.zeros(wide.size + 16, dtype=torch.uint8, device=DEV)
    view = buf[1:1 + wide.size].view(wide.shape)
    view.copy_(torch.from_numpy(wide))
    _check(wide, 5, 16, partial=True, dev_lab=view)
    _check(wide, 5, 16, partial=True)                                 # ... and aligned: the 16-byte loads


@pytest.mark.parametrize("shape,tile", [((1, 40, 48), 32),           # 16-byte loads, ragged tiles 16 wide and 8 tall
                                         ((2, 210, 410), 200),        # bytewise, three chunks per tile, ragged tiles
                                         ((1, 70, 1040), 1024)])      # 16-byte loads, 16 rows per chunk, a 16-wide ragged tile
def test_ragged_tiles_and_several_chunks_per_tile(shape, tile):
    g = np.random.default_rng(shape[1])
    lab = np.repeat(np.repeat(g.integers(0, 7, (shape[0], (shape[1] + 6) // 7, (shape[2] + 8) // 9), dtype=np.uint8), 7, 1), 9, 2)
    lab = np.ascontiguousarray(lab[:, :shape[1], :shape[2]])
    lab[g.random(shape) < 0.02] = 255
    _check(lab, 6, tile, partial=True)
    if min(shape[1:]) >= tile:
        _check(lab, 6, tile)


def test_a_tile_larger_than_the_image():
    lab = cu.ragged_map()
    sums, _ = _check(lab, 5, 64, partial=True)
    assert tuple(sums.shape) == (2, 1, 1, 5, 3)
    with pytest.raises(_lib.MrfpHipError, match="no tile"):
        ip.tile_class_centroids(torch.from_numpy(lab).to(DEV), 5, 64)


def test_past_the_grid_cap_a_workgroup_walks_many_tiles():
    g = np.random.default_rng(4)
    lab = g.choice(np.array([0, 1, 2, 3, 9, 255], dtype=np.uint8), size=(3, 64, 4100))        # 32 x 2050 tiles per image
    sums, _ = _check(lab, 4, 2, ref=cu.tile_sums_big_np)
    assert sums.shape[1] * sums.shape[2] == 65600
    _check(lab[:, :63, :4099], 4, 2, partial=True, ref=cu.tile_sums_big_np)


def test_sums_beyond_32_bits():
    lab = np.zeros((1, 3, 65600), dtype=np.uint8)
    sums, cent = _check(lab, 1, 65536, partial=True)
    assert sums[0, 0, 0, 0].tolist() == [3 * 65536, 6442352640, 3 * 65536] and cent[0, 0, 0, 0].tolist() == [32767, 1]
    assert sums[0, 0, 1, 0].tolist() == [3 * 64, 3 * 2016, 64 * 3] and cent[0, 0, 1, 0].tolist() == [65536 + 31, 1]


def test_one_class_over_a_whole_tile_and_a_single_corner_pixel():
    lab = np.full((2, 256, 256), 255, dtype=np.uint8)
    lab[0] = 2
    lab[1, 255, 255] = 1
    lab[1, 0, 0] = 0
    sums, cent = _check(lab, 3, 256)
    assert sums[0, 0, 0, 2].tolist() == [65536, 256 * 32640, 256 * 32640] and cent[0, 0, 0, 2].tolist() == [127, 127]
    assert cent[1, 0, 0, 1].tolist() == [255, 255] and cent[1, 0, 0, 0].tolist() == [0, 0] and cent[1, 0, 0, 2].tolist() == [-1, -1]
    big = np.full((1, 96, 512), 7, dtype=np.uint8)                    # tile 512: 32 rows per chunk, every lane in one run
    _check(big, 8, 512, partial=True)


def test_a_fused_table_equals_the_table_applied_first():
    g = np.random.default_rng(8)
    lab = g.integers(0, 256, (2, 37, 53), dtype=np.uint8)
    table = g.integers(0, 24, 256).astype(np.uint8)
    table[g.random(256) < 0.2] = 255
    fused_sums, fused_cent = _check(lab, 19, 8, table=table, partial=True)
    enc = ip.LabelEncoder(table)
    x = torch.from_numpy(lab).to(DEV)
    first_sums, first_cent = ip.tile_class_centroids(enc(x), 19, 8, None, True)
    assert torch.equal(fused_sums, first_sums) and torch.equal(fused_cent, first_cent)
    enc_sums, _ = ip.tile_class_centroids(x, 19, 8, enc, True)       # a LabelEncoder is taken as its table
    assert torch.equal(fused_sums, enc_sums)


def _toy_samples(n=12, H=96, W=160):
    g = np.random.default_rng(21)
    samples, blocks = [], {2: (40, 100), 7: (70, 8)}                  # (y, x) of a 16 x 16 block of class 3, each inside one 32 x 32 tile
    for i in range(n):
        lab = np.zeros((H, W), dtype=np.uint8)
        lab[:, W // 2:] = 1
        if i in blocks:
            y, x = blocks[i]
            lab[y:y + 16, x:x + 16] = 3
        img = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
        samples.append((torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)))
    return samples


def test_two_runs_are_bit_identical_and_nothing_depends_on_fresh_memory():
    g = np.random.default_rng(6)
    lab = torch.from_numpy(g.integers(0, 21, (2, 75, 130), dtype=np.uint8)).to(DEV)
    a = ip.tile_class_centroids(lab, 19, 32, None, True)
    b = ip.tile_class_centroids(lab, 19, 32, None, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    sites = pc.run_three(lambda: pc.named(*zip(("sums", "cent"), ip.tile_class_centroids(lab, 19, 32, None, True))))
    assert "input_pipeline._out_slot" in sites
    samples = _toy_samples(4)
    items = [(0, None, None), (2, (107, 47), 3), (1, None, None), (2, (107, 47), 3)]
    tt = ip.TrainTransform(48)

    def batch():
        img, lab = next(harness.train_batches(samples, tt, 4, items, None, random.Random(5), np.random.RandomState(5)))
        return pc.named(img=img, label=lab)
    pc.run_three(batch)


def test_train_transform_reproduces_the_references_crops():
    z = cu.load_golden()
    src = {si: (torch.from_numpy(z["src_img_%d" % si]).to(DEV), torch.from_numpy(z["src_lab_%d" % si]).to(DEV))
           for si in range(len(cu.GOLDEN_SIZES))}
    for i, (si, smin, smax, cen) in enumerate(cu.golden_templates()):
        w, h = cu.GOLDEN_SIZES[si]
        seed = int(z["seeds"][i])
        tt = ip.TrainTransform(cu.GOLDEN_CROP, smin, smax)
        d = tt.draw(w, h, random.Random(seed), np.random.RandomState(seed), centroid=cen)
        img, lab = tt(*src[si], d)
        got_lab = lab.cpu().numpy()
        got_img = img.permute(1, 2, 0).cpu().numpy()
        assert np.array_equal(got_lab, z["out_lab"][i].astype(np.int64)), "label of record %d (seed %d)" % (i, seed)
        assert np.array_equal(got_img, z["out_img"][i].astype(np.float32)), "image of record %d (seed %d)" % (i, seed)


def test_end_to_end_every_item_drawn_for_a_class_shows_it():
    samples = _toy_samples()
    cc = ip.ClassCentroids(5, tile=32)
    cc.add(0, torch.stack([s[1] for s in samples[:6]]))
    for i in range(6, 12):
        cc.add(i, samples[i][1])
    assert cc.by_class[3] == [(2, (107, 47)), (7, (15, 77))] and not cc.by_class[2] and not cc.by_class[4]
    assert len(cc.by_class[0]) == 12 * 3 * 3 and cc.by_class[0][0] == (0, (15, 15))            # class 0: the left half, 3 x 3 tiles per image
    sampler = ip.ClassUniformSampler(12, cc, pct=1.0)
    T = 48
    tt = ip.TrainTransform(T)
    shown = plain = 0
    for seed in range(20):
        items = sampler.epoch(np.random.RandomState(seed))
        assert len(items) == 2 + 2 * 3                                 # per_class = 2, classes 0, 1, 3 present, two plain items
        rng, np_rng = random.Random(seed), np.random.RandomState(100 + seed)
        rng2, np_rng2 = random.Random(seed), np.random.RandomState(100 + seed)
        got = list(harness.train_batches(samples, tt, 4, items, None, rng, np_rng))
        assert len(got) == 2 and tuple(got[0][0].shape) == (4, 3, T, T) and tuple(got[0][1].shape) == (4, T, T)
        for j, (index, cen, cls) in enumerate(items[:8]):
            img, lab = got[j // 4][0][j % 4], got[j // 4][1][j % 4]
            if cen is None:
                want = cu.parent_draw(T, 0.5, 2.0, 160, 96, rng2, np_rng2)
                wimg, wlab = tt(*samples[index], ip.Draw(*want))
                assert torch.equal(img, wimg) and torch.equal(lab, wlab)
                plain += 1
            else:
                want = cu.centroid_draw(T, 0.5, 2.0, 160, 96, rng2, np_rng2, cen)
                assert want[3] == (0, 0)                               # 96 x 160 at scale >= 0.5 never needs padding for a 48 crop
                if cls == 3:
                    assert bool((lab == 3).any()), "seed %d item %d: the crop at %s misses class 3 (flip %s, scaled %s, centroid %s)" % (
                        seed, j, want[4], want[0], want[2], want[6])
                    shown += 1
    assert shown >= 30 and plain >= 20
    short = list(harness.train_batches(samples, tt, 8, None, None, random.Random(1), np.random.RandomState(1), drop_last=False))
    assert [tuple(b[1].shape) for b in short] == [(8, T, T), (4, T, T)]
    assert len(list(harness.train_batches(samples, tt, 8, None, None, random.Random(1), np.random.RandomState(1)))) == 1
