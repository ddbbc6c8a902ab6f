"""Evaluation input path on the GPU (csrc/input.hip: label_lut_u8, label_encode_i64, eval_assemble; input_pipeline.LabelEncoder,
EvalTransform, ResizeHeightCenterCropPad; harness.eval_batches).  Every comparison is byte for byte: the look-ups against
table[map] in numpy, EvalTransform against the numpy ToTensor, ResizeHeightCenterCropPad against what PIL recorded in
tests/golden/eval_input.npz (no Pillow and no reference tree at test time)."""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

import eval_input_common as eic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mapillary_table():
    return eic.fixture()["tables"][eic.DATASETS.index("MapillarySegmentation")]


def _flat_map(n: int, seed: int) -> np.ndarray:
    """n bytes that hold all 256 values once n allows it"""
    side = max(16, int(np.ceil(np.sqrt(max(n, 1)))))
    return np.ascontiguousarray(eic.all_values_map(side, side, seed).reshape(-1)[:n])


def _chunk_walk_bytes() -> int:
    """bytes after which the capped grid makes every workgroup walk a second chunk: the cap of the row kernels
    (csrc/common.hpp: lines_per_image) times the bytes of one chunk (csrc/input.hip: 16 per lane)"""
    common = open(os.path.join(ROOT, "mrfp_amd", "csrc", "common.hpp")).read()
    cap = int(re.search(r'env_switch\("MRFP_ROW_BLOCKS", (\d+)\)', common).group(1))
    threads = int(re.search(r"constexpr int kThreads = (\d+);", common).group(1))
    src = open(os.path.join(ROOT, "mrfp_amd", "csrc", "input.hip")).read()
    vec = int(re.search(r"constexpr int kLutVec = (\d+);", src).group(1))
    assert "lines_per_image(1, nchunks)" in src
    return cap * threads * vec


SIZES = [1, 15, 16, 17, 4099]
OFFSETS = [(0, 0), (1, 1), (3, 3), (1, 3), (3, 1)]          # (source, destination) byte offsets in a larger buffer


@pytest.mark.parametrize("n", SIZES)
def test_label_lut_u8_sizes_offsets_in_place(n):
    from mrfp_amd import input_pipeline as ip
    table = _mapillary_table()
    enc = ip.LabelEncoder(table)
    src = _flat_map(n, n)
    for so, do in OFFSETS:
        sbuf = torch.zeros(n + 64, dtype=torch.uint8, device=DEV)
        sbuf[so:so + n] = torch.from_numpy(src).to(DEV)
        dbuf = torch.full((n + 64,), 77, dtype=torch.uint8, device=DEV)
        got = enc(sbuf[so:so + n], out=dbuf[do:do + n])
        assert got.data_ptr() == dbuf.data_ptr() + do
        d = dbuf.cpu().numpy()
        assert np.array_equal(d[do:do + n], table[src]), (n, so, do)
        assert (d[:do] == 77).all() and (d[do + n:] == 77).all(), (n, so, do)          # not a byte beside the slice
        inplace = sbuf[so:so + n]
        assert enc(inplace, out=inplace) is inplace
        assert np.array_equal(inplace.cpu().numpy(), table[src]), (n, so, "in place")
    fresh = enc(torch.from_numpy(src).to(DEV))
    assert fresh.dtype == torch.uint8 and np.array_equal(fresh.cpu().numpy(), table[src])


@pytest.mark.parametrize("n", SIZES)
def test_label_encode_i64_sizes_offsets_null_table(n):
    from mrfp_amd import input_pipeline as ip
    table = _mapillary_table()
    enc = ip.LabelEncoder(table)
    src = _flat_map(n, n + 1)
    for so, do in OFFSETS:                                   # the destination offset counts int64 elements here
        sbuf = torch.zeros(n + 64, dtype=torch.uint8, device=DEV)
        sbuf[so:so + n] = torch.from_numpy(src).to(DEV)
        dbuf = torch.full((n + 8,), -5, dtype=torch.int64, device=DEV)
        got = enc.to_int64(sbuf[so:so + n], out=dbuf[do:do + n])
        assert got.data_ptr() == dbuf.data_ptr() + 8 * do
        d = dbuf.cpu().numpy()
        assert np.array_equal(d[do:do + n], table[src].astype(np.int64)), (n, so, do)
        assert (d[:do] == -5).all() and (d[do + n:] == -5).all(), (n, so, do)
        ident = ip._to_int64(sbuf[so:so + n], None, None, "out")                        # the null table: identity
        assert ident.dtype == torch.int64 and np.array_equal(ident.cpu().numpy(), src.astype(np.int64)), (n, so)


def test_label_kernels_all_values_and_empty():
    from mrfp_amd import _lib
    from mrfp_amd import input_pipeline as ip
    m = eic.all_values_map(32, 48, seed=5)
    assert len(np.unique(m)) == 256
    x = torch.from_numpy(m).to(DEV)
    for name in eic.DATASETS:
        enc = ip.label_encoder(name)
        want = eic.fixture()["tables"][eic.DATASETS.index(name)][m]
        assert np.array_equal(enc(x).cpu().numpy(), want), name
        assert np.array_equal(enc.to_int64(x).cpu().numpy(), want.astype(np.int64)), name
    # n == 0: valid, nothing written (through the C entries with live pointers, and through the wrappers)
    enc = ip.label_encoder("MapillarySegmentation")
    guard8 = torch.full((32,), 9, dtype=torch.uint8, device=DEV)
    guard64 = torch.full((4,), 9, dtype=torch.int64, device=DEV)
    _lib.call("mrfp_label_lut_u8", x.data_ptr(), guard8.data_ptr(), 0, enc.device_table(x.device).data_ptr(), _lib.stream())
    _lib.call("mrfp_label_encode_i64", x.data_ptr(), None, guard64.data_ptr(), 0, _lib.stream())
    assert (guard8 == 9).all() and (guard64 == 9).all()
    e = torch.empty((0, 7), dtype=torch.uint8, device=DEV)
    assert tuple(enc(e).shape) == (0, 7) and enc.to_int64(e).dtype == torch.int64


def test_label_kernels_walk_several_chunks():
    """The capped grid: every workgroup walks three chunks, the last one partial (+ 7 odd bytes), from an odd source offset."""
    from mrfp_amd import input_pipeline as ip
    sweep = _chunk_walk_bytes()
    n = 2 * sweep + sweep // 2 + 7
    table = _mapillary_table()
    enc = ip.LabelEncoder(table)
    base = _flat_map(1 << 16, 9)
    src = np.resize(base, n + 3)
    buf = torch.from_numpy(src).to(DEV)
    tdev = torch.from_numpy(table.copy()).to(DEV)
    for off in (0, 3):
        x = buf[off:off + n]
        want = tdev[x.long()]                                # the reference on the device: 25 MB maps are not copied back
        assert np.array_equal(want[:70000].cpu().numpy(), table[src[off:off + 70000]])
        got = enc(x)
        assert torch.equal(got, want), off
        got64 = enc.to_int64(x)
        assert torch.equal(got64, want.long()), off
        del got, got64, want
    x = buf[3:3 + n]
    want = tdev[x.long()]
    enc(x, out=x)
    assert torch.equal(x, want)


@pytest.mark.parametrize("H,W", [(5, 7), (33, 65)])
def test_eval_transform(H, W):
    from mrfp_amd import input_pipeline as ip
    img, lab = eic.sample(W, H, seed=H, ids=36)
    xi, xl = torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)
    tf = ip.EvalTransform()
    for name in (None, "CityscapesSegmentation", "GTAVSegmentation"):
        enc = ip.label_encoder(name) if name else None
        want_img, want_lab = eic.eval_transform(img, lab, enc.table if enc else None)
        got_img, got_lab = tf(xi, xl, enc)
        assert got_img.dtype == torch.float32 and got_lab.dtype == torch.int64
        assert np.array_equal(got_img.cpu().numpy(), want_img) and np.array_equal(got_lab.cpu().numpy(), want_lab), name
        bi = torch.full((2, 3, H, W), -1.0, device=DEV)
        bl = torch.full((2, H, W), -1, dtype=torch.int64, device=DEV)
        oi, ol = tf(xi, xl, enc, out_img=bi[1], out_lab=bl[1])                        # into one sample of a batch
        assert oi.data_ptr() == bi[1].data_ptr() and ol.data_ptr() == bl[1].data_ptr()
        assert np.array_equal(bi[1].cpu().numpy(), want_img) and np.array_equal(bl[1].cpu().numpy(), want_lab), name
        assert (bi[0] == -1).all() and (bl[0] == -1).all()


@pytest.mark.parametrize("case", range(len(eic.CASES)), ids=[c[0] for c in eic.CASES])
def test_resize_height_center_crop_pad_equals_pil(case):
    from mrfp_amd import input_pipeline as ip
    f = eic.fixture()
    name = eic.CASES[case][0]
    img, lab = eic.case_sample(case)
    xi, xl = torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)
    enc = ip.label_encoder("MapillarySegmentation")
    t = eic.EVAL_SIZE
    want_img = f["img_" + name].astype(np.float32).transpose(2, 0, 1)
    for v, (with_enc, ign) in enumerate(eic.VARIANTS):
        tf = ip.ResizeHeightCenterCropPad(t, ignore_index=ign)
        want_lab = f["lab_" + name][v].astype(np.int64)
        for warm in (False, True):                                                     # cold tables, then the cached ones
            got_img, got_lab = tf(xi, xl, enc if with_enc else None)
            assert np.array_equal(got_img.cpu().numpy(), want_img), (name, with_enc, ign, warm)
            assert np.array_equal(got_lab.cpu().numpy(), want_lab), (name, with_enc, ign, warm)
        bi = torch.full((2, 3, t, t), -1.0, device=DEV)
        bl = torch.full((2, t, t), -1, dtype=torch.int64, device=DEV)
        tf(xi, xl, enc if with_enc else None, out_img=bi[0], out_lab=bl[0])
        assert np.array_equal(bi[0].cpu().numpy(), want_img) and np.array_equal(bl[0].cpu().numpy(), want_lab)
        assert (bi[1] == -1).all() and (bl[1] == -1).all()
    assert ip.ResizeHeightCenterCropPad(t).ignore_index == 0                           # the reference's default: padding is class 0


def _mobilenet():
    import deepv3_common as dc
    from mrfp_amd import synth
    from mrfp_amd.config import cfg
    from mrfp_amd.network import deepv3
    cfg.MODEL.ACT_DTYPE = torch.float32
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    with contextlib.redirect_stdout(io.StringIO()):
        m = deepv3.DeepMobileNetV3PlusD(None, 19, crit, crit)
    m.load_state_dict(synth.synth_state_dict(dc.spec("DeepMobileNetV3PlusD"), seed=0))
    return m.to(DEV)


def test_eval_batches_feed_evaluate():
    """The reference's batch-1 eval loop in one line: the histogram equals the one from tensors the numpy restatement prepared."""
    from mrfp_amd import harness
    from mrfp_amd import input_pipeline as ip
    model = _mobilenet()
    enc = ip.label_encoder("CityscapesSegmentation")
    host = [eic.sample(224, 160, seed=s, ids=34) for s in (41, 42)]
    samples = [(torch.from_numpy(i).to(DEV), torch.from_numpy(l).to(DEV)) for i, l in host]
    hist, miou, dropped = harness.evaluate(model, harness.eval_batches(samples, ip.EvalTransform(), enc))
    ref = []
    for i, l in host:
        a, b = eic.eval_transform(i, l, enc.table)
        ref.append((torch.from_numpy(a)[None].to(DEV), torch.from_numpy(b)[None].to(DEV)))
    hist_r, miou_r, dropped_r = harness.evaluate(model, ref)
    assert dropped == dropped_r == 0 and hist.sum() == sum(int((enc.table[l] < 19).sum()) for _, l in host) > 0
    assert np.array_equal(hist, hist_r) and miou == miou_r
    first = next(iter(harness.eval_batches(samples[:1], ip.ResizeHeightCenterCropPad(32), ip.label_encoder("MapillarySegmentation"))))
    assert tuple(first[0].shape) == (1, 3, 32, 32) and tuple(first[1].shape) == (1, 32, 32) and first[1].dtype == torch.int64
