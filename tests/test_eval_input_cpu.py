"""No-GPU checks of the evaluation input path: the label tables of the seven dataset classes against the recorded ones
(tests/golden/eval_input.npz, made from the reference by tests/golden/make_golden_eval_input.py), LabelEncoder's construction
against a literal replay of the loops, the numpy restatement of ResizeHeightCenterCropPad (tests/eval_input_common.py) against
PIL and the fixture, and the host-side argument checks of the three C entries."""
import ctypes

import numpy as np
import pytest

from mrfp_amd import _lib, build
from mrfp_amd import input_pipeline as ip

import eval_input_common as eic


def test_preset_tables_equal_the_recorded_ones():
    f = eic.fixture()
    assert tuple(str(n) for n in f["names"]) == eic.DATASETS and f["tables"].shape == (7, 256)
    for name, want in zip(eic.DATASETS, f["tables"]):
        for spelled in (name, name[:-len("Segmentation")]):
            enc = ip.label_encoder(spelled)
            assert enc.table.dtype == np.uint8 and np.array_equal(enc.table, want), spelled
    with pytest.raises(KeyError):
        ip.label_encoder("KittiSegmentation")
    t = {n: f["tables"][i] for i, n in enumerate(eic.DATASETS)}
    # the kept quirks, spelled out
    assert np.array_equal(t["BDD100kSegmentation"], np.arange(256))                       # encode_segmap is never called there
    assert np.array_equal(t["CityscapesSegmentation"][34:], np.arange(34, 256))           # ids in neither list stay
    assert t["GTAVSegmentation"][34] == 255 and np.array_equal(t["GTAVSegmentation"][35:], np.arange(35, 256))
    assert (t["SynthiaSegmentation"] != 255).sum() == 19                                  # an all-255 map to start from
    assert np.array_equal(t["MapillarySegmentation"][66:], np.arange(66, 256)) and (t["MapillarySegmentation"][:66] < 19).sum() == 25


LISTS = [
    ([0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30, -1], [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33], 255),
    ([0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30, -1], list(range(19)), 255),    # chains: a written train id is a later valid id
    ([0, 13, 14, 22], [3, 4, 2, 21, 5, 7, 15, 9, 6, 16, 1, 10, 17, 8, 18, 19, 20, 12, 11], 255),
    ([5, 300, -7], [9, 8, 7, 0, 250], 11),                                                # ids no uint8 holds; ignore_index is a valid id
    ([], [], 255),
]


@pytest.mark.parametrize("case", range(len(LISTS)))
def test_encoder_from_lists_equals_the_literal_loops(case):
    void, valid, ignore = LISTS[case]
    enc = ip.LabelEncoder.from_lists(void, valid, ignore)
    for seed in (0, 1):
        m = eic.all_values_map(seed=seed)
        assert len(np.unique(m)) == 256
        assert np.array_equal(enc.table[m], eic.encode_lists(m, void, valid, ignore))


def test_encoder_from_map_equals_the_literal_loops():
    m = eic.all_values_map(seed=3)
    cm = {i: 255 for i in range(66)}
    cm.update({13: 0, 24: 0, 2: 1, 65: 18, 300: 4, -1: 5})
    assert np.array_equal(ip.LabelEncoder.from_map(cm).table[m], eic.encode_map(m, cm))
    sm = dict(zip([3, 4, 2, 21, 5], range(5)))
    assert np.array_equal(ip.LabelEncoder.from_map(sm, default=255).table[m], eic.encode_map(m, sm, 255))
    with pytest.raises(ValueError):
        ip.LabelEncoder(np.arange(255))
    with pytest.raises(ValueError):
        ip.LabelEncoder.from_map({1: 256})


def test_geometry_of_the_cases():
    want = {"half_even": (21, 0, 2), "diff3": (19, 0, 2), "diff1": (17, 0, 0), "exact": (16, 0, 0), "narrow": (12, 4, -2),
            "pad_only": (15, 1, 0), "upscale": (20, 0, 2), "down16": (18, 0, 1), "same_height": (20, 0, 2)}
    for name, w, h in eic.CASES:
        assert eic.geometry(w, h, eic.EVAL_SIZE) == want[name], name
        assert ip.ResizeHeightCenterCropPad(eic.EVAL_SIZE).geometry(w, h) == want[name], name
    assert ip.ResizeHeightCenterCropPad(16).ignore_index == 0            # CenterCropPad's default, which main.py:779 keeps


@pytest.mark.parametrize("case", range(len(eic.CASES)))
def test_restatement_equals_fixture_and_pil(case):
    f = eic.fixture()
    name = eic.CASES[case][0]
    img, lab = eic.case_sample(case)
    mapillary = f["tables"][eic.DATASETS.index("MapillarySegmentation")]
    try:
        import PIL.Image  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    for v, (enc, ign) in enumerate(eic.VARIANTS):
        table = mapillary if enc else None
        got_img, got_lab = eic.rhccp_numpy(img, lab, eic.EVAL_SIZE, ign, table)
        assert np.array_equal(got_img, f["img_" + name]) and np.array_equal(got_lab, f["lab_" + name][v]), (name, enc, ign)
        if have_pil:
            pil_img, pil_lab = eic.rhccp_pil(img, lab, eic.EVAL_SIZE, ign, table)
            assert np.array_equal(got_img, pil_img) and np.array_equal(got_lab, pil_lab), (name, enc, ign)
    if name == "narrow":                 # 2 outside columns (0), 4 pad columns (ignore_index), then the first 10 content columns
        row = f["lab_narrow"][3][5]
        assert list(row[:6]) == [0, 0, 255, 255, 255, 255] and np.array_equal(row[6:], lab[eic.io.nearest_table(40, 16)[5]][eic.io.nearest_table(30, 12)[:10]])
        assert not f["img_narrow"][:, :6].any()
    if name == "pad_only":
        assert list(f["lab_pad_only"][3][5][:1]) == [255] and list(f["lab_pad_only"][2][5][:1]) == [0]


@pytest.fixture(scope="module")
def cdll():
    build.build()
    return _lib.lib()


def test_c_entries_check_their_arguments_before_any_launch(cdll):
    """Null pointers, negative sizes, crop / pad ranges beyond int32: nonzero, the entry named in mrfp_last_error, nothing
    launched (the pointers are host memory and there may be no device at all)."""
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255
    q = p + 1024
    big = 2147483647
    ok = (p, p, p, p, 4, 4, 4, 4, 0, 0, 0, 0, 4, 4, 0, None, q, q, None)     # mrfp_eval_assemble with valid arguments
    assert [n for n in _lib.ARG_NAMES["mrfp_eval_assemble"]] == ["img", "lab", "ytab", "xtab", "Hs", "Ws", "Hl", "Wl", "pad_x", "pad_y",
                                                                  "x1", "y1", "Hc", "Wc", "pad_label", "lut", "out_img", "out_lab", "stream"]

    def ea(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[_lib.ARG_NAMES["mrfp_eval_assemble"].index(k)] = v
        return tuple(a)
    cases = [
        ("mrfp_label_lut_u8", (None, p, 16, q, None), b"label_lut_u8: null argument"),
        ("mrfp_label_lut_u8", (p, None, 16, q, None), b"label_lut_u8: null argument"),
        ("mrfp_label_lut_u8", (p, p, 16, None, None), b"label_lut_u8: null argument"),
        ("mrfp_label_lut_u8", (p, p, -1, q, None), b"label_lut_u8: negative size -1"),
        ("mrfp_label_lut_u8", (p, p + 8, 16, q, None), b"label_lut_u8: src and dst overlap"),
        ("mrfp_label_encode_i64", (None, q, p, 16, None), b"label_encode_i64: null argument"),
        ("mrfp_label_encode_i64", (p, None, None, 16, None), b"label_encode_i64: null argument"),
        ("mrfp_label_encode_i64", (p, None, q, -5, None), b"label_encode_i64: negative size -5"),
        ("mrfp_label_encode_i64", (p, None, q + 4, 16, None), b"label_encode_i64: dst_i64 is not 8-byte aligned"),
        ("mrfp_eval_assemble", ea(img=None), b"eval_assemble: null argument"),
        ("mrfp_eval_assemble", ea(xtab=None), b"eval_assemble: null argument"),
        ("mrfp_eval_assemble", ea(out_lab=None), b"eval_assemble: null argument"),
        ("mrfp_eval_assemble", ea(Hc=-4), b"eval_assemble: bad sizes"),
        ("mrfp_eval_assemble", ea(Ws=0), b"eval_assemble: bad sizes"),
        ("mrfp_eval_assemble", ea(Wl=65536), b"eval_assemble: bad sizes"),
        ("mrfp_eval_assemble", ea(pad_x=-1), b"eval_assemble: negative padding"),
        ("mrfp_eval_assemble", ea(pad_label=256), b"eval_assemble: pad_label 256"),
        ("mrfp_eval_assemble", ea(x1=big), b"overflows int32"),
        ("mrfp_eval_assemble", ea(y1=big - 3), b"overflows int32"),
        ("mrfp_eval_assemble", ea(pad_x=big // 2), b"overflows int32"),
        ("mrfp_eval_assemble", ea(x1=-big, pad_x=5), b"overflows int32"),
        ("mrfp_eval_assemble", ea(y1=-big - 1), b"overflows int32"),
    ]
    for name, args, text in cases:
        assert len(args) == len(_lib.ARG_NAMES[name]), name
        rc = getattr(cdll, name)(*args)
        err = cdll.mrfp_last_error()
        assert rc != 0 and text in err and err.startswith(name[len("mrfp_"):].encode()), (name, args, rc, err)
    # n == 0 is valid and launches nothing: zero even without a device
    assert cdll.mrfp_label_lut_u8(p, p, 0, q, None) == 0 and cdll.mrfp_label_encode_i64(p, None, q, 0, None) == 0


def test_transforms_refuse_host_tensors():
    import torch
    img, lab = torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(8, 8, dtype=torch.uint8)
    enc = ip.label_encoder("GTAVSegmentation")
    for f in (lambda: enc(lab), lambda: enc.to_int64(lab), lambda: ip.EvalTransform()(img, lab), lambda: ip.ResizeHeightCenterCropPad(16)(img, lab)):
        with pytest.raises(_lib.MrfpHipError):
            f()
