"""No-GPU checks of the prediction path: the new prototypes and their refusals (all before any launch), the grid query,
LabelEncoder.inverse, the ops / harness argument errors, and the restatement of the kernel's interpolation against fp64 on the inputs
of the GPU tests -- which fixes, here and not on the GPU, how many pixels an fp64 comparison may leave out."""
import ctypes

import numpy as np
import pytest
import torch

from mrfp_amd import _lib, build, input_pipeline as ip

import predict_common as pc


@pytest.fixture(scope="module")
def cdll():
    build.build()
    return _lib.lib()


def test_new_prototypes_declared_and_exported(cdll):
    protos = _lib.parse_header()
    for name, nargs in (("mrfp_upsample_argmax", 18), ("mrfp_colorize_u8", 7), ("mrfp_upsample_argmax_nblocks", 3)):
        assert name in protos and len(protos[name][1]) == nargs and hasattr(cdll, name), name
    assert protos["mrfp_upsample_argmax_nblocks"][0] is ctypes.c_int64
    assert _lib.ARG_NAMES["mrfp_upsample_argmax"][-7:] == ["pred", "conf", "hist", "per_image", "ws", "loss_acc", "stream"]
    assert _lib.ARG_NAMES["mrfp_colorize_u8"] == ["pred", "palette", "image", "out", "npix", "a", "stream"]


def test_grid_query_obeys_the_cap(cdll):
    nb = cdll.mrfp_upsample_argmax_nblocks
    assert nb(3, 456, 456) == 3 * 682
    assert nb(1, 768, 768) == 2048 and nb(16, 768, 768) == 16 * 128 and nb(1, 1024, 2048) == 2048
    assert nb(2, 17, 26) == 2 * 2 and nb(1, 1, 1) == 1 and nb(1, 16, 16) == 1 and nb(1, 16, 17) == 2
    assert nb(4096, 64, 64) == 4096                   # more images than the cap: one workgroup each
    for B in (1, 2, 3, 5, 16, 100):
        for H, W in ((1, 1), (9, 9), (456, 456), (768, 768), (1024, 2048)):
            n = nb(B, H, W)
            assert n % B == 0 and B <= n <= max(B, 2048) and n // B <= -(-H * W // 256), (B, H, W, n)
    assert nb(0, 4, 4) == 0 and nb(1, 0, 4) == 0


def test_refusals_come_before_any_launch(cdll):
    """pointers into a host buffer: nothing may be launched, so this needs no GPU"""
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    ua, col = cdll.mrfp_upsample_argmax, cdll.mrfp_colorize_u8

    def refused(fn, args, text):
        rc = fn(*args)
        assert rc == -1 and text in cdll.mrfp_last_error(), (args, rc, cdll.mrfp_last_error())

    #                 P  ld  target dtype B  Hi Wi H  W  C   ignore pred conf hist per_image ws loss_acc stream
    refused(ua, (p, 24, p, 99, 1, 2, 2, 4, 4, 19, 255, p, None, None, 0, None, None, None), b"upsample_argmax: unknown dtype 99")
    refused(ua, (p, 19, p, 0, 1, 2, 2, 4, 4, 19, 255, p, None, None, 0, None, None, None), b"channel-padded")      # fp32: ld % 4
    refused(ua, (p, 28, p, 1, 1, 2, 2, 4, 4, 19, 255, p, None, None, 0, None, None, None), b"channel-padded")      # bf16: ld % 8
    refused(ua, (p, 16, p, 1, 1, 2, 2, 4, 4, 19, 255, p, None, None, 0, None, None, None), b"channel-padded")      # pitch below the classes
    refused(ua, (p + 4, 24, p, 0, 1, 2, 2, 4, 4, 19, 255, p, None, None, 0, None, None, None), b"channel-padded")  # P not 16-byte aligned
    refused(ua, (p, 72, p, 0, 1, 2, 2, 4, 4, 65, 255, p, None, None, 0, None, None, None), b"1 <= C <= 64")
    refused(ua, (p, 24, p, 0, 1, 2, 2, 4, 4, 0, 255, p, None, None, 0, None, None, None), b"1 <= C <= 64")
    refused(ua, (p, 24, p, 0, 1, 2, 2, 4, 4, 19, 255, None, None, None, 0, None, None, None), b"no output requested")
    refused(ua, (p, 24, None, 0, 1, 2, 2, 4, 4, 19, 255, p, None, p, 0, None, None, None), b"hist given without target")
    refused(ua, (p, 24, None, 0, 1, 2, 2, 4, 4, 19, 255, p, None, None, 0, p, p, None), b"loss_acc given without target")
    refused(ua, (p, 24, p, 0, 1, 2, 2, 4, 4, 19, 255, p, None, None, 0, None, p, None), b"loss_acc given without ws")
    refused(ua, (p, 24, p, 0, 0, 2, 2, 4, 4, 19, 255, p, None, None, 0, None, None, None), b"bad arguments")
    refused(ua, (p, 24, p, 0, 1, 2, 2, 0, 4, 19, 255, p, None, None, 0, None, None, None), b"bad arguments")
    refused(ua, (None, 24, p, 0, 1, 2, 2, 4, 4, 19, 255, p, None, None, 0, None, None, None), b"bad arguments")
    refused(ua, (p, 24, p, 0, 1, 2, 2, 1 << 16, 1 << 16, 19, 255, p, None, None, 0, None, None, None), b"sizes out of range")
    refused(col, (p, p, None, p, 16, 257, None), b"blend weight")
    refused(col, (p, p, p, p, 16, -1, None), b"blend weight")
    refused(col, (None, p, None, p, 16, 256, None), b"null argument")
    refused(col, (p, p, None, p, -1, 256, None), b"negative size")
    assert col(p, p, None, p, 0, 256, None) == 0                       # nothing to do, nothing launched


def test_ops_refuse_host_tensors_and_bad_arguments():
    from mrfp_amd import ops
    z = pc.to_device(pc.scores("c19_ld32", pc.F32), "cpu")
    with pytest.raises(_lib.MrfpHipError):
        ops.upsample_argmax(z, (17, 26), 19)
    with pytest.raises(_lib.MrfpHipError):
        ops.colorize(torch.zeros(4, dtype=torch.uint8), torch.zeros(256, 3, dtype=torch.uint8))
    r = ops.Prediction(None, None, None, None)
    assert r._fields == ("pred", "conf", "hist", "loss_acc")


def test_label_encoder_inverse():
    void, valid = [0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30, -1], [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28,
                                                                            31, 32, 33]
    enc = ip.LabelEncoder.from_lists(void, valid)
    inv = enc.inverse()
    assert isinstance(inv, ip.LabelEncoder) and inv is not enc and inv.table.dtype == np.uint8
    assert [int(inv.table[i]) for i in range(len(valid))] == valid
    city = ip.label_encoder("CityscapesSegmentation")
    assert np.array_equal(city.table, enc.table)
    assert [int(v) for v in city.inverse().table[:19]] == valid and int(city.inverse().table[255]) == 0
    assert int(city.inverse(fill=77).table[255]) == 77 and [int(v) for v in city.inverse(fill=77).table[:19]] == valid
    # one-to-one on the valid ids: the round trip is the identity there
    for i in valid:
        assert int(inv.table[enc.table[i]]) == i
    # many-to-one: the smallest id wins; train ids nothing maps to, and 255, take the fill
    many = ip.LabelEncoder.from_map({9: 2, 4: 2, 30: 2, 5: 0, 200: 1, 7: 255}, default=255)
    t = many.inverse(fill=9).table
    assert (int(t[0]), int(t[1]), int(t[2])) == (5, 200, 4) and int(t[255]) == 9 and int(t[3]) == 9
    assert set(np.unique(t).tolist()) == {4, 5, 9, 200}
    ident = ip.LabelEncoder(np.arange(256))
    assert np.array_equal(ident.inverse(fill=255).table, np.arange(256))      # 255 -> fill = 255
    assert int(ident.inverse().table[255]) == 0
    with pytest.raises(ValueError):
        enc.inverse(fill=256)


def test_harness_entry_points_exist():
    import inspect
    from mrfp_amd import harness
    assert list(inspect.signature(harness.predict).parameters) == ["model", "images", "fold", "want_conf"]
    assert list(inspect.signature(harness.validate).parameters) == ["model", "batches", "num_classes", "fold", "ignore_index", "per_image"]
    assert inspect.isgeneratorfunction(harness.predict)


def test_restatement_by_hand():
    """1 x 2 source, 1 x 3 output: columns (a, (a+b)/2, b); pad channel never read"""
    z = torch.tensor([[[[0.0, 4.0, 1e30, 1e30], [2.0, 1.0, 1e30, 1e30]]]])            # [1,1,2,4]: classes (0, 4) and (2, 1)
    got = pc.restated_z(z, 2, 1, 3)
    assert np.array_equal(got[0, 0], np.array([[0.0, 4.0], [1.0, 2.5], [2.0, 1.0]], dtype=np.float32))
    assert np.array_equal(pc.fp64_z(z, 2, 1, 3)[0, 0], np.array([[0.0, 4.0], [1.0, 2.5], [2.0, 1.0]]))
    up = pc.restated_z(z, 2, 4, 2)                                                    # out > 1 over a one-high source: rows repeat
    assert np.array_equal(up[0, 0], up[0, 3]) and np.array_equal(up[0, 0], np.array([[0.0, 4.0], [2.0, 1.0]], dtype=np.float32))


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=pc.dname)
def test_decidable_share_and_restatement_error(dtype):
    """On the inputs of the GPU tests: the share of pixels under the dtype's top-two gap stays under its cap (1 % fp32 / fp16, 5 %
    bf16), and on every other pixel the fp32 restatement -- hence the kernel -- has the fp64 arg-max.  The restated score itself stays
    within the rounding of its format of the fp64 one."""
    worst_share, worst_err = 0.0, 0.0
    for case in pc.CASES:
        name, B, Hi, Wi, H, W, C, _ = case
        z32, am64, decidable = pc.reference(name, dtype)
        share = 1.0 - decidable.mean()
        z64 = pc.fp64_z(pc.scores(name, dtype), C, H, W)
        err = np.abs(z32.astype(np.float64) - z64)
        scale = {pc.F32: 2.0 ** -23, pc.BF16: 2.0 ** -8, pc.F16: 2.0 ** -11}[dtype]
        bound = 5e-4 + scale * np.abs(z64)            # fp32 interpolation error (3.6e-4 measured at 192 -> 768) + half an ulp of the format
        assert (err <= bound).all(), (name, float((err - bound).max()))
        am32 = np.argmax(z32, axis=-1)
        assert np.array_equal(am32[decidable], am64[decidable]), name
        print("%s %s: %.3f %% of %d pixels under the gap, max |z32 - z64| %.3g" % (name, pc.dname(dtype), 100 * share, decidable.size, err.max()))
        worst_share, worst_err = max(worst_share, share), max(worst_err, float(err.max()))
        assert share <= pc.GAP_CAP[dtype], (name, share)
    print("%s: worst share %.3f %%, worst error %.3g" % (pc.dname(dtype), 100 * worst_share, worst_err))
