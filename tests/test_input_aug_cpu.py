"""No-GPU checks of the augmentation half of the input path: the numpy restatements of tests/input_aug_common.py against PIL and
numpy themselves (0 differing bytes / bits), the host side of mrfp_amd/input_pipeline.py (rotate_plan, the draws, the geometry)
against the restatements and against a transcript of the reference's random calls, and the refusals of the new C-ABI entries."""
import ctypes
import random

import numpy as np
import pytest
import torch

import input_aug_common as iac
from oracle import input_oracle as io


@pytest.mark.parametrize("H,W", iac.SHAPES)
def test_rotate_restatement_equals_pil(H, W):
    pytest.importorskip("PIL.Image")
    img, lab = iac.sample(W, H, seed=H)
    assert set(np.unique(lab)) >= set(range(19)) | {255}
    kinds = set()
    for angle in iac.ANGLES:
        want_img, want_lab = iac.rotate_pil(img, lab, angle)
        got_img, got_lab = iac.rotate_numpy(img, lab, angle)
        assert int((want_img != got_img).sum()) == 0 and int((want_lab != got_lab).sum()) == 0, (H, W, angle)
        kinds.add(iac.rotate_matrix(W, H, angle)[0])
    assert kinds == ({"copy", "rot90", "rot180", "rot270", "affine"} if H == W else {"copy", "rot180", "affine"})


def test_rotate_plan_is_pils_dispatch_and_matrix():
    from mrfp_amd import input_pipeline as ip
    names = {ip.ROT_AFFINE: "affine", ip.ROT_COPY: "copy", ip.ROT_90: "rot90", ip.ROT_180: "rot180", ip.ROT_270: "rot270"}
    for H, W in iac.SHAPES + ((1024, 2048),):
        for angle in iac.ANGLES + (-1e-20, 1e-20, 359.99999999999997, -90, -180.0, 450):
            kind, m = iac.rotate_matrix(W, H, angle)
            mode, pm = ip.rotate_plan(W, H, angle)
            assert names[mode] == kind, (H, W, angle)
            if kind == "affine":                            # equal as bit patterns: -0.0 and 0.0 differ
                assert np.array_equal(np.array(pm, np.float64).view(np.uint64), np.array(m, np.float64).view(np.uint64)), (H, W, angle)


def test_rotate_corner_fill_is_class_zero():
    """The kept quirk: no fillcolor, so the corners a rotation uncovers are label 0, not 255."""
    lab = np.full((20, 30), 7, np.uint8)
    _, out = iac.rotate_numpy(np.zeros((20, 30, 3), np.uint8), lab, 30.0)
    assert out[0, 0] == 0 and out[-1, -1] == 0 and out[10, 15] == 7 and set(np.unique(out)) == {0, 7}


def test_fixed_point_guard_raises():
    from mrfp_amd import _lib, build
    from mrfp_amd import input_pipeline as ip
    kind, m = iac.rotate_matrix(40000, 100, 7.3)
    assert kind == "affine" and not iac.fixed_range_ok(40000, 100, m)
    with pytest.raises(_lib.MrfpHipError, match="32768"):
        ip.rotate_plan(40000, 100, 7.3)
    assert ip.rotate_plan(32000, 100, 7.3)[0] == ip.ROT_AFFINE and ip.rotate_plan(40000, 100, 180)[0] == ip.ROT_180
    # the C entry checks for itself, on the host, before any launch (pointers into a host buffer: nothing runs)
    build.build()
    cdll = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255
    rc = cdll.mrfp_affine_u8(p, p + 64, p + 128, p + 192, 100, 40000, 0, 0, *m, None)
    assert rc == -1 and b"outside the 16.16 fixed-point range" in cdll.mrfp_last_error()


def test_new_entries_refuse_bad_arguments_before_any_launch():
    from mrfp_amd import _lib, build
    build.build()
    cdll = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255
    ident = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    cases = [
        ("mrfp_affine_u8", (None, p, p + 64, p + 128, 4, 4, 0, 0, *ident, None), b"affine_u8: null or aliased argument"),
        ("mrfp_affine_u8", (p, p + 64, p, p + 128, 4, 4, 0, 0, *ident, None), b"affine_u8: null or aliased argument"),
        ("mrfp_affine_u8", (p, p + 64, p + 128, p + 192, 0, 4, 0, 0, *ident, None), b"affine_u8: bad sizes 0x4"),
        ("mrfp_affine_u8", (p, p + 64, p + 128, p + 192, 4, 65536, 0, 0, *ident, None), b"affine_u8: bad sizes 4x65536"),
        ("mrfp_affine_u8", (p, p + 64, p + 128, p + 192, 4, 4, 5, 0, *ident, None),
         b"affine_u8: mode 5 (0 affine, 1 copy, 2 / 3 / 4 the 90 / 180 / 270 degree transposes)"),
        ("mrfp_affine_u8", (p, p + 64, p + 128, p + 192, 4, 5, 2, 0, *ident, None),
         b"affine_u8: the 90 / 270 degree transposes keep the size of square images only (4x5)"),
        ("mrfp_affine_u8", (p, p + 64, p + 128, p + 192, 4, 4, 0, 0, float("nan"), 0.0, 0.0, 0.0, 1.0, 0.0, None), None),
        ("mrfp_u8hwc_to_f32chw_norm", (p, p + 64, 0, 4, 0.5, 0.5, 0.5, 1.0, 1.0, 1.0, None), b"u8hwc_to_f32chw_norm: bad arguments"),
        ("mrfp_u8hwc_to_f32chw_norm", (p, p + 64, 2, 2, 0.5, 0.5, 0.5, 1.0, 0.0, 1.0, None),
         b"u8hwc_to_f32chw_norm: finite means and finite non-zero standard deviations expected"),
    ]
    for name, args, text in cases:
        assert len(args) == len(_lib.ARG_NAMES[name]), name
        rc = getattr(cdll, name)(*args)
        msg = cdll.mrfp_last_error()
        assert rc == -1 and (msg == text if text is not None else b"fixed-point range" in msg), (name, rc, msg)
    # the double arguments reach the library as doubles (the header parser maps them)
    assert cdll.mrfp_affine_u8.argtypes[8:14] == [ctypes.c_double] * 6


def test_python_surface_refuses_cpu_tensors_and_wrong_dtypes():
    from mrfp_amd import _lib
    from mrfp_amd import input_pipeline as ip
    img, lab = torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(8, 8, dtype=torch.uint8)
    with pytest.raises(_lib.MrfpHipError, match="rotate"):
        ip.rotate(img, lab, 10.0)
    with pytest.raises(_lib.MrfpHipError, match="contrast"):
        ip.contrast(img)
    t = ip.ScaleCropTransform(8, 8)
    with pytest.raises(_lib.MrfpHipError, match="ScaleCropTransform"):
        t(img, lab, t.draw(8, 8, random.Random(0)))
    with pytest.raises(_lib.MrfpHipError, match="FixScaleCropTransform"):
        ip.FixScaleCropTransform(8)(img.float(), lab)
    with pytest.raises(_lib.MrfpHipError, match="CropTransform"):
        c = ip.CropTransform.p2(4, 6)
        c(img, lab, c.draw(8, 8, random.Random(0)))
    for bad in (((0.5, 0.5), (1, 1, 1)), ((0.5, 0.5, 0.5), (1, 0, 1)), 3):
        with pytest.raises(ValueError):
            ip.ScaleCropTransform(8, 8, normalize=bad)
        with pytest.raises(ValueError):
            ip.FixScaleCropTransform(8, normalize=bad)


def test_random_scale_crop_equals_pil():
    pytest.importorskip("PIL.Image")
    seen = set()
    for (H, W), base, crop, fill in (((96, 128), 64, 48, 0), ((200, 150), 40, 64, 255), ((37, 53), 30, 30, 7)):
        img, lab = iac.sample(W, H, seed=W)
        r = random.Random(H)
        for _ in range(6):
            short = r.randint(int(base * 0.5), int(base * 2.0))
            scaled, pad = iac.scale_crop_geometry(W, H, short, crop)
            xy = (r.randint(0, scaled[0] + pad[0] - crop), r.randint(0, scaled[1] + pad[1] - crop))
            kw = dict(flip=False, jitter=None, degrees=None, scaled=scaled, pad=pad, crop=xy, blur=None, crop_size=crop, fill=fill)
            want_img, want_lab = iac.scale_crop_pil(img, lab, **kw)
            got_img, got_lab = iac.scale_crop_numpy(img, lab, **kw)
            assert np.array_equal(want_img, got_img) and np.array_equal(want_lab.astype(np.int64), got_lab), (H, W, short)
            seen.add(bool(pad[0] or pad[1]))
            if pad[1] and xy[1] + crop > scaled[1]:
                assert (got_lab[scaled[1] - xy[1]:] == fill).all() and (got_img[:, scaled[1] - xy[1]:] == 0).all()
    assert seen == {True, False}


def test_scale_crop_composition_restatement_equals_pil():
    """Flip, jitter, rotation, blur, contrast and normalise together, for seeded draws of the product's own draw()."""
    pytest.importorskip("PIL.Image")
    from mrfp_amd import input_pipeline as ip
    img, lab = iac.sample(128, 96, seed=3)
    t = ip.ScaleCropTransform(64, 48, fill=255, rotate_degree=15, jitter=True, contrast=True, normalize=iac.IMAGENET)
    r, nr = random.Random(5), np.random.RandomState(5)
    draws = [t.draw(128, 96, r, nr) for _ in range(6)]
    assert any(d.jitter for d in draws) and any(d.blur is not None for d in draws) and any(d.flip for d in draws)
    for d in draws:
        kw = dict(iac.draw_kwargs(d), crop_size=48, fill=255, contrast=True, normalize=iac.IMAGENET)
        want_img, want_lab = iac.scale_crop_pil(img, lab, **kw)
        got_img, got_lab = iac.scale_crop_numpy(img, lab, **kw)
        assert np.array_equal(want_img.view(np.uint32), got_img.view(np.uint32)), d
        assert np.array_equal(want_lab.astype(np.int64), got_lab), d


def test_fix_scale_crop_equals_pil_and_geometry():
    pytest.importorskip("PIL.Image")
    from mrfp_amd import input_pipeline as ip
    for (H, W), crop in (((60, 90), 48), ((90, 60), 48), ((30, 37), 24), ((64, 64), 32), ((50, 50), 50)):
        img, lab = iac.sample(W, H, seed=crop)
        assert ip.FixScaleCropTransform(crop).geometry(W, H) == iac.fix_scale_crop_geometry(W, H, crop)
        for contrast, norm in ((False, None), (True, iac.IMAGENET)):
            want_img, want_lab = iac.fix_scale_crop_pil(img, lab, crop, contrast, norm)
            got_img, got_lab = iac.fix_scale_crop_transform_numpy(img, lab, crop, contrast, norm)
            assert np.array_equal(want_img.view(np.uint32), got_img.view(np.uint32)), (H, W, crop)
            assert np.array_equal(want_lab.astype(np.int64), got_lab), (H, W, crop)
    assert iac.fix_scale_crop_geometry(37, 30, 24) == (29, 24, 2, 0)          # round(2.5): half to even


def test_contrast_restatement_equals_pil_at_factor_two():
    """ImageEnhance.Contrast(img).enhance(2.0): the blend with the rounded L mean, clipped at both ends."""
    Image = pytest.importorskip("PIL.Image")
    for H, W in ((37, 53), (64, 64)):
        img, _ = iac.sample(W, H, seed=W)
        want = np.array(io.jitter_pil(Image.fromarray(img), "contrast", 2.0))
        got = io.jitter_u8(img, "contrast", 2.0)
        assert np.array_equal(want, got) and (got == 0).any() and (got == 255).any()


def test_random_crop_p2_equals_pil_and_names_the_width_first():
    Image = pytest.importorskip("PIL.Image")
    from mrfp_amd import input_pipeline as ip
    img, lab = iac.sample(53, 37, seed=1)
    t = ip.CropTransform.p2(20, 12)                                       # RandomCrop_p2(crop_sizew=20, crop_sizeh=12)
    assert (t.crop_size, t.base_size) == (20, 12)
    r, ref = random.Random(3), random.Random(3)
    for _ in range(8):
        d = t.draw(53, 37, r, np.random.RandomState(0))
        ref.random(), ref.random()                                        # flip and jitter gates of the composition around it
        x0, y0 = ref.randint(0, 53 - 20), ref.randint(0, 37 - 12)         # dataloaders.py:247-248
        assert d.crop == (x0, y0)
        if ref.random() < 0.5:
            ref.random()
        box = (x0, y0, x0 + 20, y0 + 12)                                   # :250-252
        want_img, want_lab = np.array(Image.fromarray(img).crop(box)), np.array(Image.fromarray(lab).crop(box))
        assert np.array_equal(want_img, img[y0:y0 + 12, x0:x0 + 20]) and np.array_equal(want_lab, lab[y0:y0 + 12, x0:x0 + 20])
        assert want_img.shape == (12, 20, 3)


def test_normalize_restatement_is_numpy_exhaustively():
    """All 256 byte values x 3 channels with the ImageNet constants of main.py:140: the stated precisions are numpy's."""
    img = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, 2)          # [256,1,3]
    mean, std = iac.IMAGENET
    want = iac.normalize_reference(img, mean, std)
    got = iac.normalize_numpy(img, mean, std)
    assert want.dtype == got.dtype == np.float32 and np.array_equal(want.view(np.uint32), got.view(np.uint32))
    # the float64 steps matter: an all-float32 evaluation differs somewhere
    f = np.float32
    v32 = ((img.astype(f) / f(255.0)) - np.asarray(mean, f)) / np.asarray(std, f)
    assert (v32.view(np.uint32) != want.view(np.uint32)).any()


def _transcript(w, h, base, crop, degree, jitter, r, nr):
    """The random / np.random calls of the classes in the composition's order, statement by statement."""
    rec = {}
    rec["flip"] = r.random() < 0.5                                        # RandomHorizontalFlip :145
    rec["jitter"] = None
    if jitter and r.random() < 0.5:                                       # ColorJitter.__call__ :655
        b, c, s, hu = 0.5, 0.2, 0.2, 0.3                                  # brightness, contrast, saturation, hue (main.py:412)
        tr = [("brightness", nr.uniform(max(0, 1 - b), 1 + b)), ("contrast", nr.uniform(max(0, 1 - c), 1 + c)),
              ("saturation", nr.uniform(max(0, 1 - s), 1 + s)), ("hue", nr.uniform(-hu, hu))]      # :624-639
        nr.shuffle(tr)                                                    # :643
        rec["jitter"] = [(k, float(v)) for k, v in tr]
    rec["degrees"] = r.uniform(-1 * degree, degree) if degree is not None else None      # RandomRotate :160
    short = r.randint(int(base * 0.5), int(base * 2.0))                   # RandomScaleCrop :190
    rec["scaled"], rec["pad"] = iac.scale_crop_geometry(w, h, short, crop)
    W2, H2 = rec["scaled"][0] + rec["pad"][0], rec["scaled"][1] + rec["pad"][1]
    rec["crop"] = (r.randint(0, W2 - crop), r.randint(0, H2 - crop))      # :208-209
    rec["blur"] = None
    if r.random() < 0.5:                                                  # RandomGaussianBlur :172
        rec["blur"] = r.random()                                          # :174
    return rec


@pytest.mark.parametrize("degree,jitter", [(None, False), (10, False), (None, True), (15.5, True)])
def test_draw_consumes_the_streams_as_the_classes_do(degree, jitter):
    from mrfp_amd import input_pipeline as ip
    t = ip.ScaleCropTransform(40, 64, rotate_degree=degree, jitter=jitter)
    r1, n1, r2, n2 = random.Random(11), np.random.RandomState(11), random.Random(11), np.random.RandomState(11)
    for w, h in ((150, 200), (128, 96), (70, 70)) * 4:
        d = t.draw(w, h, r1, n1)
        rec = _transcript(w, h, 40, 64, degree, jitter, r2, n2)
        assert iac.draw_kwargs(d) == rec, (w, h)
    assert r1.random() == r2.random() and n1.uniform() == n2.uniform()    # the same amounts consumed


def test_golden_cases_follow_the_geometry():
    img, _ = iac.golden_source()
    h, w = img.shape[:2]
    for case in iac.GOLDEN_TRAIN:
        short = min(case["scaled"])
        assert iac.scale_crop_geometry(w, h, short, iac.GOLDEN_CROP) == (case["scaled"], case["pad"]), case
        x1, y1 = case["crop"]
        assert 0 <= x1 <= case["scaled"][0] + case["pad"][0] - iac.GOLDEN_CROP and 0 <= y1 <= case["scaled"][1] + case["pad"][1] - iac.GOLDEN_CROP
