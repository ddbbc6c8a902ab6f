"""The augmentation half of the input path on the GPU (csrc/input.hip: affine_u8, u8hwc_to_f32chw_norm;
mrfp_amd/input_pipeline.py: rotate, contrast, ScaleCropTransform, FixScaleCropTransform, CropTransform.p2) against the PIL calls
of the reference's classes and numpy's Normalize: images equal bit for bit, labels as int64."""
import contextlib
import io as _io
import random

import numpy as np
import pytest
import torch

import input_aug_common as iac
from oracle import input_oracle as io

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


@pytest.mark.parametrize("H,W", iac.SHAPES)
def test_rotate_equals_pil(H, W):
    pytest.importorskip("PIL.Image")
    from mrfp_amd import input_pipeline as ip
    img, lab = iac.sample(W, H, seed=H)
    xi, xl = _dev(img, lab)
    for angle in iac.ANGLES:
        want_img, want_lab = iac.rotate_pil(img, lab, angle)
        got_img, got_lab = ip.rotate(xi, xl, angle)
        assert got_img.dtype == torch.uint8 and got_lab.dtype == torch.uint8 and got_img.data_ptr() != xi.data_ptr()
        assert int((got_img.cpu().numpy() != want_img).sum()) == 0, (H, W, angle)
        assert int((got_lab.cpu().numpy() != want_lab).sum()) == 0, (H, W, angle)


def test_rotate_walks_the_capped_grid():
    """More pixels than one sweep of the capped grid (8192 workgroups of 256 lanes): every lane takes a second pixel."""
    from mrfp_amd import input_pipeline as ip
    H, W = 1100, 2000
    assert H * W > 8192 * 256
    img, lab = iac.sample(W, H, seed=7)
    got_img, got_lab = ip.rotate(*_dev(img, lab), 7.3)
    want_img, want_lab = iac.rotate_numpy(img, lab, 7.3)
    assert np.array_equal(got_img.cpu().numpy(), want_img) and np.array_equal(got_lab.cpu().numpy(), want_lab)


def test_contrast_equals_pil_at_factor_two():
    Image = pytest.importorskip("PIL.Image")
    from mrfp_amd import input_pipeline as ip
    for H, W in ((37, 53), (64, 64)):
        img, _ = iac.sample(W, H, seed=W)
        want = np.array(io.jitter_pil(Image.fromarray(img), "contrast", 2.0))
        got = ip.contrast(_dev(img)[0])
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want) and (want == 0).any() and (want == 255).any()


@pytest.mark.parametrize("H,W,base,crop", [(96, 128, 64, 48), (200, 150, 40, 64)])
def test_scale_crop_transform_equals_pil(H, W, base, crop):
    pytest.importorskip("PIL.Image")
    from mrfp_amd import input_pipeline as ip
    img, lab = iac.sample(W, H, seed=base)
    xi, xl = _dev(img, lab)
    seen_pad = set()
    for variant, kw in enumerate((dict(rotate_degree=15, jitter=True, fill=255), dict(rotate_degree=10, contrast=True, normalize=iac.IMAGENET),
                                  dict())):
        t = ip.ScaleCropTransform(base, crop, **kw)
        r, nr = random.Random(9 + variant), np.random.RandomState(9 + variant)
        draws = [t.draw(W, H, r, nr) for _ in range(6)]
        for d in draws:
            ref = dict(iac.draw_kwargs(d), crop_size=crop, fill=kw.get("fill", 0), contrast=kw.get("contrast", False),
                       normalize=kw.get("normalize"))
            want_img, want_lab = iac.scale_crop_pil(img, lab, **ref)
            got_img, got_lab = t(xi, xl, d)
            assert got_img.dtype == torch.float32 and got_lab.dtype == torch.int64 and tuple(got_img.shape) == (3, crop, crop)
            assert np.array_equal(_bits(got_img.cpu().numpy()), _bits(want_img)), (variant, d)
            assert np.array_equal(got_lab.cpu().numpy(), want_lab.astype(np.int64)), (variant, d)
            seen_pad.add(bool(d.pad[0] or d.pad[1]))
    assert seen_pad == {True, False}                           # some draws pad (short_size < crop_size), some do not


def test_scale_crop_padding_and_transposes_with_flip():
    """Fixed draws: padding on the right and at the bottom only, with `fill`; the flip taken inside the rotation on the copy and
    the exact-transpose paths (square source: 90 / 270) and on the affine path (non-square 90)."""
    pytest.importorskip("PIL.Image")
    from mrfp_amd import input_pipeline as ip
    for (H, W) in ((64, 64), (60, 90)):
        img, lab = iac.sample(W, H, seed=2)
        xi, xl = _dev(img, lab)
        t = ip.ScaleCropTransform(40, 48, fill=255, rotate_degree=180)
        for degrees in (0.0, 90.0, 180.0, 270.0, -90.0, 33.3, None):
            for flip in (False, True):
                scaled, pad = iac.scale_crop_geometry(W, H, 30, 48)
                d = ip.ScaleCropDraw(flip, None, degrees, scaled, pad, (0, 0), None)
                want_img, want_lab = iac.scale_crop_pil(img, lab, **iac.draw_kwargs(d), crop_size=48, fill=255)
                got_img, got_lab = t(xi, xl, d)
                assert np.array_equal(_bits(got_img.cpu().numpy()), _bits(want_img)), (H, W, degrees, flip)
                assert np.array_equal(got_lab.cpu().numpy(), want_lab.astype(np.int64)), (H, W, degrees, flip)
                assert (got_lab[scaled[1]:] == 255).all() and (got_img[:, scaled[1]:] == 0).all() and pad[1] == 18


@pytest.mark.parametrize("H,W", [(60, 90), (90, 60)])
def test_fix_scale_crop_transform_equals_pil(H, W):
    pytest.importorskip("PIL.Image")
    from mrfp_amd import input_pipeline as ip
    img, lab = iac.sample(W, H, seed=W)
    xi, xl = _dev(img, lab)
    enc = ip.label_encoder("CityscapesSegmentation")
    for contrast, norm, table in ((False, None, None), (True, iac.IMAGENET, None), (True, iac.IMAGENET, enc.table)):
        t = ip.FixScaleCropTransform(48, contrast=contrast, normalize=norm)
        want_img, want_lab = iac.fix_scale_crop_pil(img, lab, 48, contrast, norm, table)
        for warm in (False, True):                             # cold tables, then the cached ones
            got_img, got_lab = t(xi, xl, enc if table is not None else None)
            assert np.array_equal(_bits(got_img.cpu().numpy()), _bits(want_img)), (contrast, warm)
            assert np.array_equal(got_lab.cpu().numpy(), want_lab.astype(np.int64)), (contrast, warm)


def test_normalize_store_is_numpy_on_every_byte():
    """All 256 byte values in each channel through the fused Normalize + ToTensor store: bit-equal to numpy's statements."""
    from mrfp_amd import input_pipeline as ip
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = np.stack([v, v[::-1], v.T], -1)
    lab = np.zeros((16, 16), np.uint8)
    for mean, std in (iac.IMAGENET, ((0.0, 0.5, 1.0), (1.0, 0.1, 3.0))):
        got, _ = ip.FixScaleCropTransform(16, normalize=(mean, std))(*_dev(img, lab))
        want = iac.normalize_reference(img, mean, std).transpose(2, 0, 1)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (mean, std)


def test_mixed_batch_through_out_slots():
    from mrfp_amd import input_pipeline as ip
    T = 48
    srcs = [iac.sample(w, h, seed=w) for h, w in [(96, 128), (80, 100), (60, 90), (70, 50)]]
    tts = [ip.ScaleCropTransform(64, T, rotate_degree=12, contrast=True, normalize=iac.IMAGENET), ip.CropTransform.p2(T, T),
           ip.FixScaleCropTransform(T, contrast=True, normalize=iac.IMAGENET), ip.ScaleCropTransform(40, T, fill=255, jitter=True)]
    r, nr = random.Random(1), np.random.RandomState(1)
    draws = [t.draw(i.shape[1], i.shape[0], r, nr) if hasattr(t, "draw") else None for t, (i, _) in zip(tts, srcs)]
    imgs = torch.full((4, 3, T, T), -7.0, device=DEV)
    labs = torch.full((4, T, T), -7, dtype=torch.int64, device=DEV)
    dev_srcs = [_dev(a, b) for a, b in srcs]
    for i, (t, d, (xi, xl)) in enumerate(zip(tts, draws, dev_srcs)):
        if i == 1:
            continue                                           # slot 1 stays untouched until the others are checked
        oi, ol = t(xi, xl, d, out_img=imgs[i], out_lab=labs[i])
        assert oi.data_ptr() == imgs[i].data_ptr() and ol.data_ptr() == labs[i].data_ptr()
    assert (imgs[1] == -7).all() and (labs[1] == -7).all()
    tts[1](*dev_srcs[1], draws[1], out_img=imgs[1], out_lab=labs[1])
    for i, (t, d, (xi, xl)) in enumerate(zip(tts, draws, dev_srcs)):
        wi, wl = t(xi, xl, d)
        assert torch.equal(imgs[i], wi) and torch.equal(labs[i], wl), i
    x0, y0 = draws[1].crop                                     # RandomCrop_p2 is the plain crop (flip, jitter, blur as drawn aside)
    if not draws[1].flip:
        assert np.array_equal(labs[1].cpu().numpy(), srcs[1][1][y0:y0 + T, x0:x0 + T].astype(np.int64))


def test_refuses_cpu_tensors_and_bad_slots():
    from mrfp_amd import _lib
    from mrfp_amd import input_pipeline as ip
    xi, xl = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV), torch.zeros(8, 8, dtype=torch.uint8, device=DEV)
    sc, fx = ip.ScaleCropTransform(8, 8), ip.FixScaleCropTransform(8)
    d = ip.ScaleCropDraw(False, None, None, (8, 8), (0, 0), (0, 0), None)
    for call in (lambda **kw: sc(kw.pop("img", xi), kw.pop("lab", xl), d, **kw), lambda **kw: fx(kw.pop("img", xi), kw.pop("lab", xl), **kw)):
        with pytest.raises(_lib.MrfpHipError):
            call(img=xi.cpu())
        with pytest.raises(_lib.MrfpHipError):
            call(lab=xl.long())
        with pytest.raises(_lib.MrfpHipError):
            call(lab=xl[:7])
        with pytest.raises(_lib.MrfpHipError, match="out_img"):
            call(out_img=torch.zeros(3, 8, 9, device=DEV))
        with pytest.raises(_lib.MrfpHipError, match="out_lab"):
            call(out_lab=torch.zeros(8, 8, dtype=torch.int32, device=DEV))
        with pytest.raises(_lib.MrfpHipError, match="out_img"):
            call(out_img=torch.zeros(3, 8, 8))
    with pytest.raises(_lib.MrfpHipError, match="ScaleCropTransform"):
        sc(xi, xl, ip.ScaleCropDraw(False, None, None, (8, 8), (0, 0), (1, 0), None))          # the crop leaves the image
    with pytest.raises(_lib.MrfpHipError):
        ip.rotate(xi.cpu(), xl, 5.0)
    with pytest.raises(_lib.MrfpHipError):
        ip.rotate(xi, xl.float(), 5.0)
    with pytest.raises(_lib.MrfpHipError):
        ip.contrast(xi.float())


def _mobilenet():
    import deepv3_common as dc
    from mrfp_amd import synth
    from mrfp_amd.config import cfg
    from mrfp_amd.network import deepv3
    cfg.MODEL.ACT_DTYPE = torch.float32
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    with contextlib.redirect_stdout(_io.StringIO()):
        m = deepv3.DeepMobileNetV3PlusD(None, 19, crit, crit)
    m.load_state_dict(synth.synth_state_dict(dc.spec("DeepMobileNetV3PlusD"), seed=0))
    return m.to(DEV)


def test_fix_scale_crop_batches_feed_evaluate():
    """harness.eval_batches with FixScaleCropTransform: the histogram equals the one from tensors the numpy restatement prepared."""
    import eval_input_common as eic
    from mrfp_amd import harness
    from mrfp_amd import input_pipeline as ip
    model = _mobilenet()
    enc = ip.label_encoder("CityscapesSegmentation")
    host = [eic.sample(224, 160, seed=s, ids=34) for s in (41, 42)]
    samples = [_dev(i, l) for i, l in host]
    tf = ip.FixScaleCropTransform(128, contrast=True, normalize=iac.IMAGENET)
    hist, miou, dropped = harness.evaluate(model, harness.eval_batches(samples, tf, enc))
    ref = []
    for i, l in host:
        a, b = iac.fix_scale_crop_transform_numpy(i, l, 128, True, iac.IMAGENET, enc.table)
        ref.append((torch.from_numpy(a)[None].to(DEV), torch.from_numpy(b)[None].to(DEV)))
    hist_r, miou_r, dropped_r = harness.evaluate(model, ref)
    assert dropped == dropped_r == 0 and hist.sum() > 0
    assert np.array_equal(hist, hist_r) and miou == miou_r
