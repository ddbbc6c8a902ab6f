"""The Resize and Crop training compositions on the GPU (mrfp_amd/input_pipeline.py::ResizeTransform / CropTransform) against
the reference's PIL calls: byte-exact with the recorded outputs (tests/golden/input_resize.npz) and with live PIL when Pillow
is present; a batch filled per sample through out_img / out_lab, mixing TrainTransform and ResizeTransform samples."""
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _mg():
    sys.path.insert(0, GDIR)
    import make_golden_input_resize as mg
    return mg


def _draw(d, **kw):
    from mrfp_amd.input_pipeline import Draw
    return Draw(d["flip"], d["jitter"], kw.get("scaled", (0, 0)), (0, 0), kw.get("crop", (0, 0)), d["blur"])


def test_resize_and_crop_equal_golden_pil_outputs():
    from mrfp_amd.input_pipeline import CropTransform, ResizeTransform
    mg = _mg()
    G = np.load(os.path.join(GDIR, "input_resize.npz"))
    xi, xl = torch.from_numpy(G["img"]).to(DEV), torch.from_numpy(G["lab"]).to(DEV)
    H, W = G["lab"].shape
    for i, d in enumerate(mg.RESIZE):
        t = ResizeTransform(*d["size"])
        im, lb = t(xi, xl, _draw(d, scaled=d["size"]))
        assert im.shape == (3, d["size"][1], d["size"][0]) and lb.dtype == torch.int64
        assert np.array_equal(im.cpu().numpy(), G["resize_img_%d" % i].astype(np.float32)), i
        assert np.array_equal(lb.cpu().numpy(), G["resize_lab_%d" % i].astype(np.int64)), i
    t = CropTransform(*mg.CROP_SIZE)
    for i, d in enumerate(mg.CROP):
        im, lb = t(xi, xl, _draw(d, scaled=(W, H), crop=d["crop"]))
        assert im.shape == (3, mg.CROP_SIZE[0], mg.CROP_SIZE[1])
        assert np.array_equal(im.cpu().numpy(), G["crop_img_%d" % i].astype(np.float32)), i
        assert np.array_equal(lb.cpu().numpy(), G["crop_lab_%d" % i].astype(np.int64)), i


@pytest.mark.parametrize("H,W,size1,size2", [(96, 128, 80, 60), (60, 90, 160, 120), (75, 75, 75, 75), (128, 256, 256, 96)])
def test_resize_transform_equals_pil(H, W, size1, size2):
    Image = pytest.importorskip("PIL.Image")
    from mrfp_amd.input_pipeline import ResizeTransform
    mg = _mg()
    rng = np.random.default_rng(H + W + size1)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    lab = rng.integers(0, 19, (H, W), dtype=np.uint8)
    t = ResizeTransform(size1, size2)
    r, nr = random.Random(9), np.random.RandomState(9)
    draws = [t.draw(W, H, r, nr) for _ in range(12)]
    assert any(d.jitter for d in draws) and any(d.blur is not None for d in draws) and any(d.flip for d in draws)
    xi, xl = torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)
    for d in draws:
        want_im, want_lab = mg.resize_pil(Image.fromarray(img), Image.fromarray(lab), size=(size1, size2), flip=d.flip,
                                          jitter=d.jitter, blur=d.blur)
        got_im, got_lab = t(xi, xl, d)
        assert np.array_equal(got_im.cpu().numpy(), want_im), d
        assert np.array_equal(got_lab.cpu().numpy(), want_lab.astype(np.int64)), d


@pytest.mark.parametrize("H,W,base,crop", [(96, 128, 64, 96), (60, 90, 60, 90), (200, 150, 48, 32)])
def test_crop_transform_equals_pil(H, W, base, crop):
    Image = pytest.importorskip("PIL.Image")
    from mrfp_amd.input_pipeline import CropTransform
    mg = _mg()
    rng = np.random.default_rng(H * W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    lab = rng.integers(0, 19, (H, W), dtype=np.uint8)
    t = CropTransform(base, crop)
    r, nr = random.Random(4), np.random.RandomState(4)
    draws = [t.draw(W, H, r, nr) for _ in range(12)]
    xi, xl = torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)
    for d in draws:
        want_im, want_lab = mg.crop_pil(Image.fromarray(img), Image.fromarray(lab), base_size=base, crop_size=crop, crop=d.crop,
                                        flip=d.flip, jitter=d.jitter, blur=d.blur)
        got_im, got_lab = t(xi, xl, d)
        assert np.array_equal(got_im.cpu().numpy(), want_im), d
        assert np.array_equal(got_lab.cpu().numpy(), want_lab.astype(np.int64)), d


def test_mixed_batch_through_out_slots():
    """GTAV + Synthia (main.py:821 ConcatDataset): one batch holds TrainTransform and ResizeTransform samples, each written into
    its slot of the batch tensors; equal to the per-sample results."""
    from mrfp_amd.input_pipeline import ResizeTransform, TrainTransform
    T = 64
    rng = np.random.default_rng(0)
    srcs = [(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 19, (h, w), dtype=np.uint8))
            for h, w in [(96, 128), (80, 100), (96, 128), (70, 50)]]
    tts = [TrainTransform(T), ResizeTransform(T, T), TrainTransform(T), ResizeTransform(T, T)]
    r, nr = random.Random(1), np.random.RandomState(1)
    draws = [t.draw(img.shape[1], img.shape[0], r, nr) for t, (img, _) in zip(tts, srcs)]
    imgs = torch.full((4, 3, T, T), -1.0, device=DEV)
    labs = torch.full((4, T, T), -1, dtype=torch.int64, device=DEV)
    dev_srcs = [(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)) for a, b in srcs]
    for i, (t, d, (xi, xl)) in enumerate(zip(tts, draws, dev_srcs)):
        oi, ol = t(xi, xl, d, out_img=imgs[i], out_lab=labs[i])
        assert oi.data_ptr() == imgs[i].data_ptr() and ol.data_ptr() == labs[i].data_ptr()
    for i, (t, d, (xi, xl)) in enumerate(zip(tts, draws, dev_srcs)):
        wi, wl = t(xi, xl, d)
        assert torch.equal(imgs[i], wi) and torch.equal(labs[i], wl), i


def test_refuses_cpu_tensors_and_bad_slots():
    from mrfp_amd import _lib
    from mrfp_amd.input_pipeline import CropTransform, Draw, ResizeTransform
    d = Draw(False, None, (8, 8), (0, 0), (0, 0), None)
    for t in (ResizeTransform(8, 8), CropTransform(8, 8)):
        with pytest.raises(_lib.MrfpHipError):
            t(torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(8, 8, dtype=torch.uint8), d)
        xi, xl = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV), torch.zeros(8, 8, dtype=torch.uint8, device=DEV)
        with pytest.raises(_lib.MrfpHipError):
            t(xi, xl, d, out_img=torch.zeros(3, 8, 9, device=DEV))
    with pytest.raises(_lib.MrfpHipError):
        CropTransform(8, 8)(torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV), torch.zeros(8, 8, dtype=torch.uint8, device=DEV),
                            Draw(False, None, (8, 8), (0, 0), (1, 0), None))
