"""The augmentation compositions against what PIL and numpy recorded in tests/golden/input_aug.npz (no Pillow and no reference
tree at test time): the numpy restatement of tests/input_aug_common.py everywhere, the device path on the GPU.  Images are
compared as bit patterns (Normalize leaves floats), labels as int64."""
import numpy as np
import pytest

import input_aug_common as iac

DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_fixture_sources_are_the_hashed_samples():
    G = iac.fixture()
    img, lab = iac.golden_source()
    assert np.array_equal(G["img"], img) and np.array_equal(G["lab"], lab) and img.shape == (30, 40, 3)
    for i, case in enumerate(iac.GOLDEN_EVAL):
        si, sl = iac.golden_source(case["w"], case["h"])
        assert np.array_equal(G["eval_src_img_%d" % i], si) and np.array_equal(G["eval_src_lab_%d" % i], sl)


@pytest.mark.parametrize("i", range(len(iac.GOLDEN_TRAIN)))
def test_scale_crop_restatement_equals_golden(i):
    G = iac.fixture()
    im, lb = iac.scale_crop_numpy(G["img"], G["lab"], crop_size=iac.GOLDEN_CROP, **iac.GOLDEN_TRAIN[i])
    assert np.array_equal(_bits(im), _bits(G["train_img_%d" % i])) and np.array_equal(lb, G["train_lab_%d" % i].astype(np.int64))


@pytest.mark.parametrize("i", range(len(iac.GOLDEN_EVAL)))
def test_fix_scale_crop_restatement_equals_golden(i):
    G = iac.fixture()
    case = iac.GOLDEN_EVAL[i]
    im, lb = iac.fix_scale_crop_transform_numpy(G["eval_src_img_%d" % i], G["eval_src_lab_%d" % i], iac.GOLDEN_CROP, case["contrast"],
                                                case["normalize"])
    assert np.array_equal(_bits(im), _bits(G["eval_img_%d" % i])) and np.array_equal(lb, G["eval_lab_%d" % i].astype(np.int64))


def test_golden_covers_the_paths():
    pads = [bool(c["pad"][0] or c["pad"][1]) for c in iac.GOLDEN_TRAIN]
    assert True in pads and False in pads
    assert any(c["degrees"] is not None and c["jitter"] for c in iac.GOLDEN_TRAIN)
    assert any(c["degrees"] is not None and c["blur"] is not None for c in iac.GOLDEN_TRAIN)
    assert any(c["degrees"] == 180.0 for c in iac.GOLDEN_TRAIN)
    assert sum(c["w"] > c["h"] and c["contrast"] and c["normalize"] is not None for c in iac.GOLDEN_EVAL) >= 1
    assert sum(c["h"] > c["w"] and c["contrast"] and c["normalize"] is not None for c in iac.GOLDEN_EVAL) >= 1


@pytest.mark.gpu
def test_device_equals_golden():
    import torch
    from mrfp_amd import input_pipeline as ip
    G = iac.fixture()
    xi, xl = torch.from_numpy(G["img"]).to(DEV), torch.from_numpy(G["lab"]).to(DEV)
    t = iac.GOLDEN_CROP
    for i, case in enumerate(iac.GOLDEN_TRAIN):
        tf = ip.ScaleCropTransform(t, t, fill=case.get("fill", 0), rotate_degree=None if case["degrees"] is None else 180,
                                   jitter=bool(case["jitter"]), contrast=case.get("contrast", False), normalize=case.get("normalize"))
        d = ip.ScaleCropDraw(case["flip"], case["jitter"], case["degrees"], case["scaled"], case["pad"], case["crop"], case["blur"])
        im, lb = tf(xi, xl, d)
        assert im.dtype == torch.float32 and lb.dtype == torch.int64 and tuple(im.shape) == (3, t, t)
        assert np.array_equal(_bits(im.cpu().numpy()), _bits(G["train_img_%d" % i])), i
        assert np.array_equal(lb.cpu().numpy(), G["train_lab_%d" % i].astype(np.int64)), i
    for i, case in enumerate(iac.GOLDEN_EVAL):
        si, sl = torch.from_numpy(G["eval_src_img_%d" % i]).to(DEV), torch.from_numpy(G["eval_src_lab_%d" % i]).to(DEV)
        im, lb = ip.FixScaleCropTransform(t, contrast=case["contrast"], normalize=case["normalize"])(si, sl)
        assert np.array_equal(_bits(im.cpu().numpy()), _bits(G["eval_img_%d" % i])), i
        assert np.array_equal(lb.cpu().numpy(), G["eval_lab_%d" % i].astype(np.int64)), i
