"""Focal and soft Dice / Jaccard criteria, what needs no GPU: the float64 restatements the GPU tests compare the kernels with
(region_loss_common) against F.cross_entropy and an independent numpy loop, the C header's new entries, the routing of the three
modules through loss.fused_ce_kwargs / fused_loss, and the argument refusals, raised before anything touches the library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import loss_common as lc
import region_loss_common as rc
from mrfp_amd import _lib, loss, ops

F64 = torch.float64


def _case(seed=3, B=2, C=3, H=4, W=5):
    x, y, yt, w, wb = rc.make_case(B, C, H, W, torch.float32, seed)
    return x.double(), y, yt, w.double(), wb.double()


@pytest.mark.parametrize("mode", rc.MODES)
@pytest.mark.parametrize("wform", ["none", "shared", "per_image"])
def test_focal_restatement_at_gamma_zero_is_the_cross_entropy(wform, mode):
    x, _, yt, w, wb = _case(B=3, C=5, H=6, W=7)
    wt = {"none": None, "shared": w, "per_image": wb}[wform]
    got = rc.ref_focal(x, yt, wt, 0.0, mode)
    want = lc.ref_loss(x, yt, wt, 0.0, mode)
    if wform != "per_image" and mode != "image_mean":
        assert want.item() == F.cross_entropy(x, yt, weight=wt, ignore_index=255, reduction=mode).item()
    assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item())


def test_focal_restatement_down_weights_easy_pixels():
    x, _, yt, w, _ = _case(B=2, C=5, H=6, W=7)
    lp = F.log_softmax(x, 1)
    total = 0.0
    for b, i, j in np.ndindex(*yt.shape):
        t = int(yt[b, i, j])
        if t != 255:
            pt = float(lp[b, t, i, j].exp())
            total += -float(w[t]) * (1.0 - pt) ** 2.0 * float(lp[b, t, i, j])
    assert abs(rc.ref_focal(x, yt, w, 2.0, "sum").item() - total) <= 1e-10 * abs(total)
    assert rc.ref_focal(x, yt, w, 2.0, "sum") < rc.ref_focal(x, yt, w, 0.5, "sum") < rc.ref_focal(x, yt, w, 0.0, "sum")


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("present_only", [True, False])
@pytest.mark.parametrize("kind", rc.KINDS)
def test_region_restatement_equals_the_numpy_loop(kind, present_only, per_image):
    x, y, yt, w, _ = _case()                       # 2 x 3 x 4 x 5
    for wt in (None, w):
        for smooth in (1.0, 1e-3):
            got = rc.ref_region(x, yt, wt, kind, smooth, present_only, per_image).item()
            want = rc.np_region(x, y, wt, kind, smooth, present_only, per_image)
            assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    sums = rc.ref_region(x, yt, want_sums=True, per_image=per_image)
    assert tuple(sums.shape) == (2 if per_image else 1, 3, 3)
    assert np.array_equal(sums[:, 2].sum(0).numpy(), np.bincount(yt[yt != 255].numpy(), minlength=3).astype(np.float64))


def test_an_all_ignored_batch_gives_zero():
    x, y, yt, w, _ = _case()
    blank = torch.full_like(yt, 255)
    xg = x.clone().requires_grad_(True)
    for kind in rc.KINDS:
        for per_image in (False, True):
            l = rc.ref_region(xg, blank, w, kind, 1.0, True, per_image)
            assert l.item() == 0.0 and rc.np_region(x, blank, w, kind, 1.0, True, per_image) == 0.0
            (g,) = torch.autograd.grad(l, xg)
            assert float(g.abs().max()) == 0.0
    # one blank image of two: per_image averages over the image that has a class
    half = yt.clone()
    half[1] = 255
    one = rc.ref_region(x[:1], yt[:1], w, "dice", 1.0, True, True).item()
    assert abs(rc.ref_region(x, half, w, "dice", 1.0, True, True).item() - one) <= 1e-15


NEW_ENTRIES = ["mrfp_focal_fwd", "mrfp_focal_bwd", "mrfp_upsample_focal_fwd", "mrfp_upsample_focal_bwd", "mrfp_region_nblocks",
               "mrfp_region_ws_floats", "mrfp_region_out_floats", "mrfp_region_fwd", "mrfp_region_bwd", "mrfp_upsample_region_fwd",
               "mrfp_upsample_region_bwd"]


def test_header_declares_the_new_entries():
    protos = _lib.parse_header()
    for n in NEW_ENTRIES:
        assert n in protos and len(protos[n][1]) == len(_lib.ARG_NAMES[n]), n
    names = _lib.ARG_NAMES
    # the ce_w argument lists with gamma where they have smoothing
    for tail in ("fwd", "bwd"):
        for pre in ("mrfp_", "mrfp_upsample_"):
            assert names[pre + "focal_" + tail] == [("gamma" if a == "smoothing" else a) for a in names[pre + "ce_w_" + tail]]
    # the fused forms add the score geometry to the dense ones, as every loss entry does
    for tail in ("fwd", "bwd"):
        dense, fused = names["mrfp_region_" + tail], names["mrfp_upsample_region_" + tail]
        assert dense[0] == "logits" and fused[:2] == ["P", "ld"] and dense[-1] == fused[-1] == "stream"
        assert set(dense) - set(fused) == {"logits", "HW"} and set(fused) - set(dense) >= {"P", "ld", "Hi", "Wi", "H", "W"}
    assert names["mrfp_region_nblocks"] == ["B", "HW"] and names["mrfp_region_out_floats"] == ["B", "C", "per_image"]
    assert "MRFP_REGION_DICE = 0" in open(_lib.HEADER).read() and ops.REGION_KINDS == {"dice": 0, "jaccard": 1}


class _Foreign(nn.Module):
    def forward(self, x, y):
        return x.sum()


def test_routing_of_the_three_modules(monkeypatch):
    assert {"FocalLoss2d", "RegionLoss2d", "SumLoss"} <= set(loss.__all__)
    focal = loss.FocalLoss2d(gamma=1.5, weight=[0.5] * 19, ignore_index=7, reduction="sum")
    region = loss.RegionLoss2d("jaccard", smooth=0.5, present_only=False, weight=[2.0] * 19, ignore_index=7, per_image=True)
    ce = nn.CrossEntropyLoss(ignore_index=7)
    both = loss.SumLoss((1.0, ce), (0.5, region))
    assert list(loss.fused_ce_kwargs(focal)) == ["focal"] and list(loss.fused_ce_kwargs(region)) == ["region"]
    assert list(loss.fused_ce_kwargs(both)) == ["sum"]
    # weights are buffers that stay out of the state dict
    for m in (focal, region):
        assert "weight" in dict(m.named_buffers()) and not m.state_dict()
    # what stays on the stock call
    assert loss.fused_ce_kwargs(_Foreign()) is None and loss.fused_ce_kwargs(nn.CrossEntropyLoss(reduction="none")) is None
    assert loss.fused_ce_kwargs(loss.FocalLoss2d(reduction="none")) is None
    for part in (_Foreign(), nn.CrossEntropyLoss(reduction="none"), loss.FocalLoss2d(reduction="none")):
        s = loss.SumLoss((1.0, ce), (0.5, part))
        assert loss.fused_ce_kwargs(s) is None and loss.fused_loss(s, "x", "y") is None and s.fused("x", "y") is None
    nested = loss.SumLoss((1.0, loss.SumLoss((1.0, ce), (2.0, _Foreign()))), (0.5, region))
    assert loss.fused_ce_kwargs(nested) is None

    # the operators each module reaches, and with which arguments
    seen = []

    def op(name, value):
        def f(*a, **k):
            seen.append((name, a, k))
            return value
        return f
    for name, value in (("focal_loss", 2.0), ("upsample_focal_loss", 3.0), ("region_loss", 5.0), ("upsample_region_loss", 7.0),
                        ("cross_entropy", 11.0), ("upsample_cross_entropy", 13.0)):
        monkeypatch.setattr(ops, name, op(name, value))
    assert loss.fused_loss(focal, "x", "y") == 2.0 and loss.fused_loss(focal, "P", "y", (8, 8), 19) == 3.0
    (n1, a1, k1), (n2, a2, k2) = seen
    assert (n1, a1) == ("focal_loss", ("x", "y", 7)) and (n2, a2) == ("upsample_focal_loss", ("P", "y", (8, 8), 19, 7))
    assert k1 == k2 and k1["gamma"] == 1.5 and k1["reduction"] == "sum" and k1["weight"] is focal.weight
    del seen[:]
    assert loss.fused_loss(region, "x", "y") == 5.0 and loss.fused_loss(region, "P", "y", (8, 8), 19) == 7.0 and region("x", "y") == 5.0
    assert seen[0][:2] == ("region_loss", ("x", "y", 7)) and seen[1][:2] == ("upsample_region_loss", ("P", "y", (8, 8), 19, 7))
    assert seen[0][2] == dict(kind="jaccard", smooth=0.5, present_only=False, weight=region.weight, per_image=True)
    del seen[:]
    assert loss.fused_loss(both, "x", "y") == 1.0 * 11.0 + 0.5 * 5.0 and both("x", "y") == 13.5
    assert loss.fused_loss(both, "P", "y", (8, 8), 19) == 1.0 * 13.0 + 0.5 * 7.0
    # an unfused sum is the sum of its parts' own forwards
    assert loss.SumLoss((2.0, _Foreign()), (0.5, region))(torch.ones(2, 2), "y").item() == 2.0 * 4.0 + 0.5 * 5.0


def test_refusals_come_before_the_library(monkeypatch):
    def no_lib():
        raise AssertionError("an argument refusal touched the library")
    monkeypatch.setattr(_lib, "lib", no_lib)
    E = _lib.MrfpHipError
    x = torch.zeros(2, 5, 3, 4)
    y = torch.zeros(2, 3, 4, dtype=torch.int64)
    for bad in (-0.5, float("nan"), float("inf"), "two"):
        with pytest.raises(E, match="focal_loss: gamma"):
            ops.focal_loss(x, y, gamma=bad)
        with pytest.raises(E, match="upsample_focal_loss: gamma"):
            ops.upsample_focal_loss(x, y, (6, 8), 5, gamma=bad)
        with pytest.raises(E, match="FocalLoss2d: gamma"):
            loss.FocalLoss2d(gamma=bad)
    with pytest.raises(E, match="region_loss: present_only=False needs smooth > 0"):
        ops.region_loss(x, y, present_only=False, smooth=0.0)
    with pytest.raises(E, match="upsample_region_loss: smooth"):
        ops.upsample_region_loss(x, y, (6, 8), 5, smooth=-1.0)
    with pytest.raises(E, match="RegionLoss2d: present_only=False needs smooth > 0"):
        loss.RegionLoss2d(present_only=False, smooth=0)
    with pytest.raises(E, match="region_loss: kind"):
        ops.region_loss(x, y, kind="lovasz")
    assert loss.RegionLoss2d(smooth=0.0).smooth == 0.0               # fine with present_only

    # what depends on the tensors: the criterion records' check, on CPU tensors here (the operators refuse those at their door)
    src = ops._Scores(x)
    focal = ops._Focal("focal_loss", 255, 2.0, "mean", False)
    region = ops._Region("region_loss", 255)
    for crit, shapes in ((focal, [(4,), (3, 5), (2, 5, 1)]), (region, [(4,), (2, 5)])):
        for shape in shapes:
            with pytest.raises(E, match=crit.who + ": weight must be a float32 tensor"):
                crit.check(src, y, torch.ones(shape))
        with pytest.raises(E, match=crit.who + ": weight must be a float32 tensor"):
            crit.check(src, y, torch.ones(5, dtype=F64))
        with pytest.raises(E, match=crit.who + ": weight must be a float32 tensor"):
            crit.check(src, y, torch.ones(5, device="meta"))
        with pytest.raises(E, match=crit.who + ": target must be int64"):
            crit.check(src, y.int(), None)
        t, w = crit.check(src, y, torch.ones(5))
        assert t.dtype == torch.int64 and tuple(w.shape) == (5,)
    wide = ops._Scores(torch.zeros(1, 65, 2, 2))
    y1 = torch.zeros(1, 2, 2, dtype=torch.int64)
    with pytest.raises(E, match="focal_loss: 1 <= C <= 64"):
        focal.check(wide, y1, None)
    with pytest.raises(E, match="region_loss: 1 <= C <= 64"):
        region.check(wide, y1, None)
    with pytest.raises(E, match="region_sums: 1 <= C <= 64"):
        ops._Region("region_sums", 255).check(ops._Scores(torch.zeros(1, 72, 2, 2), (4, 4), 65), torch.zeros(1, 4, 4, dtype=torch.int64), None)
    with pytest.raises(E, match="focal_loss: reduction must be 'mean' or 'sum'"):
        ops._Focal("focal_loss", 255, 2.0, "none", False).check(src, y, None)
    # and the operators' door
    with pytest.raises(E, match="must live on the GPU"):
        ops.region_loss(x, y)
