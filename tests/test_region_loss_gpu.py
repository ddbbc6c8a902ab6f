"""Focal and soft Dice / Jaccard losses on the GPU (csrc/loss.hip: Focal; csrc/region.hip) against the float64 torch restatements
of region_loss_common on the CPU, dense logits and the fused source (referenced as F.interpolate(P[:, :C].double(), size,
mode="bilinear", align_corners=True)), and the criteria on a model.

Bounds: the project's own for this kernel family (test_loss_gpu.LOSS_TOL / GRAD_TOL) -- loss relative 1e-5 (fp32) / 2e-3 (16-bit),
gradient 2e-5 / 1.5e-2 of the tensor maximum.  Inputs are rounded to the activation dtype first.

Shapes: C in {2, 19, 24, 25, 64} (two class-pad boundaries and the maximum); dense 5 x 7 (less than one wave) and 33 x 65 (several
workgroups per image and a tail); fused 5 x 7 -> 17 x 25 and 1 x 9 -> 6 x 33 with the score pitch equal to and larger than C rounded
to a chunk; B = 3 with one image entirely ignored; one capped-grid case where a workgroup walks its image more than once."""
import contextlib
import functools
import io
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import loss_common as lc
import region_loss_common as rc
from mrfp_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
LOSS_TOL = {F32: 1e-5, BF16: 2e-3, F16: 2e-3}
GRAD_TOL = {F32: 2e-5, BF16: 1.5e-2, F16: 1.5e-2}
CLASSES = [2, 19, 24, 25, 64]
DENSE = [(5, 7), (33, 65)]
FUSED = [((5, 7), (17, 25)), ((1, 9), (6, 33))]
WFORMS = ("none", "shared", "per_image")


def dname(d):
    return str(d).replace("torch.", "")


def ops():
    from mrfp_amd import ops as o
    return o


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


def bwd_scale(dtype, summed=False):
    """0.7, or the 4096 loss scale of the float16 tests (1/#pixels gradients survive float16); `sum` gradients are O(1)."""
    return 4096.0 if dtype == F16 and not summed else 0.7


def chunk(dtype):
    return 16 // torch.empty((), dtype=dtype).element_size()


def on_device(x, dtype, ld=None):
    """Dense logits (ld None) or scores zero-padded to pitch ld, channels-last on the device, requiring a gradient."""
    if ld is not None:
        P = torch.zeros(x.shape[0], ld, x.shape[2], x.shape[3])
        P[:, :x.shape[1]] = x
        x = P
    return x.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)


def pitches(C, dtype):
    e = chunk(dtype)
    cr = (C + e - 1) // e * e
    return [cr, cr + 2 * e]


def upsampled(xc, size):
    return F.interpolate(xc, size, mode="bilinear", align_corners=True)


def check(ld, gd, lref, gref, dtype, what):
    le = abs(ld.item() - lref.item()) / abs(lref.item())
    ge = relerr(gd, gref)
    print("%s: loss relerr %.3g gradient relerr %.3g" % (what, le, ge))
    assert le < LOSS_TOL[dtype] and ge < GRAD_TOL[dtype], (what, le, ge)


def weight_of(form, w, wb):
    return {"none": None, "shared": w, "per_image": wb}[form]


def focal_kwargs(gamma, wt, mode):
    return dict(gamma=gamma, weight=None if wt is None else wt.to(DEV), reduction="sum" if mode == "sum" else "mean",
                per_image=mode == "image_mean")


def run_focal(x, y, yt, w, wb, dtype, size, ld, combos, what):
    """Every (gamma, weight form, mode) of `combos` on one input: kernels against the float64 restatement (of the upsampled scores
    with `size`)."""
    C = x.shape[1]
    for gamma, form, mode in combos:
        wt = weight_of(form, w, wb)
        s = bwd_scale(dtype, mode == "sum")
        xc = x.double().requires_grad_(True)
        lref = rc.ref_focal(xc if size is None else upsampled(xc, size), yt, None if wt is None else wt.double(), gamma, mode)
        (lref * s).backward()
        xd = on_device(x, dtype, ld)
        if size is None:
            l = ops().focal_loss(xd, y.to(DEV), 255, **focal_kwargs(gamma, wt, mode))
        else:
            l = ops().upsample_focal_loss(xd, y.to(DEV), size, C, 255, **focal_kwargs(gamma, wt, mode))
        (l * s).backward()
        assert l.dtype == F32 and xd.grad.dtype == dtype
        check(l, xd.grad[:, :C], lref, xc.grad, dtype, "%s gamma=%g %s %s" % (what, gamma, form, mode))
        assert float(xd.grad[:, C:].abs().max() if xd.shape[1] > C else 0.0) == 0.0


def latin(gammas=rc.GAMMAS):
    """Every gamma with every weight form and with every mode; every (weight form, mode) pair over the gammas."""
    return [(g, WFORMS[(i + k) % 3], rc.MODES[(2 * i + k) % 3]) for i, g in enumerate(gammas) for k in range(3)]


REGION_COMBOS = [(kind, present, per_image, smooth, (i + j + k) % 2 == 0)
                 for i, kind in enumerate(rc.KINDS) for j, present in enumerate((True, False)) for k, per_image in enumerate((False, True))
                 for smooth in (1.0, 1e-3)]


def run_region(x, y, yt, w, dtype, size, ld, what, combos=REGION_COMBOS):
    C = x.shape[1]
    for kind, present, per_image, smooth, weighted in combos:
        wt = w if weighted else None
        s = bwd_scale(dtype)
        xc = x.double().requires_grad_(True)
        lref = rc.ref_region(xc if size is None else upsampled(xc, size), yt, None if wt is None else wt.double(), kind, smooth,
                             present, per_image)
        (lref * s).backward()
        xd = on_device(x, dtype, ld)
        kw = dict(kind=kind, smooth=smooth, present_only=present, per_image=per_image, weight=None if wt is None else wt.to(DEV))
        if size is None:
            l = ops().region_loss(xd, y.to(DEV), 255, **kw)
        else:
            l = ops().upsample_region_loss(xd, y.to(DEV), size, C, 255, **kw)
        (l * s).backward()
        assert l.dtype == F32 and xd.grad.dtype == dtype
        check(l, xd.grad[:, :C], lref, xc.grad, dtype, "%s %s present_only=%s per_image=%s s=%g weighted=%s" % (
            what, kind, present, per_image, smooth, weighted))
        assert float(xd.grad[:, C:].abs().max() if xd.shape[1] > C else 0.0) == 0.0


# ---- focal ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("hw", DENSE, ids=str)
@pytest.mark.parametrize("C", CLASSES)
def test_dense_focal(C, hw, dtype):
    x, y, yt, w, wb = rc.make_case(2, C, hw[0], hw[1], dtype, 1000 + C + hw[0])
    run_focal(x, y, yt, w, wb, dtype, None, None, latin(), "dense focal C=%d %s %s" % (C, hw, dname(dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("case", FUSED, ids=str)
@pytest.mark.parametrize("C", CLASSES)
def test_fused_focal(C, case, dtype):
    low, size = case
    x, y, yt, w, wb = rc.make_case(2, C, size[0], size[1], dtype, 2000 + C + size[0], scale=2.0, low=low)
    for k, ld in enumerate(pitches(C, dtype)):
        run_focal(x, y, yt, w, wb, dtype, size, ld, latin()[k::2], "fused focal C=%d %s ld=%d %s" % (C, case, ld, dname(dtype)))


def test_focal_every_gamma_weight_form_and_mode():
    """The full cross product on one small case (19 classes, fp32, dense 5 x 7 and fused 5 x 7 -> 17 x 25)."""
    combos = [(g, f, m) for g in rc.GAMMAS for f in WFORMS for m in rc.MODES]
    x, y, yt, w, wb = rc.make_case(2, 19, 5, 7, F32, 77)
    run_focal(x, y, yt, w, wb, F32, None, None, combos, "dense focal full")
    x, y, yt, w, wb = rc.make_case(2, 19, 17, 25, F32, 78, scale=2.0, low=(5, 7))
    run_focal(x, y, yt, w, wb, F32, (17, 25), 20, combos, "fused focal full")


def ulp_at(v, dtype):
    """One rounding step of dtype at the magnitude v."""
    mant = {BF16: 7, F16: 10}[dtype]
    return 2.0 ** (math.floor(math.log2(v)) - mant)


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
@pytest.mark.parametrize("C", [2, 19, 64])
def test_gamma_zero_is_the_weighted_cross_entropy(C, fused, dtype):
    """gamma = 0: the loss equals ops.cross_entropy(..., weight=w, _general=True) bit for bit; the gradient agrees within 1e-6 of the
    tensor maximum (fp32), within one rounding step of the activation dtype at the tensor maximum (bf16 / fp16)."""
    size, low = ((17, 25), (5, 7)) if fused else ((33, 65), None)
    x, y, _, w, wb = rc.make_case(2, C, size[0], size[1], dtype, 3000 + C, low=low)
    yd = y.to(DEV)
    for form in WFORMS:
        for mode in rc.MODES:
            wt = weight_of(form, w, wb)
            kw = focal_kwargs(0.0, wt, mode)
            ckw = dict(weight=kw["weight"], reduction=kw["reduction"], per_image=kw["per_image"], _general=True)
            s = bwd_scale(dtype, mode == "sum")
            a, b = on_device(x, dtype, 72 if fused else None), on_device(x, dtype, 72 if fused else None)
            if fused:
                lf = ops().upsample_focal_loss(a, yd, size, C, 255, **kw)
                lc_ = ops().upsample_cross_entropy(b, yd, size, C, 255, **ckw)
            else:
                lf = ops().focal_loss(a, yd, 255, **kw)
                lc_ = ops().cross_entropy(b, yd, 255, **ckw)
            (lf * s).backward()
            (lc_ * s).backward()
            assert torch.equal(lf.view(torch.int32), lc_.view(torch.int32)), (form, mode, lf.item(), lc_.item())
            gmax = float(b.grad.abs().max())
            diff = float((a.grad.double() - b.grad.double()).abs().max())
            bound = 1e-6 * gmax if dtype == F32 else ulp_at(gmax, dtype)
            print("gamma 0 %s %s: gradient difference %.3g, bound %.3g" % (form, mode, diff, bound))
            assert diff <= bound, (form, mode, diff, bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_extreme_logits_give_finite_gradients(dtype):
    """Logits of +-80: pixels whose true class has +80 and every other -80 (p_t rounds to 1: loss 0, gradient exactly 0, for every
    gamma, 0.5 < 1 among them) and pixels whose true class has -80 and another +80 (confident and wrong: finite loss and gradient)."""
    B, C, H, W = 2, 19, 9, 11
    g = torch.Generator().manual_seed(5)
    y = torch.randint(0, C, (B, H, W), generator=g)
    right = torch.rand(B, H, W, generator=g) < 0.5
    hot = torch.where(right, y, (y + 1 + torch.randint(0, C - 1, (B, H, W), generator=g)) % C)
    x = torch.full((B, C, H, W), -80.0).scatter_(1, hot[:, None], 80.0)
    for gamma in rc.GAMMAS:
        xd = on_device(x, dtype)
        l = ops().focal_loss(xd, y.to(DEV), 255, gamma=gamma, reduction="sum")
        l.backward()
        grad = xd.grad.float().cpu()
        assert math.isfinite(l.item()) and bool(torch.isfinite(grad).all()), gamma
        assert float(grad.permute(0, 2, 3, 1)[right].abs().max()) == 0.0, gamma
        assert float(grad.permute(0, 2, 3, 1)[~right].abs().max()) > 0.0, gamma
        want = 160.0 * int((~right).sum())            # -log p_t = 160, (1 - p_t)^gamma = 1 at each wrong pixel
        assert abs(l.item() - want) <= 1e-5 * want, (gamma, l.item(), want)
    for kind in rc.KINDS:
        xd = on_device(x, dtype)
        l = ops().region_loss(xd, y.to(DEV), 255, kind=kind)
        (l * bwd_scale(dtype)).backward()
        assert math.isfinite(l.item()) and bool(torch.isfinite(xd.grad.float()).all()), kind


# ---- region ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("hw", DENSE, ids=str)
@pytest.mark.parametrize("C", CLASSES)
def test_dense_region(C, hw, dtype):
    x, y, yt, w, _ = rc.make_case(2, C, hw[0], hw[1], dtype, 4000 + C + hw[0])
    run_region(x, y, yt, w, dtype, None, None, "dense region C=%d %s %s" % (C, hw, dname(dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("case", FUSED, ids=str)
@pytest.mark.parametrize("C", CLASSES)
def test_fused_region(C, case, dtype):
    low, size = case
    x, y, yt, w, _ = rc.make_case(2, C, size[0], size[1], dtype, 5000 + C + size[0], scale=2.0, low=low)
    for k, ld in enumerate(pitches(C, dtype)):
        run_region(x, y, yt, w, dtype, size, ld, "fused region C=%d %s ld=%d %s" % (C, case, ld, dname(dtype)), REGION_COMBOS[k::2])


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
def test_one_image_entirely_ignored(fused, dtype):
    """B = 3, image 1 all 255, class C-1 absent, labels -1 and C present: the region loss per image averages over the two images that
    have a class, and image 1's gradient is exactly 0; the focal sums skip it."""
    C = 19
    size, low = ((17, 25), (5, 7)) if fused else ((33, 65), None)
    x, y, yt, w, wb = rc.make_case(3, C, size[0], size[1], dtype, 6000, scale=2.0, low=low, blank_image=1)
    assert int((y == -1).sum()) > 0 and int((y == C).sum()) > 0 and int((y == C - 1).sum()) == 0
    ld = 24 if fused else None
    sz = size if fused else None
    run_region(x, y, yt, w, dtype, sz, ld, "blank image region %s" % dname(dtype))
    run_focal(x, y, yt, w, wb, dtype, sz, ld, [(g, f, m) for g, f, m in latin() if m != "image_mean"], "blank image focal %s" % dname(dtype))
    if not fused:
        xd = on_device(x, dtype)
        ops().region_loss(xd, y.to(DEV), 255, per_image=True).backward()
        assert float(xd.grad[1].abs().max()) == 0.0 and float(xd.grad[0].abs().max()) > 0.0


@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
def test_all_ignored_gives_zero_loss_and_gradient(fused):
    C = 19
    x = torch.randn(2, C, 5, 7)
    size = (17, 25) if fused else (5, 7)
    y = torch.full((2,) + size, 255, dtype=torch.int64)
    y[0, 0, 0], y[1, 2, 3] = -1, C
    for kind in rc.KINDS:
        for per_image in (False, True):
            for present in (True, False):
                xd = on_device(x, BF16, 24 if fused else None)
                kw = dict(kind=kind, per_image=per_image, present_only=present)
                l = ops().upsample_region_loss(xd, y.to(DEV), size, C, 255, **kw) if fused else ops().region_loss(xd, y.to(DEV), 255, **kw)
                l.backward()
                if present:
                    assert l.item() == 0.0 and float(xd.grad.abs().max()) == 0.0, (kind, per_image)
                else:          # every class counts, S_c = s / s = 1: the loss is 0 here as well
                    assert abs(l.item()) < 1e-6 and float(xd.grad.abs().max()) == 0.0, (kind, per_image)
    xd = on_device(x, BF16, 24 if fused else None)
    l = ops().upsample_focal_loss(xd, y.to(DEV), size, C, 255, reduction="sum") if fused else ops().focal_loss(xd, y.to(DEV), 255, reduction="sum")
    l.backward()
    assert l.item() == 0.0 and float(xd.grad.abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
@pytest.mark.parametrize("C", CLASSES)
def test_region_sums(C, fused, dtype):
    """T exactly np.bincount; I and P within the loss bound of the float64 sums."""
    size, low = ((17, 25), (5, 7)) if fused else ((33, 65), None)
    x, y, yt, _, _ = rc.make_case(3, C, size[0], size[1], dtype, 7000 + C, scale=2.0, low=low, blank_image=2)
    xd = on_device(x, dtype, pitches(C, dtype)[1] if fused else None).detach()
    for per_image in (False, True):
        kw = dict(size=size, channels=C) if fused else {}
        got = ops().region_sums(xd, y.to(DEV), 255, per_image=per_image, **kw)
        assert got.dtype == torch.float64 and tuple(got.shape) == (3 if per_image else 1, 3, C)
        got = got.cpu()
        xr = x.double()
        ref = rc.ref_region(upsampled(xr, size) if fused else xr, yt, want_sums=True, per_image=per_image)
        groups = [yt[b] for b in range(3)] if per_image else [yt]
        for r, lab in enumerate(groups):
            assert np.array_equal(got[r, 2].numpy(), np.bincount(lab[lab != 255].numpy().ravel(), minlength=C).astype(np.float64))
        for q in (0, 1):
            err = ((got[:, q] - ref[:, q]).abs().max() / ref[:, q].abs().max()).item()
            assert err < LOSS_TOL[dtype], (q, err)


# ---- the capped grid: B = 64, 96 x 96, C = 3 -- ce_w_blocks_x gives 32 workgroups per image = 8 192 threads < 9 216 pixels ------------
CAP_B, CAP_S, CAP_C = 64, 96, 3


@functools.lru_cache(maxsize=None)
def capped_case(fused):
    """Inputs and float64 references (loss, gradient) of the capped-grid case, computed once and not modified."""
    low = (24, 24) if fused else None
    x, y, yt, w, wb = rc.make_case(CAP_B, CAP_C, CAP_S, CAP_S, BF16, 8000, scale=2.0, low=low)
    ref = {}
    for name, f in (("focal", lambda z: rc.ref_focal(z, yt, wb.double(), 2.0, "image_mean")),
                    ("dice", lambda z: rc.ref_region(z, yt, w.double(), "dice", 1.0, True, False)),
                    ("jaccard_per_image", lambda z: rc.ref_region(z, yt, None, "jaccard", 1e-3, True, True))):
        xc = x.double().requires_grad_(True)
        l = f(upsampled(xc, (CAP_S, CAP_S)) if fused else xc)
        l.backward()
        ref[name] = (l.detach(), xc.grad)
    return x, y, w, wb, ref


@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
def test_capped_grid_and_two_runs(fused):
    """A workgroup walks its image more than once; and two runs of every operator are bit-identical."""
    from mrfp_amd import _lib
    assert _lib.lib().mrfp_region_nblocks(CAP_B, CAP_S * CAP_S) == 32 * CAP_B and 32 * 256 < CAP_S * CAP_S
    x, y, w, wb, ref = capped_case(fused)
    yd, size = y.to(DEV), (CAP_S, CAP_S)

    def run(name):
        xd = on_device(x, BF16, 8 if fused else None)
        head = (xd, yd, size, CAP_C, 255) if fused else (xd, yd, 255)
        o = ops()
        if name == "focal":
            l = (o.upsample_focal_loss if fused else o.focal_loss)(*head, gamma=2.0, weight=wb.to(DEV), per_image=True)
        elif name == "dice":
            l = (o.upsample_region_loss if fused else o.region_loss)(*head, weight=w.to(DEV))
        else:
            l = (o.upsample_region_loss if fused else o.region_loss)(*head, kind="jaccard", smooth=1e-3, per_image=True)
        l.backward()
        return l.detach(), xd.grad[:, :CAP_C]
    for name in ("focal", "dice", "jaccard_per_image"):
        l1, g1 = run(name)
        l2, g2 = run(name)
        assert torch.equal(l1, l2) and torch.equal(g1, g2), name
        check(l1, g1, ref[name][0], ref[name][1], BF16, "capped %s %s" % ("fused" if fused else "dense", name))


# ---- the modules ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
def test_sum_loss_is_the_weighted_sum_of_its_parts(fused):
    from mrfp_amd import loss as L
    C = 19
    size, low = ((17, 25), (5, 7)) if fused else ((33, 65), None)
    x, y, yt, w, _ = rc.make_case(2, C, size[0], size[1], BF16, 9000, low=low)
    ce, dice = nn.CrossEntropyLoss(weight=w, ignore_index=255).to(DEV), L.RegionLoss2d(weight=w).to(DEV)
    both = L.SumLoss((1.0, ce), (0.5, dice)).to(DEV)
    assert dice.weight.device.type == "cuda"
    tail = (size, C) if fused else ()

    def run(f):
        xd = on_device(x, BF16, 24 if fused else None)
        l = f(xd)
        l.backward()
        return l.detach(), xd.grad
    ls, gs = run(lambda xd: both.fused(xd, y.to(DEV), *tail))
    lp, gp = run(lambda xd: 1.0 * L.fused_loss(ce, xd, y.to(DEV), *tail) + 0.5 * L.fused_loss(dice, xd, y.to(DEV), *tail))
    lf, _ = run(lambda xd: L.fused_loss(both, xd, y.to(DEV), *tail))
    assert torch.equal(ls, lp) and torch.equal(gs, gp) and torch.equal(ls, lf)
    xc = x.double().requires_grad_(True)
    z = upsampled(xc, size) if fused else xc
    lref = lc.ref_loss(z, yt, w.double(), 0.0, "mean") + 0.5 * rc.ref_region(z, yt, w.double())
    lref.backward()
    check(ls, gs[:, :C], lref, xc.grad, BF16, "CE + 0.5 dice %s" % ("fused" if fused else "dense"))
    if not fused:          # the modules' forward is the fused form
        assert torch.equal(both(on_device(x, BF16), y.to(DEV)).detach(), ls)
        fl = L.FocalLoss2d(gamma=2.0, weight=w).to(DEV)
        assert torch.equal(fl(on_device(x, BF16), y.to(DEV)).detach(),
                           ops().focal_loss(on_device(x, BF16), y.to(DEV), 255, gamma=2.0, weight=w.to(DEV)).detach())


class _DeepWrap(nn.Module):
    """A network/deepv3.py factory behind the call Trainer makes: returns the factory's [main_loss, aux_loss]."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, img, label, training=True):
        return self.net(img, gts=label, aux_gts=label)


def test_trainer_step_with_focal_and_ce_plus_dice():
    """DeepMobileNetV3PlusD at 2 x 64 x 64 with criterion=FocalLoss2d() and criterion_aux=SumLoss(CE, 0.5 RegionLoss2d()): both criteria
    have a fused form and the step launches it (the main head on the fused source, the aux head dense); one Trainer.step run twice
    from the same state gives bit-identical losses and parameters."""
    import deepv3_common as dc
    from mrfp_amd import _lib, conv, loss as L
    from mrfp_amd.config import cfg
    from mrfp_amd.harness import Trainer
    from mrfp_amd.network import deepv3, wider_resnet
    sd = synth.synth_state_dict(dc.spec("DeepMobileNetV3PlusD"), seed=0)
    x, y = synth.synth_batch(2, 64, 64, seed=31)
    x, y = x.to(DEV), y.to(DEV)
    keep = (torch.rand(2, 512, generator=torch.Generator().manual_seed(32)) >= dc.DSN_P).float() / (1.0 - dc.DSN_P)

    def one_step():
        crit = L.FocalLoss2d()
        aux = L.SumLoss((1.0, nn.CrossEntropyLoss(ignore_index=255)), (0.5, L.RegionLoss2d()))
        assert L.fused_ce_kwargs(crit) is not None and L.fused_ce_kwargs(aux) is not None
        with contextlib.redirect_stdout(io.StringIO()):
            m = deepv3.DeepMobileNetV3PlusD(None, dc.NC, crit, aux)
        m.load_state_dict(sd)
        model = _DeepWrap(m.to(DEV)).train()
        tr = Trainer(model, lr=1e-2, loss_weights=(1.0, 0.4))
        names, hook = [], _lib.HOOK[0]
        _lib.HOOK[0] = lambda n, args: names.append(n)
        try:
            loss = tr.step(x, y)
            torch.cuda.synchronize()
        finally:
            _lib.HOOK[0] = hook
        return float(loss.detach()), tr.opt.flat_p.detach().clone(), names

    cfg.MODEL.ACT_DTYPE = F32
    wider_resnet.DROP_MASKS.injected = {"dsn": keep}
    try:
        l1, p1, names = one_step()
        l2, p2, _ = one_step()
    finally:
        wider_resnet.DROP_MASKS.injected = None
        conv.backward_failed()
    for n in ("mrfp_upsample_focal_fwd", "mrfp_upsample_focal_bwd", "mrfp_region_fwd", "mrfp_region_bwd", "mrfp_ce_fwd", "mrfp_ce_bwd"):
        assert n in names, n
    assert math.isfinite(l1) and l1 == l2 and torch.equal(p1.view(torch.int32), p2.view(torch.int32))
    assert bool(torch.isfinite(p1).all())
