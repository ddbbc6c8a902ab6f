"""Weighted / label-smoothed / per-image cross entropy on the GPU (csrc/loss.hip: mrfp_ce_w_*, mrfp_upsample_ce_w_*,
mrfp_label_class_weights) against torch on the CPU in float64 (loss_common.ref_loss: F.cross_entropy for `mean` / `sum`, the
per-image loop over F.nll_loss(weight=w_b) for per-image weights and `image_mean`), and the criteria on the models.

Bounds: those of test_ops_gpu.test_fused_upsample_cross_entropy -- loss relative 1e-5 (fp32) / 2e-3 (16-bit), gradient 2e-5 /
1.5e-2 of the tensor maximum (relerr as defined there).  Inputs are rounded to the activation dtype first."""
import contextlib
import functools
import io
import json
import math
import os

import numpy as np
import pytest
import torch
from torch import nn

import loss_common as lc
from mrfp_amd import synth
from oracle import mrfp_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
CL = torch.channels_last
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
LOSS_TOL = {F32: 1e-5, BF16: 2e-3, F16: 2e-3}
GRAD_TOL = {F32: 2e-5, BF16: 1.5e-2, F16: 1.5e-2}


def dname(d):
    return str(d).replace("torch.", "")


def ops():
    from mrfp_amd import ops as o
    return o


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


def kwargs_of(mode, w, eps):
    return dict(weight=None if w is None else w.to(DEV), label_smoothing=eps, reduction="sum" if mode == "sum" else "mean",
                per_image=mode == "image_mean")


def bwd_scale(dtype, mode):
    """0.7, or the 4096 loss scale of the float16 tests (1/#pixels gradients survive float16); `sum` gradients are O(1)."""
    return 4096.0 if dtype == F16 and mode != "sum" else 0.7


def pad32(x, dtype):
    B, C, Hi, Wi = x.shape
    P = torch.zeros(B, 32, Hi, Wi)
    P[:, :C] = x
    return P.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)


def inputs(shape, out, dtype, per_image_w, seed, scale):
    """(logits rounded to dtype, labels, labels for torch, weights [C] or [B,C]) of one case."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, H, W, generator=g) * scale).to(dtype).float()
    y = lc.make_labels(B, C, out[0], out[1], g)
    w = lc.make_weights(C, g, rows=B if per_image_w else None)
    return x, y, lc.mask_invalid(y, C), w


def check(ld, gd, lref, gref, dtype, what):
    le = abs(ld.item() - lref.item()) / abs(lref.item())
    ge = relerr(gd, gref)
    print("%s: loss relerr %.3g gradient relerr %.3g" % (what, le, ge))
    assert le < LOSS_TOL[dtype] and ge < GRAD_TOL[dtype], (what, le, ge)


DENSE = [(2, 19, 12, 10), (1, 19, 7, 9), (3, 5, 4, 6), (2, 64, 5, 7), (2, 8, 3, 3)]


@pytest.mark.parametrize("mode", lc.MODES)
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("shape", DENSE, ids=str)
def test_dense_weighted_cross_entropy(shape, dtype, eps, mode):
    """ops.cross_entropy(weight=, label_smoothing=, reduction=, per_image=): shared weights for mean / sum (torch's own
    F.cross_entropy is the reference), one weight row per image for image_mean.  One class has weight exactly 0, one is absent,
    ~10 % of the labels are 255 and a few are -1 / C."""
    B, C, H, W = shape
    x, y, yt, w = inputs(shape, (H, W), dtype, mode == "image_mean", 100 + sum(shape), 3.0)
    s = bwd_scale(dtype, mode)
    xc = x.double().requires_grad_(True)
    lref = lc.ref_loss(xc, yt, w.double(), eps, mode)
    (lref * s).backward()
    xd = x.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)
    ld = ops().cross_entropy(xd, y.to(DEV), 255, **kwargs_of(mode, w, eps))
    (ld * s).backward()
    assert ld.dtype == F32 and xd.grad.dtype == dtype
    check(ld, xd.grad, lref, xc.grad, dtype, "dense %s %s eps=%g %s" % (shape, dname(dtype), eps, mode))


FUSED = [((2, 19, 12, 10), (48, 40)), ((1, 19, 7, 9), (25, 33)), ((2, 19, 3, 257), (7, 771))]


@pytest.mark.parametrize("mode", lc.MODES)
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("case", FUSED, ids=str)
def test_fused_upsample_weighted_cross_entropy(case, dtype, eps, mode):
    """ops.upsample_cross_entropy with the same keywords == Upsample() then the weighted loss on the CPU; scores at pitch 32, the
    gradient of the pad channels exactly 0."""
    shape, out = case
    B, C = shape[:2]
    x, y, yt, w = inputs(shape, out, dtype, mode == "image_mean", 200 + sum(shape), 2.0)
    s = bwd_scale(dtype, mode)
    xc = x.double().requires_grad_(True)
    lref = lc.ref_loss(orc.upsample_bilinear_ac(xc, out), yt, w.double(), eps, mode)
    (lref * s).backward()
    Pd = pad32(x, dtype)
    ld = ops().upsample_cross_entropy(Pd, y.to(DEV), out, C, 255, **kwargs_of(mode, w, eps))
    (ld * s).backward()
    check(ld, Pd.grad[:, :C], lref, xc.grad, dtype, "fused %s %s eps=%g %s" % (case, dname(dtype), eps, mode))
    assert float(Pd.grad[:, C:].abs().max()) == 0.0


# ---- above the workgroup cap, several images: 3 x 419 x 419 = 526 683 pixels > 2048 * 256, 682 workgroups per image -------------------
BIG_B, BIG_C, BIG_LOW, BIG_S = 3, 19, 105, 419
BIG_EPS = 0.1


@functools.lru_cache(maxsize=None)
def big_case(kind, dtype):
    """Inputs and the float64 reference (loss, gradient) of both modes, computed once per (kind, dtype) and not modified."""
    side = BIG_S if kind == "dense" else BIG_LOW
    x, y, yt, w = inputs((BIG_B, BIG_C, side, side), (BIG_S, BIG_S), dtype, True, 300 + side, 2.0)
    ref = {}
    for mode in ("image_mean", "mean"):
        xc = x.double().requires_grad_(True)
        full = xc if kind == "dense" else orc.upsample_bilinear_ac(xc, (BIG_S, BIG_S))
        lref = lc.ref_loss(full, yt, w.double(), BIG_EPS, mode)
        (lref * 0.7).backward()
        ref[mode] = (lref.detach(), xc.grad)
    return x, y, w, ref


@pytest.mark.parametrize("mode", ["image_mean", "mean"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
@pytest.mark.parametrize("kind", ["dense", "fused"])
def test_above_the_workgroup_cap_with_per_image_weights(kind, dtype, mode):
    """B = 3 at 419 x 419: the grid is (682, 3), every workgroup walks a second pixel in part of its threads, the finalize kernel
    reduces 682 partials per image; per-image weights [3,19] (each image its own zero-weight class), eps = 0.1."""
    x, y, w, ref = big_case(kind, dtype)
    lref, gref = ref[mode]
    from mrfp_amd import _lib
    o = ops()
    assert int(_lib.lib().mrfp_ce_w_nblocks(BIG_B, BIG_S * BIG_S)) == 3 * 682
    kw = kwargs_of(mode, w, BIG_EPS)
    if kind == "dense":
        xd = x.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)
        ld = o.cross_entropy(xd, y.to(DEV), 255, **kw)
        (ld * 0.7).backward()
        grad = xd.grad
    else:
        Pd = pad32(x, dtype)
        ld = o.upsample_cross_entropy(Pd, y.to(DEV), (BIG_S, BIG_S), BIG_C, 255, **kw)
        (ld * 0.7).backward()
        grad = Pd.grad[:, :BIG_C]
        assert float(Pd.grad[:, BIG_C:].abs().max()) == 0.0
    check(ld, grad, lref, gref, dtype, "big %s %s %s" % (kind, dname(dtype), mode))


def test_shared_weights_per_image_and_per_image_weights_batch_mean():
    """The two pairings the crossing above leaves out, at a small shape: image_mean with one shared weight row (the batch-weights
    form of the per-image criterion) and mean / sum with per-image rows."""
    shape = (3, 19, 12, 10)
    for per_image_w, mode in ((False, "image_mean"), (True, "mean"), (True, "sum")):
        x, y, yt, w = inputs(shape, shape[2:], F32, per_image_w, 41, 3.0)
        xc = x.double().requires_grad_(True)
        lref = lc.ref_loss(xc, yt, w.double(), 0.1, mode)
        lref.backward()
        xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
        ld = ops().cross_entropy(xd, y.to(DEV), 255, **kwargs_of(mode, w, 0.1))
        ld.backward()
        check(ld, xd.grad, lref, xc.grad, F32, "pairing %s %s" % (per_image_w, mode))


@pytest.mark.parametrize("dtype,scale", [(F32, 0.7), (BF16, 0.7), (F16, 4096.0)], ids=["float32-0.7", "bfloat16-0.7", "float16-4096"])
def test_backward_scale(dtype, scale):
    """The incoming gradient multiplies every element: 0.7, and the 4096 loss scale of the float16 path (passed as backward()'s
    argument, as test_f16_gpu.test_upsample_ce_f16 does)."""
    case, out = (2, 19, 12, 10), (48, 40)
    x, y, yt, w = inputs(case, out, dtype, False, 51, 2.0)
    xc = x.double().requires_grad_(True)
    lref = lc.ref_loss(orc.upsample_bilinear_ac(xc, out), yt, w.double(), 0.1, "mean")
    lref.backward()
    Pd = pad32(x, dtype)
    ld = ops().upsample_cross_entropy(Pd, y.to(DEV), out, 19, 255, **kwargs_of("mean", w, 0.1))
    ld.backward(torch.tensor(scale, device=DEV))
    check(ld, Pd.grad[:, :19].float() / scale, lref, xc.grad, dtype, "scale %g fused" % scale)
    xf, yf = orc.upsample_bilinear_ac(x, out).to(dtype).float(), y
    xc = xf.double().requires_grad_(True)
    lref = lc.ref_loss(xc, yt, w.double(), 0.1, "mean")
    lref.backward()
    xd = xf.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)
    ld = ops().cross_entropy(xd, yf.to(DEV), 255, **kwargs_of("mean", w, 0.1))
    ld.backward(torch.tensor(scale, device=DEV))
    check(ld, xd.grad.float() / scale, lref, xc.grad, dtype, "scale %g dense" % scale)


def _run(kind, dtype, x, y, size, C, scale=1.0, **kw):
    """One forward + backward of the dense (`x` upsampled on the CPU first) or fused operator -> (loss, gradient of the logits / scores)."""
    o = ops()
    if kind == "dense":
        full = x if tuple(x.shape[2:]) == tuple(size) else orc.upsample_bilinear_ac(x, size).to(dtype).float()
        xd = full.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)
        ld = o.cross_entropy(xd, y.to(DEV), 255, **kw)
    else:
        xd = pad32(x, dtype)
        ld = o.upsample_cross_entropy(xd, y.to(DEV), size, C, 255, **kw)
    (ld * scale).backward()
    return ld, xd.grad


def test_two_runs_are_bit_identical():
    """Per-workgroup partials + a finalize kernel in a fixed order, no floating-point atomics: the same call twice gives the same
    bits, loss and gradient, dense and fused, at the many-workgroup shape and at a small one."""
    small = inputs((2, 19, 12, 10), (48, 40), BF16, True, 55, 2.0)
    for kind, dtype in (("dense", F32), ("fused", BF16)):
        xb, yb, wb, _ = big_case(kind, dtype)
        for x, y, w, size in ((xb, yb, wb, (BIG_S, BIG_S)), (small[0], small[1], small[3], (48, 40))):
            got = [_run(kind, dtype, x, y, size, 19, **kwargs_of("image_mean", w, 0.1)) for _ in range(2)]
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), (kind, tuple(x.shape))
            assert math.isfinite(got[0][0].item())


@pytest.mark.parametrize("kind", ["dense", "fused"])
def test_null_weights_agree_with_the_plain_path(kind):
    """weight=None / label_smoothing=0 / 'mean' through the weighted criterion (the one autograd function's `crit`, entries
    mrfp_[upsample_]ce_w_*) -- forced by the private `_general` switch (a null weight pointer) and by weight=ones(C) -- against the
    plain criterion's path, within the fp32 bound; reduction='sum' and label_smoothing=0.1 with a null weight against torch."""
    case, out = (2, 19, 12, 10), (48, 40)
    x, _, y, _ = inputs(case, out, F32, False, 61, 2.0)
    l0, g0 = _run(kind, F32, x, y, out, 19)
    assert l0.grad_fn.crit.stem == "ce"
    for kw in (dict(_general=True), dict(weight=torch.ones(19, device=DEV))):
        l1, g1 = _run(kind, F32, x, y, out, 19, **kw)
        assert l1.grad_fn.crit.stem == "ce_w" and type(l1.grad_fn) is type(l0.grad_fn), l1.grad_fn.crit.stem
        assert abs(l1.item() - l0.item()) / abs(l0.item()) < LOSS_TOL[F32] and relerr(g1, g0) < GRAD_TOL[F32], kw
    for eps, mode in ((0.0, "sum"), (0.1, "mean")):
        xc = x.double().requires_grad_(True)
        lref = lc.ref_loss(orc.upsample_bilinear_ac(xc, out), y, None, eps, mode)
        lref.backward()
        ld, gd = _run("fused", F32, x, y, out, 19, **kwargs_of(mode, None, eps))
        check(ld, gd[:, :19], lref, xc.grad, F32, "null weight eps=%g %s" % (eps, mode))


def test_zero_denominators():
    """All-ignored batch: `mean` is NaN (0/0, as torch), `sum` is 0.0.  One all-ignored image under image_mean: NaN; the same batch
    under `mean` is finite."""
    o = ops()
    x, y, yt, w = inputs((2, 19, 12, 10), (12, 10), F32, False, 71, 3.0)
    xd = x.to(DEV).contiguous(memory_format=CL)
    Pd = pad32(x, F32).detach()
    none = torch.full((2, 12, 10), 255, dtype=torch.long, device=DEV)
    half = y.clone()
    half[1] = 255
    half = half.to(DEV)
    for f in (lambda t, **k: o.cross_entropy(xd, t, 255, **k), lambda t, **k: o.upsample_cross_entropy(Pd, t, (12, 10), 19, 255, **k)):
        assert math.isnan(f(none, weight=w.to(DEV)).item())
        assert f(none, weight=w.to(DEV), reduction="sum").item() == 0.0
        assert math.isnan(f(none, weight=w.to(DEV), per_image=True).item())
        assert math.isnan(f(half, weight=w.to(DEV), per_image=True).item())
        assert math.isfinite(f(half, weight=w.to(DEV)).item())
    assert torch.isnan(torch.nn.functional.cross_entropy(x, torch.full((2, 12, 10), 255), weight=w, ignore_index=255))


def test_operator_refusals():
    from mrfp_amd import _lib
    o = ops()
    x, y, _, w = inputs((2, 19, 6, 5), (6, 5), F32, False, 81, 1.0)
    xd, yd = x.to(DEV).contiguous(memory_format=CL), y.to(DEV)
    bad = [dict(reduction="none"), dict(weight=w), dict(weight=w.to(DEV).double()), dict(weight=torch.ones(3, 19, device=DEV)),
           dict(weight=torch.ones(18, device=DEV)), dict(label_smoothing=1.0), dict(per_image=True, reduction="sum")]
    for kw in bad:
        with pytest.raises(_lib.MrfpHipError):
            o.cross_entropy(xd, yd, 255, **kw)
        with pytest.raises(_lib.MrfpHipError):
            o.upsample_cross_entropy(xd, yd, (6, 5), 19, 255, **kw)


# ---- per-image class weights --------------------------------------------------------------------------------------------------
def _label_maps(kind, H, W):
    g = torch.Generator().manual_seed(91)
    t = torch.randint(0, 19, (2, H, W), generator=g)
    t[0] = torch.randint(0, 5, (H, W), generator=g)            # image 0 lacks classes 5..18
    t[torch.rand(2, H, W, generator=g) < 0.1] = 255
    if H * W == 1:
        t[0], t[1] = 3, 11
    if kind == "one_image_255":
        t[1] = 255
    elif kind == "all_255":
        t[:] = 255
    return t


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("kind", ["mixed", "one_image_255", "all_255"])
@pytest.mark.parametrize("hw", [(33, 47), (1, 1)], ids=str)
def test_label_class_weights_equal_numpy(hw, kind, norm, batch):
    """ops.label_class_weights == np.histogram(t, range(C+1)) -> the two formulas in float64 -> .astype(float32), EQUAL not close.
    An image without some classes gives those weight 1; in a map of only 255 every n_c is 0, so every weight is 1."""
    t = _label_maps(kind, *hw)
    for ub in (1.0, 0.3):
        got = ops().label_class_weights(t.to(DEV), 19, ub, norm, batch)
        want = lc.np_class_weights(t.numpy(), 19, ub, norm, batch)
        assert got.dtype == F32 and tuple(got.shape) == ((1, 19) if batch else (2, 19))
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    if kind == "all_255":
        assert (want == 1.0).all()
    if kind == "one_image_255" and not batch:
        assert (want[1] == 1.0).all() and (want[0, 5:] == 1.0).all() and (want[0, :5] != 1.0).all() == (hw != (1, 1))


def test_image_based_criterion_stays_on_the_device(monkeypatch):
    """ImageBasedCrossEntropyLoss2d(19) on (2,19,24,20) logits against the float64 per-image loop with numpy's weights; during
    forward and backward torch.cuda.synchronize, Tensor.cpu and Tensor.item raise."""
    from mrfp_amd.loss import ImageBasedCrossEntropyLoss2d
    x, y, yt, _ = inputs((2, 19, 24, 20), (24, 20), F32, False, 95, 3.0)
    y = yt                         # (np.histogram's last bin would count a label equal to C; the label tables never produce one)
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    yd = y.to(DEV)
    for batch_weights in (False, True):
        crit = ImageBasedCrossEntropyLoss2d(19, batch_weights=batch_weights).to(DEV)
        xd.grad = None

        def boom(*a, **k):
            raise AssertionError("host synchronisation inside the criterion")
        with monkeypatch.context() as mp:
            mp.setattr(torch.cuda, "synchronize", boom)
            mp.setattr(torch.Tensor, "cpu", boom)
            mp.setattr(torch.Tensor, "item", boom)
            ld = crit(xd, yd)
            ld.backward()
        w = torch.from_numpy(lc.np_class_weights(y.numpy(), 19, 1.0, False, batch_weights)).double()
        xc = x.double().requires_grad_(True)
        lref = lc.ref_loss(xc, y, w[0] if batch_weights else w, 0.0, "image_mean")
        lref.backward()
        check(ld, xd.grad, lref, xc.grad, F32, "ImageBasedCrossEntropyLoss2d batch_weights=%s" % batch_weights)


# ---- the criteria on the models ---------------------------------------------------------------------------------------------------
class Wrapped(nn.Module):
    """A module the criterion helper does not recognise: the model takes the stock path (criterion(upsample(...).float(), gts))."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x, y):
        return self.inner(x, y)


def _mrfp(dtype):
    from mrfp_amd import deepv3
    from mrfp_amd.config import cfg
    cfg.MODEL.ACT_DTYPE = dtype
    spec = json.load(open(os.path.join(HERE, "golden", "state_dict_spec.json")))
    with contextlib.redirect_stdout(io.StringIO()):
        m = deepv3.MRFPPlus(19, criterion=nn.CrossEntropyLoss(ignore_index=255))
    m.load_state_dict(synth.synth_state_dict([(k, tuple(s)) for k, s in spec["MRFPPlus"]], seed=0))
    m = m.to(DEV).train()
    m.rng = deepv3.InjectedRandom((True, True, True), synth.synth_noise(2, seed=2))
    return m


def _mobilenet(dtype):
    import deepv3_common as dc
    from mrfp_amd.config import cfg
    from mrfp_amd.network import deepv3
    cfg.MODEL.ACT_DTYPE = dtype
    crit = nn.CrossEntropyLoss(ignore_index=255)
    with contextlib.redirect_stdout(io.StringIO()):
        m = deepv3.DeepMobileNetV3PlusD(None, 19, crit, crit)
    m.load_state_dict(synth.synth_state_dict(dc.spec("DeepMobileNetV3PlusD"), seed=0))
    return m.to(DEV).train()


@pytest.fixture(scope="module", params=["MRFPPlus", "DeepMobileNetV3PlusD"])
def model(request):
    from mrfp_amd.config import cfg
    try:
        m = (_mrfp if request.param == "MRFPPlus" else _mobilenet)(BF16)
        x, y = synth.synth_batch(2, 128, 128, seed=3)
        yield request.param, m, x.to(DEV), y.to(DEV)
    finally:
        cfg.MODEL.ACT_DTYPE = torch.float32


def _criteria():
    from mrfp_amd.loss import ImageBasedCrossEntropyLoss2d
    g = torch.Generator().manual_seed(7)
    w = lc.make_weights(19, g)
    return {"weighted_smoothed": lambda: nn.CrossEntropyLoss(weight=w.clone(), ignore_index=255, label_smoothing=0.1),
            "image_based": lambda: ImageBasedCrossEntropyLoss2d(19)}


def _train_step(name, m, x, y, crit):
    """One forward + backward with `crit` as the criterion(s) -> (main loss, d final2.weight)."""
    crit = crit.to(DEV)
    m.criterion = crit
    if name != "MRFPPlus":
        m.criterion_aux = crit
    m.zero_grad(set_to_none=True)
    if name == "MRFPPlus":
        main = total = m(x, y, training=True)
    else:
        out = m(x, gts=y)
        main, total = out[0], out[0] + out[1]
    total.backward()
    return main.detach().float().clone(), m.final2[0].weight.grad.detach().float().clone()


@pytest.mark.parametrize("which", ["weighted_smoothed", "image_based"])
def test_model_criteria_run_on_the_fused_kernels(model, which, monkeypatch):
    """With the criterion's own forward patched to raise, a training step still gives a finite loss (the criterion is computed by
    the fused kernels, main and auxiliary head); and it agrees with the stock path -- the same criterion wrapped in a module the
    helper does not recognise -- within the 16-bit bounds (bf16 activations)."""
    name, m, x, y = model
    crit = _criteria()[which]()

    def boom(self, *a, **k):
        raise AssertionError("the model called the criterion's forward: it left the fused loss kernels")
    with monkeypatch.context() as mp:
        mp.setattr(type(crit), "forward", boom)
        loss, grad = _train_step(name, m, x, y, crit)
    assert math.isfinite(loss.item()) and torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    sloss, sgrad = _train_step(name, m, x, y, Wrapped(_criteria()[which]()))
    le, ge = abs(loss.item() - sloss.item()) / abs(sloss.item()), relerr(grad, sgrad)
    print("%s %s: fused %.6f stock %.6f relerr %.3g, d final2.weight relerr %.3g" % (name, which, loss.item(), sloss.item(), le, ge))
    assert le < LOSS_TOL[BF16] and ge < GRAD_TOL[BF16], (le, ge)


def test_plain_criterion_still_takes_the_plain_launches(model, monkeypatch):
    """nn.CrossEntropyLoss(ignore_index=255): the head calls ops.upsample_cross_entropy with every new keyword at its default, the
    launches are mrfp_upsample_ce_fwd / _bwd (none of the weighted entries), and the loss is bit-identical to the operator called as
    before this feature."""
    from mrfp_amd import _lib, ops as o
    name, m, x, y = model
    orig, seen, names = o.upsample_cross_entropy, [], []

    def spy(*a, **k):
        out = orig(*a, **k)
        seen.append((a, k, out))
        return out
    monkeypatch.setattr(o, "upsample_cross_entropy", spy)
    hook = _lib.HOOK[0]
    _lib.HOOK[0] = lambda n, args: names.append(n)
    try:
        loss, _ = _train_step(name, m, x, y, nn.CrossEntropyLoss(ignore_index=255))
    finally:
        _lib.HOOK[0] = hook
        monkeypatch.undo()
    assert len(seen) == 1
    (P, gts, size, nc, ignore), kw, out = seen[0]
    assert ignore == 255 and nc == 19 and tuple(size) == (128, 128)
    assert kw == dict(weight=None, label_smoothing=0.0, reduction="mean", per_image=False)
    assert "mrfp_upsample_ce_fwd" in names and "mrfp_upsample_ce_bwd" in names and not [n for n in names if "_ce_w_" in n]
    again = o.upsample_cross_entropy(P.detach(), gts, size, nc, 255)
    assert torch.equal(again, out.detach()) and again.float().item() == loss.item()


def test_loss_launches_equal_the_recorded_ones():
    """tools/record_loss_launches.py replayed: for every case of its list, each entry point the public call reaches, every
    non-pointer argument by value, every pointer argument as null or not, and the shape, dtype and strides of the returned loss and
    of the gradient equal tests/golden/loss_launches.json -- recorded once, with the same script, from the commit before the loss
    operators' six autograd classes became one over (score source, criterion)."""
    from tools import record_loss_launches as rec
    from mrfp_amd import _lib
    hook = _lib.HOOK[0]
    got = json.loads(json.dumps(rec.record()))
    assert _lib.HOOK[0] is hook
    with open(os.path.join(HERE, "golden", "loss_launches.json")) as f:
        want = json.load(f)
    assert list(got) == list(want) and len(want) == 408
    for name in want:
        assert got[name] == want[name], name
    entries = {c[0] for v in want.values() for c in v["calls"]}
    stems = {p + s + d for p in ("mrfp_", "mrfp_upsample_") for s in ("ce", "ce_w", "soft_nll") for d in ("_fwd", "_bwd")}
    assert entries == stems | {"mrfp_ohem_target", "mrfp_upsample_ohem_target", "mrfp_bilinear_bwd"}
