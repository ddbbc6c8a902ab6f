"""Row kernels, depthwise strips and capped 1-D grids at shapes where a workgroup walks MANY lines / rows / pixels.

The op-level files (test_ops_gpu.py, test_depthwise_gpu.py, test_f16_gpu.py) run every kernel at shapes where each loop of the
launch geometry runs once; the training workload never does.  Here B * rows exceeds the launch caps at tensors of a few hundred
kilobytes (tests/launch_geometry_common.py holds the shapes, tests/test_launch_geometry_cpu.py proves on the host that each takes
the path it is listed for):

  1. row kernels where workgroup j walks lines j, j + ly, ... and the finalize kernels sum more than 3 x their lanes partial rows,
  2. lines longer than one trip of the row threads (a full trip followed by a masked partial one),
  3. depthwise 3x3 with strips of several rows, a shorter last strip, stride 2 across strip boundaries,
  4. cross entropy / arg-max histogram kernels above the 2048-workgroup cap (grid-stride loop, 2048 partial rows).

Reference: torch on the CPU in float64, fed the dtype-rounded inputs.  Tolerances are the ones the project states for the same
operator and dtype (tol() of test_ops_gpu.py and its multiples, TOL of test_depthwise_gpu.py, the cross-entropy bounds of
test_cross_entropy_and_hist / test_fused_upsample_cross_entropy), all relative to the reference tensor's maximum.

ReLU gates.  A float64 reference and an fp32 kernel may disagree about the sign of a pre-activation that lies within fp32 rounding
of zero; one such element moves its input gradient and its channel's weight gradient by percents.  Like a tie inside a max-pool
window this is a property of the input, not of the kernel: settle() (tests/rounding_model_common.py, shared with
test_ops_16bit_gpu.py) moves the (few per million) input values whose float64 pre-activation is closer to the gate than BAND x the
magnitude of its terms, and the tests assert that none is left.

Second assertion where an output line does not depend on which workgroup wrote it (bilinear, max pool, add / ReLU, the apply pass
of an eval-mode BatchNorm): the batched call is BIT-IDENTICAL to the same tensor run image by image -- at B = 1 every shape here
gives one line per workgroup.

Bounds that were measured instead of inherited: BILINEAR_F32_Y below (the fp32 bilinear resize along lines of 700 pixels), nothing
else.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eval_tta_common as etc
import launch_geometry_common as lg
from rounding_model_common import no_tie_planes, norm_pre, settle, window_max_count
from oracle import mrfp_oracle as orc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(lg.row_blocks_overridden(), reason=lg.SKIP_REASON)]
DEV = "cuda:0"
CL = torch.channels_last
F32, BF16, F16 = lg.F32, lg.BF16, lg.F16
EPS = 1e-5


def ops():
    from mrfp_amd import ops as o
    return o


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


def tol(dtype):                                  # test_ops_gpu.py
    return 2e-5 if dtype == torch.float32 else 2.5e-2


DW_TOL = {F32: 1e-3, BF16: 2e-2, F16: 2e-2}      # test_depthwise_gpu.py


def rnd(*shape, seed=0, scale=1.0, shift=0.0, dtype=F32):
    """scale * randn + shift, rounded to `dtype` (returned as float32 on the host)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype).float()


def dev(x, dtype, grad=True):
    return x.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(grad)


def gdev(g, dtype):
    return g.to(DEV, dtype).contiguous(memory_format=CL)


def leaf64(*ts):
    return [None if t is None else t.double().clone().requires_grad_(True) for t in ts]


def dname(dtype):
    return str(dtype).replace("torch.", "")


def hooked(fn):
    """-> (result of fn(), names of the library entry points it called)."""
    from mrfp_amd import _lib
    names = []
    _lib.HOOK[0] = lambda name, args: names.append(name)
    try:
        return fn(), names
    finally:
        _lib.HOOK[0] = None


def per_image(fn, *ts):
    """fn on every image of the batch on its own (B = 1: one line per workgroup), results concatenated."""
    outs = [fn(*[t[i:i + 1].contiguous(memory_format=CL) for t in ts]) for i in range(ts[0].shape[0])]
    return torch.cat(outs, 0)


ROW_CASES = [(n, d) for n in lg.ROW_SHAPES for d in lg.ROW_SHAPES[n]["dtypes"]]
ROW_IDS = ["%s-%s" % (n, dname(d)) for n, d in ROW_CASES]


# =====================================================================================================================================
# 1. row kernels with many lines per workgroup
# =====================================================================================================================================
@pytest.mark.parametrize("name,dtype", ROW_CASES, ids=ROW_IDS)
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)], ids=["plain", "relu", "relu_res"])
def test_batch_norm_act_many_lines(name, dtype, relu, res):
    """stats_kernel (forward and backward statistics), affine_fwd_kernel, affine_bwd_kernel (identity instance), bn_finalize /
    bn_bwd_finalize over B * ly > 384 partial rows; with a residual in a 16-bit type and C % 8 == 0 the sign-mask instances
    (mrfp_affine_fwd_relu_mask, mrfp_stats_bwd_mask, mrfp_affine_bwd_mask).  Training statistics, running statistics, every
    gradient, and the eval-mode forward / backward, against float64."""
    o = ops()
    shape = lg.ROW_SHAPES[name]["shape"]
    B, C, H, W = shape
    g = torch.Generator().manual_seed(C)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    r = rnd(*shape, seed=2, dtype=dtype) if res else None
    x = rnd(*shape, seed=1, scale=3.0, shift=1.5, dtype=dtype)
    gy = rnd(*shape, seed=3, dtype=dtype)
    if relu:
        both = lambda v: norm_pre(w, b, r, (0, 2, 3))(v) + norm_pre(w, b, None, (0, 2, 3), stats=(rm, rv))(v)
        x = settle(x, dtype, both)
    # float64
    x64, w64, b64, r64 = leaf64(x, w, b, r)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    y64 = F.batch_norm(x64, rm64, rv64, w64, b64, True, 0.1, EPS)
    y64 = y64 + r64 if res else y64
    y64 = F.relu(y64) if relu else y64
    y64.backward(gy.double())
    # HIP
    xd, rd = dev(x, dtype), (dev(r, dtype) if res else None)
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    rm_d, rv_d = rm.to(DEV), rv.to(DEV)

    def run():
        yd = o.batch_norm_act(xd, wd, bd, rm_d, rv_d, training=True, relu=relu, res=rd)
        yd.backward(gdev(gy, dtype))
        return yd
    yd, names = hooked(run)
    masked = res and dtype != F32 and C % 8 == 0
    assert ("mrfp_stats_bwd_mask" in names) == masked and ("mrfp_affine_bwd_mask" in names) == masked, names
    t = tol(dtype)
    errs = dict(y=relerr(yd, y64), rm=relerr(rm_d, rm64), rv=relerr(rv_d, rv64), dx=relerr(xd.grad, x64.grad),
                dw=relerr(wd.grad, w64.grad), db=relerr(bd.grad, b64.grad))
    if res:
        errs["dres"] = relerr(rd.grad, r64.grad)
    print(name, dtype, relu, res, "train", errs)
    assert errs["y"] < t
    assert errs["rm"] < 1e-5 and errs["rv"] < 1e-5 + (0 if dtype == F32 else 1e-2)
    assert errs["dx"] < 10 * t and errs["dw"] < 10 * t and errs["db"] < 10 * t
    if res:
        assert errs["dres"] < t
    # eval mode: forward and backward with the running statistics as constants
    xe = dev(x, dtype)
    we, be = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    ye = o.batch_norm_act(xe, we, be, rm.to(DEV), rv.to(DEV), training=False, relu=relu)
    ye.backward(gdev(gy, dtype))
    x2, w2, b2 = leaf64(x, w, b)
    y2 = F.batch_norm(x2, rm.double(), rv.double(), w2, b2, False, 0.1, EPS)
    y2 = F.relu(y2) if relu else y2
    y2.backward(gy.double())
    errs = dict(y=relerr(ye, y2), dx=relerr(xe.grad, x2.grad), dw=relerr(we.grad, w2.grad), db=relerr(be.grad, b2.grad))
    print(name, dtype, relu, res, "eval", errs)
    assert errs["y"] < t and errs["dx"] < 10 * t and errs["dw"] < 10 * t and errs["db"] < 10 * t


@pytest.mark.parametrize("dtype", [BF16, F16], ids=dname)
@pytest.mark.parametrize("name", ["two_lines_uneven", "two_lines_c64", "single_line_many_partials"])
def test_residual_sign_mask_many_lines_equals_reading_y(name, dtype):
    """The 1-bit sign mask of the residual BatchNorm -> add -> ReLU tail (stats_kernel<.., YM>, affine_bwd_kernel<.., YM>) where a
    workgroup walks several lines: outputs and every gradient bit-identical with the path that re-reads y (ops.SIGN_MASK off), as
    test_residual_bn_relu_sign_mask_equals_reading_y holds it at one line per workgroup.  (Against float64: the relu_res cases of
    test_batch_norm_act_many_lines.)"""
    o = ops()
    shape = lg.ROW_SHAPES[name]["shape"]
    B, C, H, W = shape
    x, r, gy = rnd(*shape, seed=11, scale=2.0), rnd(*shape, seed=12), rnd(*shape, seed=13)
    r[0, :, 0, 0] = -1e30                              # a clamped pixel
    r[-1, :, -1, -1] = 0.0
    w, b = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    outs = []
    for use_mask in (True, False):
        o.SIGN_MASK[0] = use_mask
        try:
            xd, rd = dev(x, dtype), dev(r, dtype)
            wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)

            def run():
                yd = o.batch_norm_act(xd, wd, bd, torch.zeros(C, device=DEV), torch.ones(C, device=DEV), training=True, relu=True, res=rd)
                yd.backward(gdev(gy, dtype))
                return yd
            yd, names = hooked(run)
            assert ("mrfp_stats_bwd_mask" in names) == use_mask
            outs.append((yd.detach().clone(), xd.grad.clone(), rd.grad.clone(), wd.grad.clone(), bd.grad.clone()))
        finally:
            o.SIGN_MASK[0] = True
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)
    assert (outs[0][0] == 0).any() and (outs[0][0] > 0).any()


@pytest.mark.parametrize("name,dtype", [("two_lines_uneven", F32), ("two_lines_uneven", BF16), ("scalar_c19", F32), ("wide_c2048", F32),
                                        ("two_lines_c64", BF16)], ids=lambda v: v if isinstance(v, str) else dname(v))
def test_apply_pass_that_also_emits_plane_sums_many_lines(name, dtype):
    """affine_fwd_stats_kernel (batch_norm_act / instance_norm_act with emit_stats=True): the same output bits as the plain apply
    pass, and partial rows bit-identical with those of a statistics pass over the stored output, where each workgroup accumulates
    over several lines (and, at C = 2048 in fp32, over two rounds of channel vectors)."""
    o = ops()
    shape = lg.ROW_SHAPES[name]["shape"]
    B, C, H, W = shape
    x = rnd(*shape, seed=21, scale=3.0, shift=1.5, dtype=dtype)
    w, b = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    with torch.no_grad():
        for kind in ("bn", "in"):
            outs = []
            for emit in (True, False):
                xd = dev(x, dtype, grad=False)
                if kind == "bn":
                    call = lambda: o.batch_norm_act(xd, w.to(DEV), b.to(DEV), None, None, training=True, relu=True, emit_stats=emit)
                else:
                    call = lambda: o.instance_norm_act(xd, w.to(DEV), b.to(DEV), relu=False, emit_stats=emit)
                y, names = hooked(call)
                assert ("mrfp_affine_fwd_stats" in names) == emit, (kind, names)
                outs.append(y)
            assert torch.equal(outs[0], outs[1])
            nslab, rows, _ = outs[0]._mrfp_planestats
            nslab2, rows2 = o._stats_fwd(outs[0], None)
            assert nslab == nslab2 == lg.ROW_SHAPES[name]["ly"] and torch.equal(rows, rows2)
            # ... and the sums themselves against float64 of the stored output
            s64 = outs[0].double().cpu().sum((2, 3))
            got = rows.view(B, nslab, 2, C).double().sum(1)[:, 0].cpu()
            assert relerr(got, s64) < 2e-5


@pytest.mark.parametrize("name,dtype", ROW_CASES, ids=ROW_IDS)
@pytest.mark.parametrize("relu,affine", [(False, True), (True, True), (False, False)], ids=["affine", "affine_relu", "plain"])
def test_instance_norm_act_many_lines(name, dtype, relu, affine):
    """Per-image statistics: in_finalize_kernel sums ly rows per image on 128 lanes, in_bwd_finalize_kernel on 8 lanes per image
    (unrolled bodies at ly = 550 and 500); stats / apply kernels with per-image coefficients over several lines."""
    o = ops()
    shape = lg.ROW_SHAPES[name]["shape"]
    B, C, H, W = shape
    x = rnd(*shape, seed=4, scale=50.0, shift=120.0, dtype=dtype)       # stem-like magnitudes (inputs are 0..255)
    w = (torch.rand(C) + 0.5) if affine else None
    b = (torch.randn(C) * 0.1) if affine else None
    gy = rnd(*shape, seed=5, dtype=dtype)
    if relu:
        x = settle(x, dtype, norm_pre(w, b, None, (2, 3)))
    x64, w64, b64 = leaf64(x, w, b)
    y64 = F.instance_norm(x64, None, None, w64, b64, True, 0.1, EPS)
    y64 = F.relu(y64) if relu else y64
    y64.backward(gy.double())
    xd = dev(x, dtype)
    wd = w.to(DEV).requires_grad_(True) if affine else None
    bd = b.to(DEV).requires_grad_(True) if affine else None
    yd = o.instance_norm_act(xd, wd, bd, relu=relu)
    yd.backward(gdev(gy, dtype))
    t = tol(dtype)
    errs = dict(y=relerr(yd, y64), dx=relerr(xd.grad, x64.grad))
    if affine:
        errs.update(dw=relerr(wd.grad, w64.grad), db=relerr(bd.grad, b64.grad))
    print(name, dtype, relu, affine, errs)
    assert errs["y"] < t * (1 if dtype == F32 else 2)
    assert errs["dx"] < 20 * t
    if affine:
        assert errs["dw"] < 10 * t and errs["db"] < 10 * t


@pytest.mark.parametrize("name,dtype", ROW_CASES, ids=ROW_IDS)
def test_np_plus_and_global_avg_pool_many_lines(name, dtype):
    """NP+ (plane_sum_kernel over ly rows per image, the apply pass with per-image coefficients, its backward through
    stats_kernel MODE 1 without a mean) with and without the residual, and the global average pool (mean_finalize)."""
    o = ops()
    shape = lg.ROW_SHAPES[name]["shape"]
    B, C, H, W = shape
    x = (rnd(*shape, seed=6, scale=2.0) + rnd(B, C, 1, 1, seed=7, scale=3.0)).to(dtype).float()
    alpha, beta = 1 + 0.75 * rnd(B, C, 1, 1, seed=8), 0.75 * rnd(B, C, 1, 1, seed=9)
    r = rnd(*shape, seed=11, dtype=dtype)
    gy = rnd(*shape, seed=10, dtype=dtype)
    t = tol(dtype)
    for with_res in (False, True):
        x64, r64 = leaf64(x, r)
        y64 = orc.np_plus(x64, alpha.double(), beta.double())
        y64 = y64 + r64 if with_res else y64
        y64.backward(gy.double())
        xd, rd = dev(x, dtype), dev(r, dtype)
        yd = o.np_plus(xd, alpha.to(DEV), beta.to(DEV), res=rd if with_res else None)
        yd.backward(gdev(gy, dtype))
        errs = dict(y=relerr(yd, y64), dx=relerr(xd.grad, x64.grad))
        print(name, dtype, "np_plus res", with_res, errs)
        assert errs["y"] < t and errs["dx"] < 10 * t
        if with_res:
            assert relerr(rd.grad, gy) < (1e-7 if dtype == F32 else t)
    (x64,) = leaf64(x)
    p64 = F.adaptive_avg_pool2d(x64, 1)
    gp = rnd(B, C, 1, 1, seed=19, dtype=dtype)
    p64.backward(gp.double())
    xd = dev(x, dtype)
    pd = o.global_avg_pool(xd)
    pd.backward(gp.to(DEV, dtype))
    errs = dict(y=relerr(pd, p64), dx=relerr(xd.grad, x64.grad))
    print(name, dtype, "global_avg_pool", errs)
    assert errs["y"] < t and errs["dx"] < t


@pytest.mark.parametrize("name,dtype", [("two_lines_uneven", F32), ("two_lines_uneven", BF16), ("two_lines_c64", BF16),
                                        ("scalar_c19", F32), ("scalar_c19", BF16), ("single_line_many_partials", F32)],
                         ids=lambda v: v if isinstance(v, str) else dname(v))
def test_batch_norm_relu6_many_lines(name, dtype):
    """BatchNorm + ReLU6 in training mode (statistics rows of several lines; backward through the pass mask: the masked kernel
    pair in 16 bit with C % 8 == 0, mrfp_mask_gate + the plain pair otherwise), tolerances of test_batch_norm_relu6_train_vs_fp64."""
    o = ops()
    shape = lg.ROW_SHAPES[name]["shape"]
    B, C, H, W = shape
    t = DW_TOL[dtype]
    g = torch.Generator().manual_seed(3)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    x = settle(rnd(*shape, seed=31, scale=3.0, shift=2.0, dtype=dtype), dtype, norm_pre(w, b, None, (0, 2, 3), gates=(0.0, 6.0)))
    gy = rnd(*shape, seed=32, dtype=dtype)
    xd = dev(x, dtype)
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y = o.batch_norm_relu6(xd, wd, bd, rm, rv, training=True)
    y.backward(gdev(gy, dtype))
    x64, w64, b64 = leaf64(x, w, b)
    rm64, rv64 = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    y64 = F.hardtanh(F.batch_norm(x64, rm64, rv64, w64, b64, True, 0.1, EPS), 0.0, 6.0)
    y64.backward(gy.double())
    errs = dict(y=relerr(y, y64), dx=relerr(xd.grad, x64.grad), dw=relerr(wd.grad, w64.grad), db=relerr(bd.grad, b64.grad),
                rm=relerr(rm, rm64), rv=relerr(rv, rv64))
    print(name, dtype, errs)
    assert errs["y"] < t and errs["dx"] < 5 * t and errs["dw"] < 5 * t and errs["db"] < 5 * t
    assert errs["rm"] < 1e-4 and errs["rv"] < 1e-4


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
@pytest.mark.parametrize("name", sorted(lg.RESIZE_CASES))
def test_hrfp_stage_resize_bn_relu_many_lines(name, dtype):
    """nearest resize -> BatchNorm(train) -> ReLU fused (the RESIZE instances of stats_kernel / affine_fwd_kernel through tabH /
    tabW, affine_bwd_kernel through the inverse tables) at an input whose OUTPUT has B * Ho > 2048."""
    o = ops()
    c = lg.RESIZE_CASES[name]
    shape, rs = c["shape"], c["rs"]
    B, C, H, W = shape
    w, b = torch.randn(C, generator=torch.Generator().manual_seed(5)) * 0.5, torch.zeros(C)
    x = rnd(*shape, seed=11, scale=2.0, shift=0.3, dtype=dtype)

    def pre(v):      # the statistics are those of the RESIZED tensor; every resized pixel is a source pixel, gated as x*A + S
        up = F.interpolate(v, scale_factor=(rs["scale"], rs["scale"]))
        m, var = up.mean((0, 2, 3), keepdim=True), up.var((0, 2, 3), unbiased=False, keepdim=True)
        return norm_pre(w, b, None, None, stats=(m.flatten(), var.flatten()))(v)
    x = settle(x, dtype, pre)
    (x64,) = leaf64(x)
    up = F.interpolate(x64, scale_factor=(rs["scale"], rs["scale"]))
    y64 = F.relu(F.batch_norm(up, None, None, w.double(), b.double(), True, 0.1, EPS))
    assert y64.shape[2] == c["Ho"]
    gy = rnd(*y64.shape, seed=12, dtype=dtype)
    y64.backward(gy.double())
    xd = dev(x, dtype)
    plan = o.nearest_plan(H, W, device=DEV, **rs)
    assert (plan.Ho, plan.Wo) == tuple(y64.shape[2:])
    yd = o.batch_norm_act(xd, w.to(DEV), b.to(DEV), None, None, training=True, relu=True, plan=plan)
    yd.backward(gdev(gy, dtype))
    t = tol(dtype)
    errs = dict(y=relerr(yd, y64), dx=relerr(xd.grad, x64.grad))
    print(name, dtype, errs)
    assert errs["y"] < t and errs["dx"] < 10 * t


def _bilinear(o, x, size, dtype, gy, **kw):
    xd = dev(x, dtype)
    yd = o.upsample_bilinear(xd, size, **kw)
    yd.backward(gdev(gy, dtype))
    return yd.detach(), xd.grad


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=dname)
@pytest.mark.parametrize("name", sorted(lg.BILINEAR_CASES))
def test_bilinear_many_lines(name, dtype):
    """bilinear_fwd_kernel walks output lines ("up": two per workgroup), bilinear_bwd_kernel input lines ("down"); with an addend;
    from a channel-padded source (ldi > C); into / out of a channel block of a wider tensor (concat_upsample).  Against float64,
    and bit-identical with the image-by-image run."""
    o = ops()
    c = lg.BILINEAR_CASES[name]
    shape, size = c["shape"], c["size"]
    B, C, Hi, Wi = shape
    t = tol(dtype)
    x = rnd(*shape, seed=13, dtype=dtype)
    add = rnd(B, C, *size, seed=14, dtype=dtype)
    gy = rnd(B, C, *size, seed=15, dtype=dtype)
    x64, a64 = leaf64(x, add)
    y64 = orc.upsample_bilinear_ac(x64, size)
    y64.backward(gy.double())
    yd, gx = _bilinear(o, x, size, dtype, gy)
    errs = dict(y=relerr(yd, y64), dx=relerr(gx, x64.grad))
    print(name, dtype, errs)
    assert errs["y"] < t and errs["dx"] < 4 * t
    # image by image: one line per workgroup
    y1 = per_image(lambda xi: o.upsample_bilinear(xi, size), gdev(x, dtype))
    assert torch.equal(yd, y1)

    def bwd1(xi, gi):
        xi = xi.clone().requires_grad_(True)
        o.upsample_bilinear(xi, size).backward(gi)
        return xi.grad
    assert torch.equal(gx, per_image(bwd1, gdev(x, dtype), gdev(gy, dtype)))
    # with the addend
    xd, ad = dev(x, dtype), dev(add, dtype)
    ya = o.upsample_bilinear(xd, size, addend=ad)
    ya.backward(gdev(gy, dtype))
    assert relerr(ya, y64.detach() + a64.detach()) < t and torch.equal(xd.grad, gx) and relerr(ad.grad, gy) < t
    # channel-padded source: 2 * C physical channels, the first C used; pad channels of the gradient stay zero
    xp = torch.cat([x, rnd(*shape, seed=16, dtype=dtype)], 1)
    yp, gp = _bilinear(o, xp, size, dtype, gy, channels=C)
    assert torch.equal(yp, yd) and torch.equal(gp[:, :C], gx) and float(gp[:, C:].abs().max()) == 0.0
    # the concatenation forms (ldo / ldd > C): bit-identical with the composition
    if dtype != F16:
        a = rnd(B, 16, *size, seed=17, dtype=dtype)
        gc = rnd(B, 16 + C, *size, seed=18, dtype=dtype)
        if C % (16 // torch.empty((), dtype=dtype).element_size()) == 0:
            outs = []
            for fused in (True, False):
                a_d, b_d = dev(a, dtype), dev(x, dtype)
                (y, names) = hooked(lambda: o.concat_upsample(a_d, b_d, size) if fused
                                    else o.concat_channels([a_d, o.upsample_bilinear(b_d, size)]))
                assert ("mrfp_bilinear_fwd_into" in names) == fused
                y.backward(gdev(gc, dtype))
                outs.append((y.detach().clone(), a_d.grad.clone(), b_d.grad.clone()))
            for u, v in zip(*outs):
                assert torch.equal(u, v)
            assert relerr(outs[0][0][:, 16:], y64) < t


POOL_CASES = [(n, d) for n in lg.POOL_SHAPES for d in (F32, BF16)] + [("c8", F16)]
POOL_IDS = ["%s-%s" % (n, dname(d)) for n, d in POOL_CASES]


@pytest.mark.parametrize("name,dtype", POOL_CASES, ids=POOL_IDS)
def test_maxpool_many_lines(name, dtype):
    """maxpool_fwd_kernel over two output lines per workgroup, maxpool_bwd_kernel over three or four input lines: values exact,
    gradient against float64, both bit-identical with the image-by-image run.  Inputs have no ties inside a window (asserted)."""
    o = ops()
    shape = lg.POOL_SHAPES[name]["shape"]
    x = no_tie_planes(shape, seed=16)
    assert torch.equal(x.to(dtype).float(), x)
    cnt, _ = window_max_count(x.double())
    assert int(cnt.max()) == 1                                    # a tie is a property of the input, not a kernel error
    (x64,) = leaf64(x)
    y64 = F.max_pool2d(x64, 3, 2, 1)
    gy = rnd(*y64.shape, seed=17, dtype=dtype)
    y64.backward(gy.double())
    xd = dev(x, dtype)
    yd = o.max_pool_3x3_s2(xd)
    yd.backward(gdev(gy, dtype))
    assert relerr(yd, y64) == 0.0
    assert relerr(xd.grad, x64.grad) < tol(dtype)
    assert torch.equal(yd.detach(), per_image(lambda xi: o.max_pool_3x3_s2(xi), gdev(x, dtype)))

    def bwd1(xi, gi):
        xi = xi.clone().requires_grad_(True)
        o.max_pool_3x3_s2(xi).backward(gi)
        return xi.grad
    assert torch.equal(xd.grad, per_image(bwd1, gdev(x, dtype), gdev(gy, dtype)))


@pytest.mark.parametrize("name,dtype", POOL_CASES[:-1], ids=POOL_IDS[:-1])
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
def test_instance_norm_relu_pool_many_lines(name, dtype, affine):
    """The fused InstanceNorm -> ReLU -> max pool (mrfp_maxpool_affine_fwd; pool_norm_bwd_kernel PASS 0 and PASS 1 over three or
    four input lines per workgroup) against the two-operator sequence (bounds of
    test_instance_norm_relu_pool_is_the_two_operator_sequence) and against float64.  The float64 comparison of the gradients runs
    in fp32, where the window maxima of the rounded reference are unique wherever they are positive (asserted; all-zero windows
    pass no gradient through the ReLU whichever element the pool picks); in bf16 distinct normalised values round onto each other."""
    o = ops()
    shape = lg.POOL_SHAPES[name]["shape"]
    B, C, H, W = shape
    w, b = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    x = rnd(*shape, seed=41, scale=50.0, shift=120.0, dtype=dtype)
    x = settle(x, dtype, norm_pre(w if affine else None, b if affine else None, None, (2, 3)))
    outs = []
    hits = o.POOL_FUSED_HITS[0]
    for fused in (True, False):
        o.POOL_FUSED[0] = fused
        try:
            xd = dev(x, dtype)
            wd = w.to(DEV).requires_grad_(True) if affine else None
            bd = b.to(DEV).requires_grad_(True) if affine else None
            yd = o.instance_norm_relu_pool(xd, wd, bd)
            gy = rnd(*yd.shape, seed=42, dtype=dtype)
            yd.backward(gdev(gy, dtype))
            outs.append((yd.detach(), xd.grad, wd.grad if affine else None, bd.grad if affine else None))
        finally:
            o.POOL_FUSED[0] = True
    assert o.POOL_FUSED_HITS[0] == hits + 1
    (yf, gxf, gwf, gbf), (yu, gxu, gwu, gbu) = outs
    assert torch.equal(yf, yu)
    t = tol(dtype)
    assert relerr(gxf, gxu) < (1e-5 if dtype == F32 else 1e-2)
    if affine:
        assert relerr(gwf, gwu) < 1e-4 and relerr(gbf, gbu) < 1e-4
    x64, w64, b64 = leaf64(x, w if affine else None, b if affine else None)
    z64 = F.relu(F.instance_norm(x64, None, None, w64, b64, True, 0.1, EPS))
    y64 = F.max_pool2d(z64, 3, 2, 1)
    y64.backward(gy.double())
    errs = dict(y=relerr(yf, y64))
    assert errs["y"] < t * (1 if dtype == F32 else 2)
    if dtype == F32:
        cnt, mx = window_max_count(z64.detach().float())
        assert bool(((cnt == 1) | (mx == 0)).all())
        errs["dx"] = relerr(gxf, x64.grad)
        assert errs["dx"] < 20 * t
        if affine:
            errs.update(dw=relerr(gwf, w64.grad), db=relerr(gbf, b64.grad))
            assert errs["dw"] < 10 * t and errs["db"] < 10 * t
    print(name, dtype, affine, errs)


@pytest.mark.parametrize("name,dtype", ROW_CASES, ids=ROW_IDS)
def test_line_independent_kernels_equal_the_image_by_image_run(name, dtype):
    """add, ReLU (forward and its gate) and the apply pass of an eval-mode BatchNorm (+ReLU, + residual) write an output line
    that does not depend on which workgroup wrote it: the batched launch (several lines per workgroup) is bit-identical with
    B launches of one image (one line per workgroup).  Bilinear and max pool: test_bilinear_many_lines, test_maxpool_many_lines."""
    o = ops()
    shape = lg.ROW_SHAPES[name]["shape"]
    B, C, H, W = shape
    a, b = gdev(rnd(*shape, seed=20), dtype), gdev(rnd(*shape, seed=21), dtype)
    gy = gdev(rnd(*shape, seed=22), dtype)
    w, bb = (torch.rand(C) + 0.5).to(DEV), (torch.randn(C) * 0.1).to(DEV)
    rm, rv = (torch.randn(C) * 0.1).to(DEV), (torch.rand(C) + 0.5).to(DEV)
    with torch.no_grad():
        s = o.add(a, b)
        assert torch.equal(s, per_image(o.add, a, b))
        assert relerr(s, a.double() + b.double()) < tol(dtype)
        assert torch.equal(o.relu(s), per_image(o.relu, s)) and torch.equal(o.relu(s), torch.relu(s))
        for relu in (False, True):
            bn = lambda xi, ri=None: o.batch_norm_act(xi, w, bb, rm, rv, training=False, relu=relu, res=ri)
            assert torch.equal(bn(a), per_image(bn, a))
            assert torch.equal(bn(a, b), per_image(bn, a, b))

    def bn_bwd(xi, gi):
        xi = xi.clone().requires_grad_(True)
        o.batch_norm_act(xi, w, bb, rm, rv, training=False, relu=True).backward(gi)
        return xi.grad
    assert torch.equal(bn_bwd(a, gy), per_image(bn_bwd, a, gy))


# =====================================================================================================================================
# 2. lines longer than one trip of the row threads
# =====================================================================================================================================
# Measured bounds (not inherited).  The source position of destination column ow is the fp32 product ow * (Wi - 1) / (Wo - 1), in the
# kernel as in ATen: its rounding error grows with the position (2^-24 x 350 ... 700 at the end of these lines), and with it the error of
# the two tap weights.  The op tests stop at 113 output columns, where tol() holds.  At these widths the kernel's output is 2.704e-5
# (351 -> 700) and 4.362e-5 (700 -> 351) of the maximum away from float64 -- and F.interpolate in float32 on the CPU, on the same
# inputs, is 2.704e-5 and 4.362e-5 away: the same arithmetic.  Bound: 4 x that measured reference error (the factor covers another,
# equally valid order of the fp32 operations).  The gradients (1.70e-5, 4.13e-5) stay inside the inherited 4 * tol().
BILINEAR_F32_Y = {("c8_f32", 351, 700): 4 * 2.704e-5, ("c8_f32", 700, 351): 4 * 4.362e-5}


@pytest.mark.parametrize("name", sorted(lg.TRIP_CASES))
def test_lines_longer_than_one_trip(name):
    """One full trip of 4 * rowthreads pixels followed by a partial one (clamped loads, masked tail; at 150 and 1100 pixels some
    row threads get no pixel of the last trip): BatchNorm (train, forward + backward, ReLU), InstanceNorm and the bilinear
    resize along W in both directions, against float64."""
    o = ops()
    c = lg.TRIP_CASES[name]
    shape, dtype = c["shape"], c["dtype"]
    B, C, H, W = shape
    t = tol(dtype)
    w, b = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    gy = rnd(*shape, seed=3, dtype=dtype)
    for relu in (False, True):
        x = rnd(*shape, seed=1, scale=3.0, shift=1.5, dtype=dtype)
        if relu:
            x = settle(x, dtype, norm_pre(w, b, None, (0, 2, 3)))
        x64, w64, b64 = leaf64(x, w, b)
        rm64, rv64 = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        y64 = F.batch_norm(x64, rm64, rv64, w64, b64, True, 0.1, EPS)
        y64 = F.relu(y64) if relu else y64
        y64.backward(gy.double())
        xd, wd, bd = dev(x, dtype), w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        yd = o.batch_norm_act(xd, wd, bd, rm, rv, training=True, relu=relu)
        yd.backward(gdev(gy, dtype))
        errs = dict(y=relerr(yd, y64), rm=relerr(rm, rm64), rv=relerr(rv, rv64), dx=relerr(xd.grad, x64.grad),
                    dw=relerr(wd.grad, w64.grad), db=relerr(bd.grad, b64.grad))
        print(name, "bn relu", relu, errs)
        assert errs["y"] < t and errs["rm"] < 1e-5 and errs["rv"] < 1e-5 + (0 if dtype == F32 else 1e-2)
        assert errs["dx"] < 10 * t and errs["dw"] < 10 * t and errs["db"] < 10 * t
    # InstanceNorm (+ReLU)
    x = settle(rnd(*shape, seed=4, scale=50.0, shift=120.0, dtype=dtype), dtype, norm_pre(w, b, None, (2, 3)))
    x64, w64, b64 = leaf64(x, w, b)
    y64 = F.relu(F.instance_norm(x64, None, None, w64, b64, True, 0.1, EPS))
    y64.backward(gy.double())
    xd, wd, bd = dev(x, dtype), w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    yd = o.instance_norm_act(xd, wd, bd, relu=True)
    yd.backward(gdev(gy, dtype))
    errs = dict(y=relerr(yd, y64), dx=relerr(xd.grad, x64.grad), dw=relerr(wd.grad, w64.grad), db=relerr(bd.grad, b64.grad))
    print(name, "in", errs)
    assert errs["y"] < t * (1 if dtype == F32 else 2) and errs["dx"] < 20 * t and errs["dw"] < 10 * t and errs["db"] < 10 * t
    # bilinear along W: up to W output pixels per line (forward trips), down from W input pixels per line (backward trips)
    figures = []
    for (wi, wo) in ((W // 2 + 1, W), (W, W // 2 + 1)):
        xs = rnd(B, C, H, wi, seed=13, dtype=dtype)
        size = (H + 1, wo)
        g2 = rnd(B, C, *size, seed=15, dtype=dtype)
        (x64,) = leaf64(xs)
        y64 = orc.upsample_bilinear_ac(x64, size)
        y64.backward(g2.double())
        yd, gx = _bilinear(o, xs, size, dtype, g2)
        errs = dict(y=relerr(yd, y64), dx=relerr(gx, x64.grad))
        print(name, "bilinear", wi, wo, errs)
        figures.append((wi, wo, errs))
    for wi, wo, errs in figures:
        assert errs["y"] < BILINEAR_F32_Y.get((name, wi, wo), t), (wi, wo, errs)
        assert errs["dx"] < 4 * t, (wi, wo, errs)


# =====================================================================================================================================
# 3. depthwise 3x3 with multi-row strips
# =====================================================================================================================================
DW_PARAMS = [(n, d, s, dil) for n in lg.DW_CASES for d in lg.DW_CASES[n]["dtypes"] for s in (1, 2) for dil in (1, 2)
             if not (n == "c960_f32_tall" and (s, dil) != (2, 1))]


@pytest.mark.parametrize("name,dtype,stride,dil", DW_PARAMS, ids=["%s-%s-s%d-d%d" % (n, dname(d), s, dl) for n, d, s, dl in DW_PARAMS])
def test_dwconv_multi_row_strips_vs_fp64(name, dtype, stride, dil):
    """dw_fwd_kernel / dw_dgrad_kernel / dw_wgrad_kernel with strips of several rows (a shorter last strip; stride 2 and dilation 2
    across strip boundaries; Cp > C) and dw_wgrad_reduce_kernel over B * strips slabs, as _case of test_depthwise_gpu.py."""
    o = ops()
    c = lg.DW_CASES[name]
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, C, H, W, generator=g).to(dtype)
    w = torch.randn(C, 1, 3, 3, generator=g) / 3.0
    gy = torch.randn(B, C, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=g).to(dtype)
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    y = o.depthwise_conv2d(xd, wd, None, stride, dil, dil)
    y.backward(gy.to(DEV).contiguous(memory_format=CL))
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, stride, dil, dil, C)
    y64.backward(gy.double())
    t = DW_TOL[dtype]
    errs = dict(y=relerr(y, y64), dx=relerr(xd.grad, x64.grad), dw=relerr(wd.grad, w64.grad))
    print(name, dtype, stride, dil, errs)
    assert tuple(y.shape) == tuple(y64.shape) and y.dtype == dtype
    assert errs["y"] < t and errs["dx"] < t and errs["dw"] < t


def test_dwconv_dgrad_pad_channels_zero_in_multi_row_strips():
    """Cp = 16 > C = 12 through the C ABI with garbage in dy's pad channels: the pad channels of dx come out zero in every row of
    a three-row strip (test_dgrad_pad_channels_are_zero at one row per strip)."""
    from mrfp_amd import _lib
    c = lg.DW_CASES["c12_padded"]
    B, C, H, W, Cp = c["B"], c["C"], c["H"], c["W"], 16
    g = torch.Generator().manual_seed(8)
    dy = torch.randn(B, H, W, Cp, generator=g).to(DEV, BF16)
    w = torch.randn(C, 1, 3, 3, generator=g).to(DEV)
    dx = torch.full((B, H, W, Cp), 7.0, device=DEV, dtype=BF16)
    _lib.call("mrfp_dwconv_dgrad", dy.data_ptr(), w.data_ptr(), dx.data_ptr(), _lib.BF16, B, H, W, Cp, C, H, W, 1, 1, _lib.stream())
    assert (dx[..., C:] == 0).all()
    ref = F.conv_transpose2d(dy[..., :C].permute(0, 3, 1, 2).double().cpu(), w.double().cpu(), None, 1, 1, 0, C)
    assert relerr(dx[..., :C].permute(0, 3, 1, 2), ref) < DW_TOL[BF16]


@pytest.mark.parametrize("dtype", [BF16, F16], ids=dname)
def test_dwconv_fused_statistics_with_fewer_slabs_than_rows(dtype):
    """test_fused_statistics_equal_a_separate_pass where the statistics layout is [B][nslab] with nslab = 75 < Ho = 150 and
    bn_finalize sums B * nslab = 1200 rows: fused == separate pass (both through mrfp_bn_finalize), and mean / variance against
    float64 of the stored y."""
    from mrfp_amd import _lib
    o = ops()
    name, stride = lg.DW_STATS_CASE
    c = lg.DW_CASES[name]
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, C, H, W, generator=g).to(DEV, dtype).contiguous(memory_format=CL)
    w = (torch.randn(C, 1, 3, 3, generator=g) / 3).to(DEV)
    y = o.depthwise_conv2d(x, w, None, stride, 1, 1)
    st = y._mrfp_colstats
    want = c["s%d" % stride]["fwd"][0]
    assert st.elements == B * y.shape[2] * y.shape[3] and st.final_count == B * want and st.final.numel() == st.final_count * 2 * C

    def finalize(ws, nb, nslab):
        out = torch.empty(4 * C, device=DEV)
        _lib.call("mrfp_bn_finalize", ws.data_ptr(), nb, nslab, st.elements, C, None, None, 1e-5, 0.0, None, None,
                  out[:C].data_ptr(), out[C:2 * C].data_ptr(), out[2 * C:3 * C].data_ptr(), out[3 * C:].data_ptr(), _lib.stream())
        return out[:2 * C].cpu()
    fused = finalize(st.final, 1, st.final_count)
    nslab, ws = o._stats_fwd(y, None)
    sep = finalize(ws, B, nslab)
    torch.testing.assert_close(fused, sep, rtol=2e-5, atol=1e-6)
    y64 = y.double().cpu()
    mean64 = y64.mean((0, 2, 3))
    invstd64 = 1.0 / (y64.var((0, 2, 3), unbiased=False) + 1e-5).sqrt()
    torch.testing.assert_close(fused[:C].double(), mean64, rtol=2e-5, atol=1e-6)
    torch.testing.assert_close(fused[C:].double(), invstd64, rtol=2e-5, atol=1e-6)


# =====================================================================================================================================
# 4. loss and evaluation kernels above the grid cap
# =====================================================================================================================================
def _labels(B, H, W, C, g):
    y = torch.randint(0, C, (B, H, W), generator=g)
    r = torch.rand(B, H, W, generator=g)
    y[r < 0.1] = 255
    odd = (r >= 0.1) & (r < 0.1002)                                  # a few labels outside the classes that are not 255
    y[odd] = torch.randint(C, 255, (int(odd.sum()),), generator=g)
    assert int(odd.sum()) > 10
    return y


def _mask_invalid(y, C):
    return torch.where((y >= 0) & (y < C), y, torch.full_like(y, 255))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
def test_cross_entropy_and_hist_above_the_grid_cap(dtype):
    """525 625 pixels on 2048 workgroups of 256: the grid-stride loops of ce_fwd / ce_bwd / argmax_hist take a second pixel in 1 337
    threads, ce_finalize sums 2048 partial rows.  About 10 % of the labels are 255 and a few lie in [19, 254]: the kernels treat
    every label outside 0..C-1 as ignored (torch raises for them), so the float64 reference maps them to 255 first.  Loss and
    gradient bounds of test_cross_entropy_and_hist; histogram and predictions exact."""
    o = ops()
    c = lg.CE_CASE
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    x = rnd(B, C, H, W, seed=22, scale=3.0, dtype=dtype)
    y = _labels(B, H, W, C, torch.Generator().manual_seed(23))
    (x64,) = leaf64(x)
    l64 = F.cross_entropy(x64, _mask_invalid(y, C), ignore_index=255)
    (l64 * 1.7).backward()
    xd = dev(x, dtype)
    ld = o.cross_entropy(xd, y.to(DEV), 255)
    (ld * 1.7).backward()
    errs = dict(loss=abs(ld.item() - l64.item()) / abs(l64.item()), dx=relerr(xd.grad, x64.grad))
    print(dtype, errs)
    assert errs["loss"] < 1e-5
    assert errs["dx"] < (1e-5 if dtype == F32 else 1e-2)
    hist, pred = o.argmax_hist(xd, y.to(DEV), want_pred=True)
    ref_pred = x.numpy().argmax(1)
    np.testing.assert_array_equal(pred.cpu().numpy(), ref_pred)
    np.testing.assert_array_equal(hist.cpu().numpy(), orc.fast_hist(ref_pred.flatten(), y.numpy().flatten(), C))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
def test_fused_upsample_cross_entropy_above_the_grid_cap(dtype):
    """upsample + cross entropy fused from [1, 19 -> 32 padded, 182, 182] to 725 x 725 (upsample_ce_fwd / _bwd above the cap, the
    bilinear backward behind it): bounds of test_fused_upsample_cross_entropy, pad-channel gradients exactly zero.  Labels as in
    test_cross_entropy_and_hist_above_the_grid_cap."""
    o = ops()
    c = lg.UPCE_CASE
    B, C, ld_, Hi, Wi, H, W = c["B"], c["C"], c["ld"], c["Hi"], c["Wi"], c["H"], c["W"]
    g = torch.Generator().manual_seed(31)
    x = (torch.randn(B, C, Hi, Wi, generator=g) * 2).to(dtype).float()
    y = _labels(B, H, W, C, g)
    (x64,) = leaf64(x)
    l64 = F.cross_entropy(orc.upsample_bilinear_ac(x64, (H, W)), _mask_invalid(y, C), ignore_index=255)
    (l64 * 0.7).backward()
    P = torch.zeros(B, ld_, Hi, Wi)
    P[:, :C] = x
    Pd = P.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)
    ld = o.upsample_cross_entropy(Pd, y.to(DEV), (H, W), C, 255)
    (ld * 0.7).backward()
    errs = dict(loss=abs(ld.item() - l64.item()) / abs(l64.item()), dx=relerr(Pd.grad[:, :C], x64.grad))
    print(dtype, errs)
    assert errs["loss"] < (1e-5 if dtype == F32 else 2e-3)
    assert errs["dx"] < (2e-5 if dtype == F32 else 1.5e-2)
    assert float(Pd.grad[:, C:].abs().max()) == 0.0


def test_acc_argmax_hist_above_the_grid_cap():
    """acc_argmax_hist (csrc/eval.hip, the same 2048-workgroup cap) at 525 625 pixels and 19 classes against numpy, inputs as
    test_acc_argmax_hist_matches_numpy builds them (exact ties, labels 255 / NC / -1, two uncovered pixels), vectorised."""
    o = ops()
    NC, B, H, W = 19, 1, lg.CE_CASE["H"], lg.CE_CASE["W"]
    g = torch.Generator().manual_seed(NC + H)
    acc = torch.rand(B, H, W, NC, generator=g)
    flat = acc.view(-1, NC)
    n = flat.shape[0]
    p = torch.arange(0, n, 3)                     # exact ties: the maximum is duplicated at a second (sometimes third) class
    mx = flat[p].max(1).values
    flat[p, torch.randint(0, NC, (p.numel(),), generator=g)] = mx
    flat[p[::2], NC - 1] = mx[::2]
    flat[4] = 0.25                                # all classes equal: class 0 wins
    label = torch.randint(0, NC, (B, H, W), generator=g)
    r = torch.rand(B, H, W, generator=g)
    label[r < 0.1] = 255
    label[(r >= 0.1) & (r < 0.2)] = NC
    label[(r >= 0.2) & (r < 0.25)] = -1
    cnt = torch.ones(B, H, W)
    cnt.view(-1)[5] = 0
    cnt.view(-1)[n - 3] = 0                       # (a pixel only the second trip of the grid-stride loop reaches)
    accd, cntd = acc.to(DEV), cnt.to(DEV)
    unc = torch.zeros(1, dtype=torch.int64, device=DEV)
    hist0 = torch.arange(NC * NC, dtype=torch.int64).reshape(NC, NC)
    hist, pred = o.acc_argmax_hist(accd, cntd, label.to(DEV), hist0.to(DEV), want_pred=True, uncovered=unc)
    want_hist, want_pred = etc.hist_from_acc(accd, label, NC)
    assert np.array_equal(pred.cpu().numpy().astype(np.int64), want_pred)
    assert np.array_equal(hist.cpu().numpy(), want_hist + hist0.numpy())
    assert int(unc.item()) == 2
