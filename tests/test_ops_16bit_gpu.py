"""The 16-bit instances of the row operators (csrc/stats.hip, csrc/affine.hip, csrc/resize_pool.hip through mrfp_amd/ops.py) held
to PER-ELEMENT bounds against float64, in bf16 and f16.

Metric, constants, designed upstream gradients, settled gates and the cases are those of tests/rounding_model_common.py;
tests/test_rounding_model_cpu.py proves on the host that the honest fp32 emulation passes them and that every planted defect (a
backward that ignores the statistics, a line lost from a reduction, a neighbour's coefficients, an unwritten channel vector, a
shifted gate, a double rounding, a lost multiplicity) fails them.  All inputs (x, res, addend, gy) are rounded to T before either
side sees them; the reference is torch in float64 on the CPU.  Each test prints its largest scaled value per output (-s).

The 16-bit instances are code of their own: VEC = 8 (another lane-to-channel map than fp32), the sign-mask path of the residual
tail (mrfp_affine_fwd_relu_mask / mrfp_stats_bwd_mask / mrfp_affine_bwd_mask), the gated-gradient protocol of a plain BatchNorm.
"""
import pytest
import torch
import torch.nn.functional as F

import rounding_model_common as rm
from rounding_model_common import BF16, F16, C_F32, dname, sid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
TYPES = [BF16, F16]


def ops():
    from mrfp_amd import ops as o
    return o


def dev(x, T, grad=True):
    return x.to(DEV, T).contiguous(memory_format=CL).requires_grad_(grad)


def gdev(g, T):
    return g.to(DEV, T).contiguous(memory_format=CL)


def pdev(p):
    return p.to(DEV).requires_grad_(True) if p is not None else None


def hooked(fn):
    """-> (result of fn(), names of the library entry points it called)."""
    from mrfp_amd import _lib
    names = []
    _lib.HOOK[0] = lambda name, args: names.append(name)
    try:
        return fn(), names
    finally:
        _lib.HOOK[0] = None


def check(op, label, outs, ref, T):
    """Every output of `outs` against the reference under C_F32[op]; prints the scaled values first."""
    assert set(outs) == set(ref["mag"]), (label, sorted(outs), sorted(ref["mag"]))
    for k, v in outs.items():
        assert v.dtype == (torch.float32 if k in ("dw", "db", "rm", "rv") else T), (label, k, v.dtype)
    w = rm.worst({k: v.detach().cpu() for k, v in outs.items()}, ref, T)
    print("%s %s %s scaled %s (bound %d)" % (op, label, dname(T), {k: round(v, 3) for k, v in w.items()}, C_F32[op]))
    for k, v in w.items():
        assert v < C_F32[op], (label, k, v)
    return w


def run_bn(o, c, T, **kw):
    """batch_norm_act forward and backward on the device -> outputs by the reference's names."""
    xd, rd = dev(c["x"], T), (dev(c["res"], T) if c.get("res") is not None else None)
    wd, bd = pdev(c["w"]), pdev(c["b"])
    rm_d, rv_d = c["rm"].to(DEV), c["rv"].to(DEV)

    def run():
        if c["act"] == "relu6":
            y = o.local_batch_norm_act(xd, wd, bd, rm_d, rv_d, training=True, act="relu6")
        else:
            y = o.batch_norm_act(xd, wd, bd, rm_d, rv_d, relu=c["act"] == "relu", res=rd, **kw)
        y.backward(gdev(c["gy"], T))
        return y
    y, names = hooked(run)
    outs = dict(y=y.detach(), dx=xd.grad, dw=wd.grad, db=bd.grad)
    if rd is not None:
        outs["dres"] = rd.grad
    if kw.get("training", True):
        outs.update(rm=rm_d, rv=rv_d)
    return outs, names


# =====================================================================================================================================
# 1. BatchNorm, training
# =====================================================================================================================================
@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("relu,res", rm.BN_COMBOS, ids=["plain", "relu", "res", "relu_res"])
@pytest.mark.parametrize("shape", rm.BN_SHAPES, ids=sid)
def test_batch_norm_act_train(shape, relu, res, T):
    """y, dx, dres, dweight, dbias and both running statistics.  The residual ReLU tail at C % 8 == 0 runs with the 1-bit sign mask
    and with ops.SIGN_MASK off (re-reading y), each against float64; at C = 19 / 12 there is no mask and it reads y."""
    o = ops()
    C = shape[1]
    c = rm.bn_case(shape, T, relu, res)
    ref = rm.norm_reference("bn", c["x"], c["w"], c["b"], c["gy"], res=c["res"], act=c["act"], rm=c["rm"], rv=c["rv"])
    assert rm.stat_share(ref) >= 0.25
    masked = relu and res and C % 8 == 0
    for use_mask in ((True, False) if masked else (True,)):
        o.SIGN_MASK[0] = use_mask
        try:
            outs, names = run_bn(o, c, T, training=True)
        finally:
            o.SIGN_MASK[0] = True
        want = masked and use_mask
        assert ("mrfp_stats_bwd_mask" in names) == want and ("mrfp_affine_bwd_mask" in names) == want, names
        assert ("mrfp_affine_fwd_relu_mask" in names) == want, names
        check("batch_norm", "%s relu=%d res=%d mask=%d" % (sid(shape), relu, res, want), outs, ref, T)


@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("shape", [s for s in rm.BN_SHAPES if s[1] % 8 == 0], ids=sid)
def test_plain_batch_norm_takes_the_gated_gradient_of_a_residual_tail(shape, T):
    """A plain BatchNorm (no ReLU, no residual, 16 bit, C % 8 == 0) feeding a residual tail: the tail hands it the UNMASKED gradient
    with its sign mask, and the BatchNorm's two backward passes gate it while they read it (ops.GATED_BN).  The tail against
    float64 with the device's stored output of the first layer as its residual; the first layer's dx, dweight, dbias against
    float64 of gy * [tail > 0]."""
    o = ops()
    B, C, H, W = shape
    c1 = rm.bn_case(shape, T, False, False)
    x1d, w1d, b1d = dev(c1["x"], T), pdev(c1["w"]), pdev(c1["b"])
    y1 = o.batch_norm_act(x1d, w1d, b1d, c1["rm"].to(DEV), c1["rv"].to(DEV), training=True)
    from mrfp_amd import skipgrad
    assert skipgrad.alias_cell(y1) is not None
    y1h = y1.detach().float().cpu().contiguous()
    c2 = rm.gated_tail_case(shape, T, y1h)
    gy = c1["gy"]
    ref2 = rm.norm_reference("bn", c2["x"], c2["w"], c2["b"], gy, res=y1h, act="relu", rm=c2["rm"], rv=c2["rv"])
    x2d, w2d, b2d = dev(c2["x"], T), pdev(c2["w"]), pdev(c2["b"])
    rm2, rv2 = c2["rm"].to(DEV), c2["rv"].to(DEV)
    hits = o.GATED_BN_HITS[0]

    def run():
        y2 = o.batch_norm_act(x2d, w2d, b2d, rm2, rv2, training=True, relu=True, res=y1)
        y2.backward(gdev(gy, T))
        return y2
    y2, names = hooked(run)
    assert o.GATED_BN_HITS[0] == hits + 1 and names.count("mrfp_stats_bwd_mask") == 2, names
    ref2.pop("dres"), ref2["mag"].pop("dres")                 # (never written: it travels as gy + mask)
    check("batch_norm", "%s tail" % sid(shape), dict(y=y2.detach(), dx=x2d.grad, dw=w2d.grad, db=b2d.grad, rm=rm2, rv=rv2), ref2, T)
    gated = rm.norm_model("bn", c2["x"], c2["w"], c2["b"], gy, res=y1h, act="relu")["dres"].float()     # gy * [tail > 0]: exact in T
    ref1 = rm.norm_reference("bn", c1["x"], c1["w"], c1["b"], gated)
    assert rm.stat_share(ref1) >= 0.25
    for k in ("y", "rm", "rv"):
        ref1["mag"].pop(k, None)
    check("batch_norm", "%s gated" % sid(shape), dict(dx=x1d.grad, dw=w1d.grad, db=b1d.grad), ref1, T)


# =====================================================================================================================================
# 2. BatchNorm, eval coefficients; 3. BatchNorm + ReLU6
# =====================================================================================================================================
@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", rm.BN_SHAPES[:4] + rm.BN_SHAPES[5:6], ids=sid)
def test_batch_norm_act_eval(shape, relu, T):
    """training=False: the running statistics are constants (bn_eval_coef_kernel); forward, and backward of x, weight, bias."""
    o = ops()
    c = rm.bn_eval_case(shape, T, relu)
    ref = rm.norm_reference("bn", c["x"], c["w"], c["b"], c["gy"], act=c["act"], rm=c["rm"], rv=c["rv"], training=False)
    outs, _ = run_bn(o, c, T, training=False)
    check("batch_norm_eval", "%s relu=%d" % (sid(shape), relu), outs, ref, T)


@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("shape", rm.BN_SHAPES[:4] + rm.BN_SHAPES[5:6], ids=sid)
def test_local_batch_norm_relu6(shape, T):
    """local_batch_norm_act(act="relu6"): both gates (0 and 6) settled; the pass mask gates dy inside the masked kernel pair at
    C % 8 == 0 and through mrfp_mask_gate at C = 19."""
    o = ops()
    C = shape[1]
    c = rm.bn_case(shape, T, False, False, act="relu6")
    ref = rm.norm_reference("bn", c["x"], c["w"], c["b"], c["gy"], act="relu6", rm=c["rm"], rv=c["rv"])
    assert rm.stat_share(ref) >= 0.25
    outs, names = run_bn(o, c, T)
    assert ("mrfp_stats_bwd_mask" in names) == (C % 8 == 0) and ("mrfp_mask_gate" in names) == (C % 8 != 0), names
    y = outs["y"].float()
    assert bool((y == 6).any()) and bool((y == 0).any())
    check("batch_norm_relu6", sid(shape), outs, ref, T)


# =====================================================================================================================================
# 4. InstanceNorm
# =====================================================================================================================================
def run_in(o, c, T, xd=None, **kw):
    xd = dev(c["x"], T) if xd is None else xd
    wd, bd = pdev(c["w"]), pdev(c["b"])
    y = o.instance_norm_act(xd, wd, bd, relu=c["act"] == "relu", **kw)
    return xd, wd, bd, y


@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("case", rm.IN_CASES, ids=rm.in_case_id)
def test_instance_norm_act(case, T):
    """Per-(image, channel) statistics at the stem's magnitudes (scale 50, shift 120: a mean of tens of standard deviations); affine
    and not, ReLU and not (without the affine part the gate is recomputed from x*A + S with S = -m*A alone)."""
    o = ops()
    shape, affine, relu = case
    c = rm.in_case(shape, T, affine, relu)
    ref = rm.norm_reference("in", c["x"], c["w"], c["b"], c["gy"], act=c["act"])
    assert rm.stat_share(ref) >= 0.25
    xd, wd, bd, y = run_in(o, c, T)
    y.backward(gdev(c["gy"], T))
    outs = dict(y=y.detach(), dx=xd.grad)
    if affine:
        outs.update(dw=wd.grad, db=bd.grad)
    check("instance_norm", "%s affine=%d relu=%d" % (sid(shape), affine, relu), outs, ref, T)


@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", [rm.IN_SHAPES[1], rm.IN_SHAPES[2], rm.IN_SHAPES[5]], ids=sid)
def test_instance_norm_emits_the_plane_sums_of_its_output_for_the_next_one(shape, relu, T):
    """emit_stats=True: the apply pass also writes the partial plane sums of its STORED output and a second instance_norm_act runs
    without a statistics pass of its own.  The reference of the second operator takes the device's stored y of the first as its
    input, in float64."""
    o = ops()
    c = rm.in_case(shape, T, True, relu)
    ref = rm.norm_reference("in", c["x"], c["w"], c["b"], c["gy"], act=c["act"])
    xd, wd, bd, y1 = run_in(o, c, T, emit_stats=True)
    y1.retain_grad()
    y1h = y1.detach().float().cpu().contiguous()
    check("instance_norm", "%s first" % sid(shape), dict(y=y1.detach()), dict(y=ref["y"], mag=dict(y=ref["mag"]["y"])), T)
    w2, b2, _, _ = rm.bn_params(shape[1], seed=3)
    gy2 = rm.designed_gy("in", y1h, T, seed=9)
    ref2 = rm.norm_reference("in", y1h, w2, b2, gy2)
    assert rm.stat_share(ref2) >= 0.25
    w2d, b2d = pdev(w2), pdev(b2)
    hits = o.PLANE_STATS_HITS[0]

    def run():
        y2 = o.instance_norm_act(y1, w2d, b2d)
        y2.backward(gdev(gy2, T))
        return y2
    y2, names = hooked(run)
    assert o.PLANE_STATS_HITS[0] == hits + 1 and "mrfp_stats_fwd" not in names, names
    check("instance_norm", "%s second" % sid(shape), dict(y=y2.detach(), dx=y1.grad, dw=w2d.grad, db=b2d.grad), ref2, T)


# =====================================================================================================================================
# 5. NP+
# =====================================================================================================================================
@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("shape", rm.NP_SHAPES, ids=sid)
def test_np_plus(shape, with_res, T):
    """B in {2, 4, 16} (sigma over the batch needs B >= 2); reference oracle.mrfp_oracle.np_plus in float64."""
    o = ops()
    c = rm.np_case(shape, T, with_res)
    ref = rm.np_reference(**c)
    assert rm.stat_share(ref) >= 0.25
    xd, rd = dev(c["x"], T), (dev(c["res"], T) if with_res else None)
    y = o.np_plus(xd, c["alpha"].to(DEV), c["noise"].to(DEV), res=rd)
    y.backward(gdev(c["gy"], T))
    outs = dict(y=y.detach(), dx=xd.grad)
    if with_res:
        outs["dres"] = rd.grad
    check("np_plus", "%s res=%d" % (sid(shape), with_res), outs, ref, T)


# =====================================================================================================================================
# 6. nearest resize -> BatchNorm -> ReLU
# =====================================================================================================================================
@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("name", sorted(rm.RESIZE_CASES))
def test_batch_norm_relu_behind_a_nearest_resize(name, T):
    """Statistics and apply pass through the index tables, the input gradient through the inverse tables with the pixel
    multiplicity n on the statistic terms: up 1.205 on 12 x 12 (vector and scalar path), down 0.798 on 20 x 20 (pixels nobody
    reads: n = 0, dx exactly 0), a size= plan with unequal factors."""
    o = ops()
    c = rm.resize_case(name, T)
    shape, rs = rm.RESIZE_CASES[name]
    ref = rm.norm_reference("bn", c["x"], c["w"], c["b"], c["gy"], act="relu", tabs=c["tabs"], **rs)
    assert rm.stat_share(ref) >= 0.25
    xd, wd, bd = dev(c["x"], T), pdev(c["w"]), pdev(c["b"])
    plan = o.nearest_plan(shape[2], shape[3], device=DEV, **rs)
    assert (plan.Ho, plan.Wo) == tuple(ref["y"].shape[2:])
    y = o.batch_norm_act(xd, wd, bd, None, None, training=True, relu=True, plan=plan)
    y.backward(gdev(c["gy"], T))
    check("batch_norm_resize", name, dict(y=y.detach(), dx=xd.grad, dw=wd.grad, db=bd.grad), ref, T)


# =====================================================================================================================================
# 7. bilinear; 8. max pool; 9. InstanceNorm -> ReLU -> max pool; 10. global average pool, add, ReLU, channel scale
# =====================================================================================================================================
@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("name", sorted(rm.BILINEAR_CASES))
def test_upsample_bilinear(name, with_add, T):
    """align_corners resize (+ addend): up 2x and 4x (the windowed backward), odd factors, a 1 x 1 source (the broadcast form without
    an addend), identity size, a downsample, 19 channels of a 24- / 32-channel padded buffer (pad-channel gradients exactly zero).
    Reference oracle.mrfp_oracle.upsample_bilinear_ac in float64."""
    o = ops()
    c = rm.bilinear_case(name, T)
    if not with_add:
        c["addend"] = None
    ref = rm.bilinear_model(**c)
    xd = dev(c["x"], T)
    ad = dev(c["addend"], T) if with_add else None
    y = o.upsample_bilinear(xd, c["size"], addend=ad, channels=c["channels"])
    y.backward(gdev(c["gy"], T))
    outs = dict(y=y.detach(), dx=xd.grad)
    if with_add:
        outs["dadd"] = ad.grad
    check("bilinear", "%s add=%d" % (name, with_add), outs, ref, T)
    if c["channels"] is not None:
        assert float(xd.grad[:, c["channels"]:].abs().max()) == 0.0


@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("shape", rm.POOL_SHAPES, ids=sid)
def test_max_pool_3x3_s2(shape, T):
    """Tie-free inputs: the forward is bit-identical to the reference rounded to T, the backward (up to four windows route to a
    pixel) has a per-element bound."""
    o = ops()
    c = rm.pool_case(shape, T)
    ref = rm.max_pool_model(**c)
    xd = dev(c["x"], T)
    y = o.max_pool_3x3_s2(xd)
    y.backward(gdev(c["gy"], T))
    assert torch.equal(y.detach().cpu(), ref["y"].to(T))
    check("max_pool", sid(shape), dict(y=y.detach(), dx=xd.grad), ref, T)


@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two_operators"])
@pytest.mark.parametrize("case", rm.IN_POOL_CASES, ids=lambda c: "%s-%s" % (sid(c[0]), "affine" if c[1] else "plain"))
def test_instance_norm_relu_pool(case, fused, T):
    """InstanceNorm -> ReLU -> max pool, fused (the normalised tensor never stored) and as two operators (ops.POOL_FUSED off), each
    against float64: y, dx, dweight, dbias.  Inputs keep every window's arg-max through the rounding of the normalised values
    (asserted).  The pool's input gradient is rounded to T between the two stages of the backward -- stored by the two-operator
    route, rounded in registers by the fused kernels, which keep that contract on purpose -- and the float64 reference rounds
    there too (rounding_model_common.pool_norm_model).  The two-operator route is also held stage by stage: the stored
    normalised tensor, the pool on it (exact), the stored gradient of the pool where the ReLU passes it, and the
    normalisation's backward of that stored gradient."""
    o = ops()
    shape, affine, _ = case
    c = rm.in_case(shape, T, affine, True, pool=True)
    x, w, b, gy = c["x"], c["w"], c["b"], c["gy"]
    inner = rm.norm_model("in", x, w, b, torch.zeros_like(x), act="relu")
    assert rm.window_gap_ok(inner["y"], T)
    ref = rm.pool_norm_model(x, w, b, gy, T=T)
    assert rm.stat_share(ref) >= 0.25
    xd, wd, bd = dev(x, T), pdev(w), pdev(b)
    label = "%s affine=%d fused=%d" % (sid(shape), affine, fused)
    grads = lambda: dict(dx=xd.grad, dw=wd.grad, db=bd.grad) if affine else dict(dx=xd.grad)
    if fused:
        hits = o.POOL_FUSED_HITS[0]
        y = o.instance_norm_relu_pool(xd, wd, bd)
        y.backward(gdev(gy, T))
        assert o.POOL_FUSED_HITS[0] == hits + 1
        check("instance_norm_relu_pool", label, dict(y=y.detach(), **grads()), ref, T)
        return
    seen, pool = [], o.max_pool_3x3_s2

    def recording_pool(z):
        z.retain_grad()
        seen.append(z)
        return pool(z)
    o.POOL_FUSED[0], o.max_pool_3x3_s2 = False, recording_pool
    try:
        y = o.instance_norm_relu_pool(xd, wd, bd)
        y.backward(gdev(gy, T))
    finally:
        o.POOL_FUSED[0], o.max_pool_3x3_s2 = True, pool
    (z,) = seen
    zh = z.detach().float().cpu().contiguous()
    check("instance_norm", label + " z", dict(y=z.detach()), dict(y=inner["y"], mag=dict(y=inner["mag"]["y"])), T)
    assert torch.equal(y.detach().float().cpu(), F.max_pool2d(zh, 3, 2, 1))
    check("instance_norm_relu_pool", label + " y", dict(y=y.detach()), dict(y=ref["y"], mag=dict(y=ref["mag"]["y"])), T)
    # the pool's stored input gradient, where the ReLU passes it (a window of zeros may route anywhere: gated off next)
    pr = rm.max_pool_model(inner["y"], gy)
    gate = (inner["y"] > 0).double()
    check("max_pool", label + " dz", dict(dx=(z.grad.float().cpu() * gate.float()).to(T)),
          dict(dx=pr["dx"] * gate, mag=dict(dx=pr["mag"]["dx"] * gate)), T)
    ref2 = rm.norm_reference("in", x, w, b, z.grad.detach().float().cpu().contiguous(), act="relu")
    ref2["mag"].pop("y")
    check("instance_norm", label + " bwd", grads(), ref2, T)


@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("shape", rm.EW_SHAPES, ids=sid)
def test_global_avg_pool_add_relu_channel_scale(shape, T):
    """global_avg_pool (fp32 plane mean rounded once to T; backward g / HW), add, relu(add(..)) with its gate, channel_scale
    forward and backward."""
    o = ops()
    c = rm.ew_case(shape, T)
    a, b, m, gp = c["a"], c["b"], c["m"], c["gp"]
    ref = rm.elementwise_model(**c)
    ad, bd_ = dev(a, T), dev(b, T)
    p = o.global_avg_pool(ad)
    p.backward(gp.to(DEV, T))
    outs = dict(gap=p.detach(), gap_dx=ad.grad.clone())
    ad.grad = None
    s = o.add(ad, bd_)
    r = o.relu(s)
    r.backward(gdev(b, T))
    outs.update(add=s.detach(), relu_add=r.detach())
    gate = ((a.double() + b.double()) > 0)
    want = torch.where(gate, b, torch.zeros_like(b)).to(T)
    assert torch.equal(ad.grad.cpu(), want) and torch.equal(bd_.grad.cpu(), want)
    a2 = dev(a, T)
    y = o.channel_scale(a2, m.to(DEV))
    y.backward(gdev(b, T))
    outs.update(cs=y.detach(), cs_dx=a2.grad)
    check("elementwise", sid(shape), outs, ref, T)
