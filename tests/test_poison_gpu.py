"""Every operator computes the same bits whatever its fresh memory held.

One parametrised test over CASES: the operator runs under the three fills of poison_common (0x00, 0xFF, 0x7B) with identical, seeded
inputs; the results a caller may read -- outputs, every .grad, returned counts, histograms and statistics -- must be equal bit for
bit, finite, the guard bands around every buffer intact, and the call sites recorded must include the ones the case declares
(tests/test_poison_cpu.py holds the table to the inventory of allocating functions).

Pad channels.  Where include/mrfp_hip.h or DESIGN.md promises zeros the physical tensor is compared, pad included: conv2d(phys_out=)
outputs (the packs' pad entries are zero), concat_upsample(pad_to=), pad_input_channels, the depthwise Cp > C buffers' logical slice
(depthwise_conv2d returns the logical channels only: the pad never reaches a caller), the low-resolution gradient of
upsample_bilinear(channels=) and of the fused losses (d(logits) pad channels zero).  Nothing else here has a pad.

Never compared: workspaces that are not returned, and the zero-storage dx stand-in of _SharedConv1x1Pair.backward.

Shapes: (a) ragged -- odd unequal H, W, a vector-width C and a scalar-path C; (b) many partials -- the shapes of
launch_geometry_common, which cross the launch caps; (c) Cphys > C and Nphys > N; (d) the convolution families by the cases of
test_conv_gpu / test_lowrank_skip_gpu the launch plan routes to them (the routing is read off mrfp_conv_stats_layout and
mrfp_conv_wgrad_plan, and pinned by test_poison_cpu.test_launch_plan_routes_the_chosen_cases_to_their_families: a negative block height is the weight-stationary 3x3 kernel, 128 / 192 / 256 / 384 the pointwise kernel, 240 /
288 / 1152 the long-K pointwise kernel, 64 / 96 the generic tiles; weight-gradient kernels 0 .. 4).  The row-window weight-gradient
kernels wg1 / wg3 and the 256 x 128 tile are 16-bit kernels that only the largest listed shapes reach: they run in bf16 only, wg3 at
B = 8 instead of 16 (the plan still routes it there).  The grouped weight-gradient launch (several problems of one geometry, deferred
through the gradient arena) runs in bf16 and fp32 in the flat_arena cases.

Inputs come from the builders the other tests use (rounding_model_common, loss_common, relaxed_common, eval_tta_common,
conv_exact_common, input_aug_common, synth); every case function returns pc.named(...) results, so a failure says which one differs.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

import poison_common as pc

CL = torch.channels_last
DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
IGNORE = 255

# allocating functions no single-GPU case can take: name -> reason ("host memory" / "more than one rank" are the admissible ones)
EXEMPT = {
    "ops.sync_bn_poll": "host memory: the pinned int32 word of the asynchronous read-back of the SYNC_BN flag",
}


class Case:
    """name; build() -> fn, called once OUTSIDE the poisoned block with seeded generators (identical inputs in the three runs);
    fn() -> the flat tuple of results; sites: the allocating functions the case claims to run."""

    def __init__(self, name, build, sites):
        self.name, self.build, self.sites = name, build, tuple(sites)

    def __repr__(self):
        return self.name


CASES = []


def case(name, sites):
    def deco(build):
        CASES.append(Case(name, build, sites))
        return build
    return deco


def dn(T):
    return {F32: "f32", BF16: "bf16", F16: "f16"}[T]


def sid(shape):
    return "x".join(str(int(v)) for v in shape)


def D(t, T=None):
    t = t.to(DEV) if T is None else t.to(DEV, T)
    return t.contiguous(memory_format=CL) if t.dim() == 4 else t.contiguous()


def act(shape, T, seed, **kw):
    import rounding_model_common as rm
    return D(rm.rnd(*shape, seed=seed, dtype=T, **kw), T)


def vec(n, seed, **kw):
    import rounding_model_common as rm
    return D(rm.rnd(n, seed=seed, **kw))


def leaf(t):
    return None if t is None else t.detach().clone().requires_grad_(True)


def grad(t):
    return None if t is None else t.grad


BASE = ("ops.empty_cl",)
STATS = ("ops._stats_ws",)

# (a) ragged; (b) many partials (launch_geometry_common: ROW_SHAPES two_lines_uneven / scalar_c19, TRIP_CASES c64_bf16)
RAGGED = [(3, 64, 17, 9), (2, 19, 7, 6), (1, 8, 1, 1)]


def _row_shapes():
    import launch_geometry_common as lg
    return RAGGED + [lg.ROW_SHAPES["two_lines_uneven"]["shape"], lg.ROW_SHAPES["scalar_c19"]["shape"], lg.TRIP_CASES["c64_bf16"]["shape"]]


ROW_SHAPES = _row_shapes()       # + (16, 8, 161, 5), (2, 19, 1100, 3), (2, 64, 3, 150)


# ---- normalisations ------------------------------------------------------------------------------------------------------------------
def _bn(shape, T, relu=False, res=False, relu6=False, training=True, rs=None):
    def build():
        from mrfp_amd import ops
        B, C, H, W = shape
        plan = ops.nearest_plan(H, W, device=DEV, **rs) if rs else None
        Ho, Wo = (plan.Ho, plan.Wo) if plan else (H, W)
        X, R, GY = act(shape, T, 1), (act((B, C, Ho, Wo), T, 2) if res else None), act((B, C, Ho, Wo), T, 3)
        Wt, Bt = vec(C, 4, scale=0.25, shift=1.0), vec(C, 5)

        def fn():
            x, r, w, b = leaf(X), leaf(R), leaf(Wt), leaf(Bt)
            rmean, rvar = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
            if relu6:
                y = ops.batch_norm_relu6(x, w, b, rmean, rvar, training=training)
            else:
                y = ops.batch_norm_act(x, w, b, rmean, rvar, training=training, relu=relu, res=r, plan=plan)
            y.backward(GY)
            return pc.named(y=y, dx=x.grad, dres=grad(r), dweight=w.grad, dbias=b.grad, running_mean=rmean, running_var=rvar)
        return fn
    return build


for _T in (BF16, F32, F16):
    for _s in ROW_SHAPES if _T != F16 else RAGGED[:2]:
        _fw = ("ops._BatchNormAct.forward", "ops._BatchNormAct.backward") + BASE + STATS
        CASES.append(Case("bn[%s-%s]" % (sid(_s), dn(_T)), _bn(_s, _T), _fw + ("ops._affine_fwd", "ops._affine_bwd")))
        CASES.append(Case("bn_relu[%s-%s]" % (sid(_s), dn(_T)), _bn(_s, _T, relu=True), _fw))
        CASES.append(Case("bn_relu_res[%s-%s]" % (sid(_s), dn(_T)), _bn(_s, _T, relu=True, res=True), _fw))     # sign mask where 16-bit, C % 8 == 0
        CASES.append(Case("bn_res[%s-%s]" % (sid(_s), dn(_T)), _bn(_s, _T, res=True), _fw))
        CASES.append(Case("bn_relu6[%s-%s]" % (sid(_s), dn(_T)), _bn(_s, _T, relu6=True), _fw))                 # pass mask: (n + 7) // 8 bytes
    CASES.append(Case("bn_eval_relu[%s-%s]" % (sid(RAGGED[0]), dn(_T)), _bn(RAGGED[0], _T, relu=True, training=False), _fw))


def _resize_cases():
    import launch_geometry_common as lg
    for name, c in lg.RESIZE_CASES.items():
        for T in (BF16, F32):
            CASES.append(Case("bn_relu_resize[%s-%s]" % (name, dn(T)), _bn(c["shape"], T, relu=True, rs=c["rs"]),
                              ("ops._BatchNormAct.forward", "ops._BatchNormAct.backward", "ops._affine_fwd", "ops._affine_bwd")))
    for T in (BF16, F32):
        CASES.append(Case("bn_relu_resize[ragged-%s]" % dn(T), _bn((2, 24, 13, 11), T, relu=True, rs=dict(scale=1.205)),
                          ("ops._affine_fwd", "ops._affine_bwd")))


_resize_cases()


def _inorm(shape, T, relu, affine=True):
    def build():
        from mrfp_amd import ops
        B, C, H, W = shape
        X, GY, R = act(shape, T, 11, shift=0.5), act(shape, T, 12), act(shape, T, 13)
        Wt, Bt = vec(C, 14, scale=0.25, shift=1.0), vec(C, 15)
        A, N = D(_rnd4((B, C, 1, 1), 16, 0.1, 1.0)), D(_rnd4((B, C, 1, 1), 17, 0.5, 0.0))

        def fn():
            x, r, w, b = leaf(X), leaf(R), (leaf(Wt) if affine else None), (leaf(Bt) if affine else None)
            y = ops.instance_norm_act(x, w, b, relu=relu, emit_stats=True)      # the apply pass also writes the plane sums NP+ takes
            z = ops.np_plus(y, A, N, res=r)
            z.backward(GY)
            return pc.named(y_instance_norm=y, z_np_plus=z, dx=x.grad, dres=r.grad, dweight=grad(w), dbias=grad(b))
        return fn
    return build


def _rnd4(shape, seed, scale, shift):
    import rounding_model_common as rm
    return rm.rnd(*shape, seed=seed, scale=scale, shift=shift)


def _np_plain(shape, T):
    def build():
        from mrfp_amd import ops
        B, C, H, W = shape
        X, GY = act(shape, T, 21, shift=0.5), act(shape, T, 22)
        A, N = D(_rnd4((B, C, 1, 1), 23, 0.1, 1.0)), D(_rnd4((B, C, 1, 1), 24, 0.5, 0.0))

        def fn():
            x = leaf(X)
            y = ops.np_plus(x, A, N)
            y.backward(GY)
            return pc.named(y=y, dx=x.grad)
        return fn
    return build


for _T in (BF16, F32):
    for _s in ROW_SHAPES:
        if _s[2] * _s[3] < 2:
            continue            # (one pixel per plane: the variance is 0 / 0)
        CASES.append(Case("instnorm_relu_np_res[%s-%s]" % (sid(_s), dn(_T)), _inorm(_s, _T, True),
                          ("ops._in_finalize", "ops._in_bwd_finalize", "ops._NPPlus.forward", "ops._NPPlus.backward", "ops._affine_fwd",
                           "ops._affine_bwd") + STATS))
        CASES.append(Case("np_plus[%s-%s]" % (sid(_s), dn(_T)), _np_plain(_s, _T), ("ops._NPPlus.forward", "ops._NPPlus.backward")))
    CASES.append(Case("instnorm_plain[%s-%s]" % (sid(RAGGED[0]), dn(_T)), _inorm(RAGGED[0], _T, False, affine=False), ("ops._in_finalize",)))


# ---- pools, resizes, element-wise, concatenations --------------------------------------------------------------------------------------
def _pool(shape, T, fused):
    def build():
        from mrfp_amd import ops
        B, C, H, W = shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        X, GY = act(shape, T, 31), act((B, C, Ho, Wo), T, 32)
        Wt, Bt = vec(C, 33, scale=0.25, shift=1.0), vec(C, 34)

        def fn():
            x, w, b = leaf(X), leaf(Wt), leaf(Bt)
            y = ops.instance_norm_relu_pool(x, w, b) if fused else ops.max_pool_3x3_s2(x)
            y.backward(GY)
            return pc.named(y=y, dx=x.grad, **(dict(dweight=w.grad, dbias=b.grad) if fused else {}))
        return fn
    return build


def _pool_cases():
    import launch_geometry_common as lg
    shapes = [(3, 64, 17, 9), (2, 19, 7, 6), (1, 8, 1, 1), lg.POOL_SHAPES["c8"]["shape"]]
    for T in (BF16, F32):
        for s in shapes:
            CASES.append(Case("max_pool[%s-%s]" % (sid(s), dn(T)), _pool(s, T, False), ("ops._MaxPool.forward", "ops._MaxPool.backward")))
            if s[2] * s[3] > 1:
                CASES.append(Case("instnorm_relu_pool[%s-%s]" % (sid(s), dn(T)), _pool(s, T, True),
                                  ("ops._InstanceNormReluPool.forward", "ops._InstanceNormReluPool.backward", "ops._in_finalize",
                                   "ops._in_bwd_finalize")))


_pool_cases()


def _bilinear(shape, size, T, addend=False, channels=None):
    def build():
        from mrfp_amd import ops
        B, ld, Hi, Wi = shape
        C = ld if channels is None else channels
        X, GY = act(shape, T, 41), act((B, C, size[0], size[1]), T, 42)
        AD = act((B, C, size[0], size[1]), T, 43) if addend else None

        def fn():
            x, a = leaf(X), leaf(AD)
            y = ops.upsample_bilinear(x, size, addend=a, channels=channels)
            y.backward(GY)
            return pc.named(y=y, dx=x.grad, daddend=grad(a))           # channels < ld: x.grad's pad channels are promised zero, and compared
        return fn
    return build


def _bilinear_cases():
    import launch_geometry_common as lg
    sites = ("ops._Bilinear.forward", "ops._Bilinear.backward")
    for T in (BF16, F32):
        for s, size in [((3, 64, 7, 5), (17, 23)), ((2, 19, 7, 6), (13, 9)), ((1, 8, 1, 2), (1, 5))] + \
                [(c["shape"], c["size"]) for c in lg.BILINEAR_CASES.values()]:
            CASES.append(Case("bilinear[%s-%s-%s]" % (sid(s), sid(size), dn(T)), _bilinear(s, size, T, addend=(s[1] != 19)), sites))
        # (channels < ld: backward starts from zeros_cl, so that the pad channels of the gradient are zero: no fresh buffer there)
        CASES.append(Case("bilinear_channels[2x32x7x6-19-%s]" % dn(T), _bilinear((2, 32, 7, 6), (13, 9), T, channels=19), sites[:1]))
        for s in [(3, 64, 17, 9), (2, 19, 7, 6), lg.ROW_SHAPES["two_lines_uneven"]["shape"]]:
            CASES.append(Case("broadcast[%s-%s]" % (sid(s), dn(T)), _bilinear((s[0], s[1], 1, 1), s[2:], T),
                              ("ops._Broadcast.forward", "ops._Broadcast.backward") + STATS))


_bilinear_cases()


def _elementwise(shape, T):
    def build():
        from mrfp_amd import ops
        B, C, H, W = shape
        X, Y, GY, G1 = act(shape, T, 51), act(shape, T, 52), act(shape, T, 53), act((B, C, 1, 1), T, 54)
        M = D(_rnd4((B, C), 55, 1.0, 0.0)).gt(0).float() * 2.0
        GM = D(_rnd4((B, C), 56, 1.0, 0.0))

        def fn():
            x, y = leaf(X), leaf(Y)
            s = ops.add(x, y)
            r = ops.relu(s)
            c = ops.channel_scale(r, M)
            g = ops.global_avg_pool(c)
            m = ops.plane_mean(c)
            torch.autograd.backward([c, g, m], [GY, G1, GM])
            return pc.named(add=s, relu=r, channel_scale=c, global_avg_pool=g, plane_mean=m, da=x.grad, db=y.grad)
        return fn
    return build


for _T in (BF16, F32):
    for _s in ROW_SHAPES:
        CASES.append(Case("add_relu_scale_gap_mean[%s-%s]" % (sid(_s), dn(_T)), _elementwise(_s, _T),
                          ("ops._Add.forward", "ops._GlobalAvgPool.forward", "ops._GlobalAvgPool.backward", "ops._PlaneMean.forward",
                           "ops._PlaneMean.backward", "ops._affine_fwd", "ops._affine_bwd")))


def _concat(shape, cb, T, up):
    def build():
        from mrfp_amd import ops
        B, Ca, H, W = shape
        Hi, Wi = (H // 2 + 1, W // 2 + 1) if up else (H, W)
        A, Bt = act(shape, T, 61), act((B, cb, Hi, Wi), T, 62)
        pad_to = 64 if up else 1
        Ct = (Ca + cb + pad_to - 1) // pad_to * pad_to
        GY = act((B, Ct, H, W), T, 63)

        def fn():
            a, b = leaf(A), leaf(Bt)
            y = ops.concat_upsample(a, b, (H, W), pad_to=pad_to) if up else ops.concat_channels([a, b])
            y.backward(GY)
            return pc.named(y=y, da=a.grad, db=b.grad)            # concat_upsample(pad_to=64): y is the physical buffer, its pad channels promised zero
        return fn
    return build


for _T in (BF16, F32):
    for _s, _cb in [((3, 64, 17, 9), 24), ((2, 19, 7, 6), 5), ((1, 8, 1, 1), 8), ((16, 8, 161, 5), 16)]:
        CASES.append(Case("concat_channels[%s+%d-%s]" % (sid(_s), _cb, dn(_T)), _concat(_s, _cb, _T, False),
                          ("ops._ConcatChannels.forward", "ops._ConcatChannels.backward")))
    for _s, _cb in [((3, 48, 17, 9), 24), ((2, 8, 7, 5), 8), ((16, 8, 161, 5), 16)]:
        CASES.append(Case("concat_upsample_pad64[%s+%d-%s]" % (sid(_s), _cb, dn(_T)), _concat(_s, _cb, _T, True),
                          ("ops._ConcatUpsample.forward", "ops._ConcatUpsample.backward")))


# ---- whitening (eager) -----------------------------------------------------------------------------------------------------------------
def _whiten(shape, T):
    def build():
        from mrfp_amd import ops
        B, C, H, W = shape
        n = float(H * W)
        X, Y, GY = act(shape, T, 71), act((B, 32, H, W), T, 72), act(shape, T, 73)
        GS, GMm = D(_rnd4((B, C), 74, 1.0, 0.0)), D(_rnd4((B, C // 16, 16, 16), 75, 1.0, 0.0))
        GG, GC = D(_rnd4((B, C, C), 76, 1.0, 0.0)), D(_rnd4((B, C, 32), 77, 1.0, 0.0))
        Wm0, Sh0 = D(_rnd4((B, C // 16, 16, 16), 78, 0.25, 0.0)), D(_rnd4((B, C), 79, 1.0, 0.0))
        gamma0, beta0 = vec(C, 80, scale=0.25, shift=1.0), vec(C, 81)
        eye = torch.eye(16, device=DEV)

        def fn():
            x, y2 = leaf(X), leaf(Y)
            gamma, beta, Wm, sh = leaf(gamma0), leaf(beta0), leaf(Wm0), leaf(Sh0)
            s, M = ops.group_moments(x)
            ya = ops.group_apply(x, Wm, sh)
            gram, cross = ops.channel_gram(x), ops.cross_gram(x, y2)

            def algebra(s_, M_):
                mean = (s_ / n).view(B, C // 16, 16, 1)
                cov = M_ / n - mean @ mean.transpose(-1, -2) + 1e-3 * eye
                tr = cov.diagonal(dim1=-2, dim2=-1).sum(-1).view(B, C // 16, 1, 1)
                wm = ops.group_isqrt(cov / tr, 5) * tr.rsqrt() * gamma.view(1, C // 16, 16, 1)
                return wm, beta.view(1, C) - (wm @ mean).reshape(B, C)
            yw = ops.group_whiten(x, algebra, (gamma, beta))        # eager: no captured graph
            torch.autograd.backward([s, M, ya, gram, cross, yw], [GS, GMm, GY, GG, GC, GY])
            return pc.named(sums=s, moments=M, group_apply=ya, channel_gram=gram, cross_gram=cross, group_whiten=yw, dx=x.grad, dy2=y2.grad,
                            dWm=Wm.grad, dshift=sh.grad, dgamma=gamma.grad, dbeta=beta.grad)
        return fn
    return build


for _T in (BF16, F32):
    for _s in [(3, 64, 17, 9), (2, 16, 7, 5), (2, 64, 3, 150)]:
        CASES.append(Case("whitening[%s-%s]" % (sid(_s), dn(_T)), _whiten(_s, _T),
                          ("ops._gm_call", "ops._ga_call", "ops._GroupISqrt.forward", "ops._GroupISqrt.backward", "ops._CrossGram.forward",
                           "ops.wgrad_workspace")))


# ---- Fourier amplitude mix -------------------------------------------------------------------------------------------------------------
def _fourier(shape, T, radius, high):
    def build():
        from mrfp_amd import ops
        X, GY = act(shape, T, 91), act(shape, T, 92)
        perm = torch.tensor([1, 0])

        def fn():
            x = leaf(X)
            y = ops.fourier_amplitude_mix(x, perm, radius, 0.8, high)
            y.backward(GY)
            return pc.named(y=y, dx=x.grad)
        return fn
    return build


for _s, _T, _r, _h in [((2, 16, 8, 8), F32, 3.0, False), ((2, 16, 8, 8), BF16, 3.0, False), ((2, 16, 8, 8), F32, 3.0, True),
                       ((2, 16, 8, 8), BF16, 3.0, True), ((2, 64, 48, 32), F32, 0.0, False), ((2, 64, 48, 32), BF16, 0.0, False),
                       ((2, 64, 64, 96), BF16, 6.0, False)]:
    CASES.append(Case("fourier_mix[%s-%s-r%g-%s]" % (sid(_s), dn(_T), _r, "high" if _h else "low"), _fourier(_s, _T, _r, _h),
                      ("ops._FourierMix.forward", "ops._FourierMix.backward")))


# ---- losses ------------------------------------------------------------------------------------------------------------------------------
def _loss_shapes():
    """(name, B, C, ld or None, (Hi, Wi) or None, (H, W)): dense (1,19,7,9), fused ((2,19,3,257),(7,771)) and the capped pair"""
    import launch_geometry_common as lg
    ce, up = lg.CE_CASE, lg.UPCE_CASE
    return [("dense_1x19x7x9", 1, 19, None, None, (7, 9)), ("fused_2x19x3x257_7x771", 2, 19, 32, (3, 257), (7, 771)),
            ("fused_tight_2x19x3x257_7x771", 2, 19, 0, (3, 257), (7, 771)),
            ("dense_capped", ce["B"], ce["C"], None, None, (ce["H"], ce["W"])),
            ("fused_capped", up["B"], up["C"], up["ld"], (up["Hi"], up["Wi"]), (up["H"], up["W"]))]


def _scores(B, C, ld, lo, size, T, seed):
    import eval_tta_common as tta
    if lo is None:
        return tta.nhwc_logits(B, C, size[0], size[1], T, seed).to(DEV)
    if ld == 0:                     # the tightest pitch: C rounded up to one 16-byte chunk (Cd == ld: dP is not cleared first)
        epc = 4 if T == F32 else 8
        ld = (C + epc - 1) // epc * epc
    return tta.nhwc_logits(B, ld, lo[0], lo[1], T, seed).to(DEV)


def _pixel_loss(kind, shp, T):
    def build():
        import loss_common as lc
        from mrfp_amd import ops
        _, B, C, ld, lo, size = shp
        g = torch.Generator().manual_seed(101)
        Z = _scores(B, C, ld, lo, size, T, 102)
        assert Z.is_contiguous(memory_format=CL)
        Y = lc.make_labels(B, C, size[0], size[1], g).to(DEV)
        Wc, Wb = lc.make_weights(C, g).to(DEV), lc.make_weights(C, g, rows=B).to(DEV)
        GS = torch.tensor(1.7, device=DEV)
        fused = lo is not None
        up = dict(size=size, channels=C) if fused else {}

        def one(tag, f, *a, **k):
            z = leaf(Z)
            loss = f(z, *a, **k)
            loss.backward(GS)
            return [(tag + ".loss", loss), (tag + ".dscores", z.grad)]

        def fn():
            out = []
            if kind == "ce":
                f = ops.upsample_cross_entropy if fused else ops.cross_entropy
                a = (Y, size, C) if fused else (Y,)
                out += one("plain", f, *a)
                out += one("weighted_smoothed", f, *a, weight=Wc, label_smoothing=0.1)
                out += one("per_image", f, *a, weight=Wb, per_image=True)
                out += one("sum", f, *a, reduction="sum")
                out.append(("class_weights", ops.label_class_weights(Y, C, 1.0, False, False)))
                out.append(("class_weights_norm_batch", ops.label_class_weights(Y, C, 1.0, True, True)))
            elif kind == "focal":
                f = ops.upsample_focal_loss if fused else ops.focal_loss
                a = (Y, size, C) if fused else (Y,)
                out += one("gamma2_weighted", f, *a, gamma=2.0, weight=Wc)
                out += one("gamma0.5_per_image", f, *a, gamma=0.5, per_image=True)
            elif kind == "region":
                f = ops.upsample_region_loss if fused else ops.region_loss
                a = (Y, size, C) if fused else (Y,)
                out += one("dice", f, *a, kind="dice")
                out += one("jaccard_per_image", f, *a, kind="jaccard", weight=Wc, per_image=True, present_only=False)
                out.append(("region_sums", ops.region_sums(Z, Y, **up)))
            elif kind == "ohem":
                masked, prob, state = ops.ohem_target(Z, Y, IGNORE, 0.7, (B * size[0] * size[1]) // 16, want_prob=True, want_state=True, **up)
                out += [("masked_target", masked), ("prob", prob), ("state", state.clone())]
                f = ops.upsample_ohem_cross_entropy if fused else ops.ohem_cross_entropy
                a = (Y, size, C) if fused else (Y,)
                out += one("ohem_ce", f, *a, thresh=0.6, min_kept=7, weight=Wc)
                out.append(("select_kth", ops.select_kth(prob.view(-1), 5)))
            elif kind == "relaxed":
                words, counts = ops.relax_labels(Y, C, border=1, strict_classes=[1, 3], want_counts=True)
                out += [("words", words), ("counts", counts), ("relaxed_counts", ops.relaxed_counts(words, C))]
                out += [("weights", ops.relaxed_class_weights(counts, 1.0, False, False)), ("weights_norm_batch", ops.relaxed_class_weights(counts, 1.0, True, True))]
                if fused:
                    out += one("soft_nll", ops.upsample_soft_nll, words, size, C, weight=Wb)
                else:
                    out += one("soft_nll", ops.soft_nll, words, C, weight=Wc)
            return pc.named(*out)
        return fn
    return build


_LOSS_SITES = {
    "ce": ("ops._PixelLoss.forward", "ops._Scores.grad", "ops.label_class_weights"),
    "focal": ("ops._PixelLoss.forward", "ops._Scores.grad"),
    "region": ("ops._region_forward", "ops._Scores.grad"),
    "ohem": ("ops._ohem_ws", "ops.ohem_target", "ops.select_kth", "ops._PixelLoss.forward"),
    "relaxed": ("ops.relax_labels", "ops.relaxed_counts", "ops.relaxed_class_weights", "ops._PixelLoss.forward"),
}
for _shp in _loss_shapes():
    for _T in (BF16, F32) + ((F16,) if _shp[0].startswith(("dense_1x", "fused_2x")) else ()):
        for _k in ("ce", "focal", "region", "ohem", "relaxed"):
            CASES.append(Case("%s[%s-%s]" % (_k, _shp[0], dn(_T)), _pixel_loss(_k, _shp, _T), _LOSS_SITES[_k]))


def _multihot_bytes(B, H, W, seed, C=19):
    """uint8 [B, C+1, H, W] as the reference's transform emits it (any non-zero byte is set): relaxed_common's label maps, relaxed and
    unpacked on the host."""
    import relaxed_common as rc
    words = rc.np_relax(rc.make_label_maps(B, H, W, C, seed).numpy(), C, 1)
    return torch.from_numpy(rc.unpack(words, C, set_value=200)).to(DEV)


@case("pack_multihot[2x20x7x9]", ("ops.pack_multihot",))
def _multihot():
    from mrfp_amd import ops
    M = _multihot_bytes(2, 7, 9, 111)

    def fn():
        words, counts = ops.pack_multihot(M, want_counts=True)
        return pc.named(words=words, counts=counts, words_alone=ops.pack_multihot(M))
    return fn


@case("pack_multihot[capped-1x20x725x725]", ("ops.pack_multihot",))
def _multihot_capped():
    from mrfp_amd import ops
    M = _multihot_bytes(1, 725, 725, 112)

    def fn():
        words, counts = ops.pack_multihot(M, want_counts=True)
        return pc.named(words=words, counts=counts)
    return fn


# ---- evaluation / prediction ---------------------------------------------------------------------------------------------------------------
def _predict(shp, T):
    def build():
        import loss_common as lc
        import eval_tta_common as tta
        from mrfp_amd import ops
        _, B, C, ld, lo, size = shp
        H, W = size
        g = torch.Generator().manual_seed(121)
        Z = _scores(B, C, ld, lo, size, T, 122)
        Y = lc.make_labels(B, C, H, W, g).to(DEV)
        import input_aug_common as ia
        from mrfp_amd.predict import Palette
        table = Palette.cityscapes().device_table(torch.device(DEV, torch.cuda.current_device()))
        image = torch.from_numpy(np.stack([ia.sample(W, H, 124 + i)[0] for i in range(B)])).to(DEV)
        NC = C
        ZA = tta.nhwc_logits(B, 24, max(H // 2, 1), max(W // 2, 1), T, 123).to(DEV)

        def fn():
            out = []
            if lo is None:
                hist, pred = ops.argmax_hist(Z, Y, want_pred=True)
            else:
                p = ops.upsample_argmax(Z, size, C, target=Y, per_image=True, want_pred=True, want_conf=True, loss_acc=True)
                hist, pred = p.hist, p.pred
                out += [("conf", p.conf), ("loss_acc", p.loss_acc)]
            out += [("hist", hist), ("pred", pred), ("colours", ops.colorize(pred, table)), ("blend", ops.colorize(pred, table, image, 0.4))]
            acc, cnt = torch.zeros(B, H, W, NC, device=DEV), torch.zeros(B, H, W, device=DEV)
            ops.prob_accum(ZA, acc, cnt)
            ops.prob_accum(ZA, acc, cnt, rect=(0, 0, max(H // 2, 1), W), flip=True, weight=0.5)
            unc = torch.zeros(1, dtype=torch.int64, device=DEV)
            h2, p2 = ops.acc_argmax_hist(acc, cnt, Y, want_pred=True, uncovered=unc)
            return pc.named(*out, acc=acc, cnt=cnt, acc_hist=h2, acc_pred=p2, uncovered=unc)
        return fn
    return build


for _shp in _loss_shapes():
    if _shp[0].startswith("fused_tight"):
        continue
    for _T in (BF16, F32):
        CASES.append(Case("predict[%s-%s]" % (_shp[0], dn(_T)), _predict(_shp, _T),
                          ("ops.acc_argmax_hist", "ops.colorize") + (("ops.argmax_hist",) if _shp[3] is None else ("ops.upsample_argmax",))))


# ---- convolutions ----------------------------------------------------------------------------------------------------------------------------
_CONV_SITES = ("conv._Conv2d.forward", "conv._Conv2d.backward", "conv.get_pack", "conv._launch_wgrads.run",
               "ops.wgrad_workspace")


def _conv(c, T, phys_out=None, want_dx=True, cphys=None):
    """cphys: the input arrives channel-padded to cphys > C (zeros), as concat_upsample(pad_to=) hands it over: the dgrad pack's pad rows
    are zero, so x.grad's pad channels are promised exact zeros -- x.grad is compared over the physical channel count."""
    def build():
        import conv_exact_common as cx
        from mrfp_amd import conv
        B, C, H, W, N, k, st, pad, dil, hb = c
        d = cx.dense_data(c)
        epc = 4 if T == F32 else 8
        xh = d["x"] if cphys is None else torch.cat([d["x"], torch.zeros(B, cphys - C, H, W)], 1)
        X, Wt, Bt = D(xh, T), d["w"].to(DEV), (d["b"].to(DEV) if hb else None)
        Np = phys_out if phys_out is not None else N
        gy = d["gy"]
        if Np != N:
            gy = torch.cat([gy, torch.zeros(B, Np - N, *gy.shape[2:])], 1)
        GY = D(gy, T)
        dx = want_dx and xh.shape[1] % epc == 0

        def fn():
            x, w, b = (leaf(X) if dx else X), leaf(Wt), leaf(Bt)
            y = conv.conv2d(x, w, b, st, pad, dil, phys_out)
            cs = getattr(y, "_mrfp_colstats", None)
            stats = cs.final.clone() if cs is not None else None
            y.backward(GY)
            return pc.named(y=y, colstats=stats, dx=(x.grad if dx else None), dweight=w.grad, dbias=grad(b))      # phys_out: y's pad channels are promised zero, and compared
        return fn
    return build


def _conv_cases():
    import conv_exact_common as cx
    C = cx.CASES
    both = [("igemm_stem_cpad", C[0], None), ("igemm_strided3x3", (2, 128, 16, 16, 128, 3, 2, 1, 1, False), None),
            ("igemm_dilated_bias", (2, 64, 19, 23, 128, 3, 1, 2, 2, True), None),
            ("pw_1x1", (2, 64, 20, 18, 256, 1, 1, 0, 1, False), None), ("pw_1x1_strided", (2, 256, 16, 16, 512, 1, 2, 0, 1, False), None),
            ("npad_19", (2, 256, 12, 10, 19, 1, 1, 0, 1, True), None), ("npad_19_phys32", (2, 256, 12, 10, 19, 1, 1, 0, 1, True), 32),
            ("decoder_304", (2, 304, 12, 10, 256, 3, 1, 1, 1, False), None),
            ("c64", (3, 64, 33, 31, 64, 3, 1, 1, 1, False), None), ("c64_bias", (2, 64, 20, 18, 64, 3, 1, 1, 1, True), None),
            ("c128_dgrad", cx.c64_as_dense(cx.C128_CASES[0]), None),
            ("pwk", cx.pwk_as_dense(cx.PWK_CASES[2]), None)]
    for T in (BF16, F32):
        c = (2, 304, 12, 10, 256, 3, 1, 1, 1, False)
        CASES.append(Case("conv_cpad_304_in_320[%s-%s]" % (cx.sid(c), dn(T)), _conv(c, T, cphys=320), _CONV_SITES + ("conv.conv2d",)))
    for name, c, po in both:
        for T in (BF16, F32):
            CASES.append(Case("conv_%s[%s-%s]" % (name, cx.sid(c), dn(T)), _conv(c, T, po),
                              _CONV_SITES + (("ops.channel_sums",) if c[9] else ("conv.conv2d",))))      # (bias-free: the epilogue statistics rows)
    # 16-bit kernels only the largest listed shapes reach: weight-gradient kernels wg1 (1), wg3 (0, at B = 8) and the 256 x 128 tile (4)
    for name, c in [("wg1", cx.pwk_as_dense(cx.PWK_CASES[4])), ("wg3", (8, 128, 192, 192, 128, 3, 1, 1, 1, False)),
                    ("wgrad_tile4", (2, 304, 240, 240, 256, 3, 1, 1, 1, False))]:
        CASES.append(Case("conv_%s[%s-bf16]" % (name, cx.sid(c)), _conv(c, BF16), _CONV_SITES + ("conv.conv2d",)))


_conv_cases()


def _wstats(c, T):
    def build():
        import conv_exact_common as cx
        from mrfp_amd import conv, ops
        B, C, N, H, W, dil, rs = c
        d = cx.conv_data(B, C, H, W, N, 3, 1, dil, dil, False, cx.seed_of(c))
        X, Wt = D(d["x"], T), d["w"].to(DEV)
        plan = ops.nearest_plan(H, W, device=DEV, **(rs if isinstance(rs, dict) else dict(scale=rs)))
        GY = act((B, N, plan.Ho, plan.Wo), T, 131)
        G, Bb = vec(N, 132, scale=0.25, shift=1.0), vec(N, 133)

        def fn():
            x, w, g, b = leaf(X), leaf(Wt), leaf(G), leaf(Bb)
            rmean, rvar = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
            y = conv.conv2d(x, w, None, 1, dil, dil, stat_resize=plan)
            z = ops.batch_norm_act(y, g, b, rmean, rvar, training=True, relu=True, plan=plan)
            z.backward(GY)
            return pc.named(y_conv=y, z_bn=z, dx=x.grad, dweight=w.grad, dgamma=g.grad, dbeta=b.grad, running_mean=rmean, running_var=rvar)
        return fn
    return build


def _wstat_cases():
    import conv_exact_common as cx
    c = min(cx.WSTAT_CASES, key=lambda c: c[0] * c[1] * c[3] * c[4])
    for T in (BF16, F32):
        CASES.append(Case("conv_wstats_resize_bn[%s-%s]" % ("x".join(str(v) for v in c[:6]), dn(T)), _wstats(c, T), ("conv.conv2d", "conv._Conv2d.forward")))


_wstat_cases()


def _pad_input(shape, T):
    def build():
        from mrfp_amd import conv
        X = act(shape, F32, 141).contiguous()

        def fn():
            return pc.named(y=conv.pad_input_channels(X, T))            # the physical tensor: zero pad channels promised
        return fn
    return build


for _T in (BF16, F32):
    for _s in [(2, 3, 17, 9), (1, 1, 1, 1), (2, 3, 161, 5)]:
        CASES.append(Case("pad_input_channels[%s-%s]" % (sid(_s), dn(_T)), _pad_input(_s, _T), ("conv.pad_input_channels",)))


def _depthwise(B, C, H, W, stride, dil, T, bias):
    def build():
        import conv_exact_common as cx
        from mrfp_amd import ops
        d = cx.dw_data((B, C, H, W, stride, dil))
        X, Wt, Bt, GY = D(d["x"], T), d["w"].to(DEV), (d["b"].to(DEV) if bias else None), D(d["gy"], T)

        def fn():
            x, w, b = leaf(X), leaf(Wt), leaf(Bt)
            y = ops.depthwise_conv2d(x, w, b, stride, dil, dil)
            cs = getattr(y, "_mrfp_colstats", None)
            stats = cs.final.clone() if cs is not None else None
            y.backward(GY)
            return pc.named(y=y, colstats=stats, dx=x.grad, dweight=w.grad, dbias=grad(b))           # Cp > C: the caller sees the logical channels only (the pad is not returned)
        return fn
    return build


def _depthwise_cases():
    import launch_geometry_common as lg
    p = lg.DW_CASES["c12_padded"]
    sites = ("ops._DepthwiseConv2d.forward", "ops._DepthwiseConv2d.backward")
    for T in (BF16, F32):
        for st in (1, 2):
            CASES.append(Case("depthwise[c12_padded-s%d-%s]" % (st, dn(T)), _depthwise(p["B"], p["C"], p["H"], p["W"], st, 1, T, True),
                              sites + ("ops.channel_sums",)))
            CASES.append(Case("depthwise[3x24x17x9-s%d-%s]" % (st, dn(T)), _depthwise(3, 24, 17, 9, st, 2, T, False),
                              sites + ("ops.depthwise_conv2d",)))
        CASES.append(Case("depthwise[2x19x7x6-s1-%s]" % dn(T), _depthwise(2, 19, 7, 6, 1, 1, T, False), sites))


_depthwise_cases()


def _head(c, T, mode):
    """conv 3x3 with a skip alias -> the shared pointwise pair on the alias (low-rank stand-in), or a residual tail on the alias (gate):
    mode 'lowrank' (the dgrad takes the factors), 'unlowrank' / 'ungate' (only the alias is used: the convolution's output has no
    gradient, and backward materialises the tagged gradient)."""
    def build():
        import conv_exact_common as cx
        from mrfp_amd import conv, ops
        B, C, H, W, N, dil = c
        d = cx.conv_data(B, C, H, W, N, 3, 1, dil, dil, False, cx.seed_of(c))
        X, W3, GY = D(d["x"], T), d["w"].to(DEV), D(d["gy"], T)
        X1 = D(cx.ternary((B, C, (H + 1) // 2, (W + 1) // 2), 32, 151), T)
        Wf, Bf = cx.ternary((19, C, 1, 1), 16, 152).to(DEV), cx.ternary((19,), 32, 153).to(DEV)
        G1 = D(torch.cat([cx.ternary((B, 19, (H + 1) // 2, (W + 1) // 2), 8, 154), torch.zeros(B, 13, (H + 1) // 2, (W + 1) // 2)], 1), T)
        G2 = D(torch.cat([cx.ternary((B, 19, H, W), 8, 155), torch.zeros(B, 13, H, W)], 1), T)
        GZ = D(cx.ternary((B, C, H, W), 16, 156), T)
        Gm, Bt = vec(C, 157, scale=0.25, shift=1.0), vec(C, 158)
        XT = D(cx.ternary((B, C, H, W), 32, 159), T)

        def fn():
            x, x1, xt, w3, wf, bf, g, bb = leaf(X), leaf(X1), leaf(XT), leaf(W3), leaf(Wf), leaf(Bf), leaf(Gm), leaf(Bt)
            hits = (conv.LOWRANK_SKIP_HITS[0], conv.GATED_SKIP_HITS[0])
            y, alias = conv.conv2d(x, w3, None, 1, dil, dil, None, True)
            outs, gys = ([y], [GY]) if mode in ("lowrank", "gated") else ([], [])
            if mode in ("lowrank", "unlowrank"):
                p_low, p_half = conv.shared_conv1x1_pair(x1, alias, wf, bf, 32)
                outs, gys = outs + [p_low, p_half], gys + [G1, G2]
            else:
                rmean, rvar = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
                z = ops.batch_norm_act(xt, g, bb, rmean, rvar, training=True, relu=True, res=alias)
                outs, gys = outs + [z], gys + [GZ]
            try:
                torch.autograd.backward(outs, gys)
            except Exception:
                conv.backward_failed()
                raise
            if T != F32 and mode == "lowrank":
                assert conv.LOWRANK_SKIP_HITS[0] == hits[0] + 1
            if T != F32 and mode == "gated":
                assert conv.GATED_SKIP_HITS[0] == hits[1] + 1
            if mode in ("lowrank", "unlowrank"):
                onames, used = ["p_low", "p_half"], dict(dx1=x1.grad, dwf=wf.grad, dbf=bf.grad)
            else:
                onames, used = ["z_tail"], dict(dxt=xt.grad, dgamma=g.grad, dbeta=bb.grad)
            onames = (["y"] if len(outs) > len(onames) else []) + onames
            return pc.named(*zip(onames, outs), dx=x.grad, dw3=grad(w3), **used)
        return fn
    return build


def _head_cases():
    import conv_exact_common as cx
    small = (3, 64, 10, 140, 64, 1)          # N = 64: c64 dgrad in bf16 (the low-rank operand), generic tiles in fp32
    both = cx.C128_CASES[0][:6]              # 128 -> 64: the dgrad is the 128-output form of that kernel (two column groups)
    assert small in cx.LOWRANK_CASES and both == (2, 128, 20, 18, 64, 1)
    pair = ("conv._SharedConv1x1Pair.forward", "conv._SharedConv1x1Pair.backward")
    for T in (BF16, F16, F32):
        CASES.append(Case("lowrank_pair[%s-%s]" % (sid(small), dn(T)), _head(small, T, "lowrank"), pair))
        CASES.append(Case("gated_tail[%s-%s]" % (sid(small), dn(T)), _head(small, T, "gated"), ("ops._BatchNormAct.backward",)))
    CASES.append(Case("lowrank_pair[%s-bf16]" % sid(both), _head(both, BF16, "lowrank"), pair))
    CASES.append(Case("unlowrank[%s-bf16]" % sid(small), _head(small, BF16, "unlowrank"), pair + ("skipgrad.unlowrank",)))
    CASES.append(Case("ungate[%s-bf16]" % sid(small), _head(small, BF16, "ungate"), ("skipgrad.ungate",)))


_head_cases()


# ---- folded inference ----------------------------------------------------------------------------------------------------------------------------
def _folded(specs, T):
    """specs: [(case tuple, act, with residual)]: one registered fold set, every pair evaluated folded."""
    def build():
        import conv_exact_common as cx
        import rounding_model_common as rm
        data = []
        for c, a, res in specs:
            B, C, H, W, N, k, st, pad, dil, hb = c[:10]
            groups = c[10] if len(c) > 10 else 1
            sd = cx.seed_of(c)
            epc = 4 if T == F32 else 8
            Np = (N + epc - 1) // epc * epc
            Ho, Wo = cx.out_size(H, k, st, pad, dil), cx.out_size(W, k, st, pad, dil)
            data.append(dict(x=act((B, C, H, W), T, 161), w=cx.ternary((N, C // groups, k, k), 32, sd) * 0.125,
                             b=cx.ternary((N,), 32, sd + 1) if hb else None, bn=rm.bn_params(N, sd % 97),
                             res=act((B, Np, Ho, Wo), T, 162) if res else None))

        def fn():
            from mrfp_amd import conv
            from mrfp_amd.inference import _FoldSet
            from mrfp_amd.network import mynn
            pairs = _FoldSet()
            for (c, a, res), d in zip(specs, data):
                B, C, H, W, N, k, st, pad, dil, hb = c[:10]
                groups = c[10] if len(c) > 10 else 1
                m = mynn.HipConv2d(C, N, k, st, pad, dil, groups=groups, bias=hb)
                n = mynn.HipLocalBatchNorm2d(N)
                with torch.no_grad():
                    m.weight.copy_(d["w"])
                    if hb:
                        m.bias.copy_(d["b"])
                    n.weight.copy_(d["bn"][0]); n.bias.copy_(d["bn"][1]); n.running_mean.copy_(d["bn"][2]); n.running_var.copy_(d["bn"][3])
                pairs.append((m.to(DEV).eval(), n.to(DEV).eval()))
            conv.register_fold_set(pairs)
            out = []
            with torch.no_grad():
                for (c, a, res), d, (m, n) in zip(specs, data, pairs):
                    if m.groups != 1:
                        out.append(conv.depthwise_conv2d_folded(d["x"], m, n, a))
                    else:
                        out.append(conv.conv2d_folded(d["x"], m, n, a, d["res"]))
            fn.keep = pairs                     # the set is held by weak reference: alive until the next run replaces it
            return pc.named(*(("y%d_%s" % (i, cx.sid(c[:9])), t) for i, ((c, _a, _r), t) in enumerate(zip(specs, out))))
        return fn
    return build


def _fold_cases():
    import conv_exact_common as cx
    specs = [(cx.CASES[0], 1, False),                                     # generic tiles, Cphys > C
             ((2, 64, 20, 18, 256, 1, 1, 0, 1, False), 0, True),          # pointwise, residual
             ((3, 64, 33, 31, 64, 3, 1, 1, 1, False), 1, True),           # weight-stationary 3x3
             ((2, 256, 12, 10, 19, 1, 1, 0, 1, True), 0, False),          # Nphys > N, conv bias
             ((2, 128, 16, 16, 128, 3, 2, 1, 1, False), 2, False),        # strided, ReLU6
             ((3, 24, 17, 9, 24, 3, 2, 1, 1, False, 24), 2, False),       # depthwise
             ((2, 19, 7, 6, 19, 3, 1, 2, 2, True, 19), 0, False)]         # depthwise, Cp > C (the logical slice is returned)
    for T in (BF16, F32):
        CASES.append(Case("folded_set[%s]" % dn(T), _folded(specs, T), ("conv._fold_slot", "conv.conv2d_folded", "conv.depthwise_conv2d_folded")))
    CASES.append(Case("folded_pwk[bf16]", _folded([(cx.pwk_as_dense(cx.PWK_CASES[2]), 1, False)], BF16), ("conv._fold_slot", "conv.conv2d_folded")))


_fold_cases()


# ---- trainer arenas -----------------------------------------------------------------------------------------------------------------------------
def _arena(T):
    """Two convolutions of ONE geometry with their gradients in a flat arena: backward queues both weight gradients and issues one
    GROUPED launch (mrfp_conv_wgrad_grouped: problems x split-K slabs in one workspace); then the accumulation arena and a checked,
    averaged optimiser step."""
    def build():
        import conv_exact_common as cx
        c = (2, 64, 40, 36, 64, 3, 1, 1, 1, 2)
        assert c in cx.GROUP_CASES
        X0, G0 = cx.group_data(c, 0)
        X1, G1 = cx.group_data(c, 1)
        X0, G0, X1, G1 = (D(t, T) for t in (X0, G0, X1, G1))
        W0, W1 = cx.ternary((64, 64, 3, 3), 16, 171) * 0.125, cx.ternary((64, 64, 3, 3), 16, 172) * 0.125

        def fn():
            from mrfp_amd import conv, harness
            from mrfp_amd.network import mynn
            m = torch.nn.ModuleList([mynn.HipConv2d(64, 64, 3, 1, 1, bias=False), mynn.HipConv2d(64, 64, 3, 1, 1, bias=False)])
            with torch.no_grad():
                m[0].weight.copy_(W0); m[1].weight.copy_(W1)
            m = m.to(DEV)
            opt = harness.FlatSGD(m, lr=0.1, average="ema")
            scaler = harness.LossScaler(init_scale=1.0, dynamic=False, device=DEV)
            seen = len(conv.WGRAD_GROUP_LAUNCHES)
            x0, x1 = leaf(X0), leaf(X1)
            try:
                torch.autograd.backward([m[0](x0), m[1](x1)], [G0, G1])      # one geometry twice: queued, then ONE grouped launch
            except Exception:
                conv.backward_failed()
                raise
            conv.join_wgrad_stream()
            assert list(conv.WGRAD_GROUP_LAUNCHES)[seen:] == [2]
            g1 = opt.flat_g.clone()
            opt.accumulate(first=True)
            opt.accumulate()
            opt.accumulate(into_grad=True)
            g3 = opt.flat_g.clone()
            opt.step(gscale=1.0 / 3.0, scaler=scaler, max_grad_norm=5.0)
            y = m[0](x0.detach())                                            # the repacked weights
            return pc.named(grad_arena=g1, grad_arena_x3=g3, accum_arena=opt.flat_a, params=opt.flat_p, momentum=opt.flat_m, average=opt.flat_e,
                            scaler_state=scaler.state.clone(), dx0=x0.grad, dx1=x1.grad, y_after_step=y)
        return fn
    return build


for _T in (BF16, F32):
    CASES.append(Case("flat_arena_grouped_wgrad_accumulate_sgd[2x64x40x36-%s]" % dn(_T), _arena(_T),
                      ("harness.FlatArena.accumulate", "harness.FlatSGD.step", "conv._launch_wgrads.run", "conv._Conv2d.backward",
                       "ops.wgrad_workspace")))


# ---- input pipeline --------------------------------------------------------------------------------------------------------------------------------
def _sample(w, h, seed=0):
    import input_aug_common as ia
    img, lab = ia.sample(w, h, seed)
    return torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)


def _train_transforms(w, h):
    def build():
        from mrfp_amd import input_pipeline as ip
        img, lab = _sample(w, h, 3)
        jit = [("brightness", 1.2), ("contrast", 0.9), ("saturation", 1.1), ("hue", 0.1)]
        T = min(w, h) - 4
        d_train = ip.Draw(True, jit, (w + 5, h - 3), (2, 4), (1, 2), 0.6)
        train = ip.TrainTransform(T)
        d_train.pad = (max((T - (w + 5)) // 2 + 1, 0) if T > w + 5 else 0, (T - (h - 3)) // 2 + 1 if T > h - 3 else 0)
        W2, H2 = w + 5 + 2 * d_train.pad[0], h - 3 + 2 * d_train.pad[1]
        d_train.crop = (min(1, W2 - T), min(2, H2 - T))
        resize, d_res = ip.ResizeTransform(w // 2 + 1, h // 2 + 2), ip.Draw(False, jit[:2], (0, 0), (0, 0), (0, 0), None)
        crop, d_crop = ip.CropTransform(h - 6, w - 7), ip.Draw(True, None, (w, h), (0, 0), (3, 2), 0.3)
        sc = ip.ScaleCropTransform(min(w, h), T, fill=7, rotate_degree=10.0, jitter=True, contrast=True, normalize=((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)))
        ow, oh = (T - 3, int(1.0 * h * (T - 3) / w)) if h > w else (int(1.0 * w * (T - 3) / h), T - 3)
        d_sc = ip.ScaleCropDraw(True, jit[1:3], 7.3, (ow, oh), (max(T - ow, 0), max(T - oh, 0)), (0, 0), 0.4)
        d_sc2 = ip.ScaleCropDraw(False, None, 180.0, (ow, oh), (max(T - ow, 0), max(T - oh, 0)), (0, 0), None)

        def fn():
            out = []
            for tag, pair in (("train", train(img, lab, d_train)), ("resize", resize(img, lab, d_res)), ("crop", crop(img, lab, d_crop)),
                              ("scale_crop_rotated", sc(img, lab, d_sc)), ("scale_crop_180", sc(img, lab, d_sc2)),
                              ("rotate", ip.rotate(img, lab, -13.9))):
                out += [(tag + ".image", pair[0]), (tag + ".label", pair[1])]
            return pc.named(*out, contrast=ip.contrast(img, 2.0))
        return fn
    return build


def _eval_transforms(w, h):
    def build():
        from mrfp_amd import input_pipeline as ip
        img, lab = _sample(w, h, 5)
        enc = ip.label_encoder("Mapillary")
        fix = ip.FixScaleCropTransform(min(w, h) - 3, contrast=True, normalize=((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)))
        fix2 = ip.FixScaleCropTransform(min(w, h) + 5)
        rh, rh_narrow = ip.ResizeHeightCenterCropPad(16), ip.ResizeHeightCenterCropPad(h + 9, ignore_index=255)
        ev = ip.EvalTransform()

        def fn():
            out = []
            for tag, pair in (("fix_scale_crop", fix(img, lab, enc)), ("fix_scale_crop_plain", fix2(img, lab)), ("resize_height", rh(img, lab, enc)),
                              ("resize_height_tall", rh_narrow(img, lab)), ("eval", ev(img, lab, enc))):
                out += [(tag + ".image", pair[0]), (tag + ".label", pair[1])]
            return pc.named(*out, encoded=enc(lab), encoded_int64=enc.to_int64(lab))
        return fn
    return build


def _freq(shape, radius):
    def build():
        from mrfp_amd import input_pipeline as ip
        X = D(_rnd4(shape, 181, 60.0, 120.0)).contiguous()

        def fn():
            return pc.named(hpf=ip.hpf(X, radius), lpf=ip.lpf(X, radius), phot=ip.phot(X))
        return fn
    return build


for _w, _h in [(53, 37), (70, 130)]:
    CASES.append(Case("input_train_transforms[%dx%d]" % (_w, _h), _train_transforms(_w, _h),
                      ("input_pipeline._jitter", "input_pipeline._resample", "input_pipeline._out_slot", "input_pipeline._assemble",
                       "input_pipeline._rotate", "input_pipeline._assemble_post")))
    CASES.append(Case("input_eval_transforms[%dx%d]" % (_w, _h), _eval_transforms(_w, _h),
                      ("input_pipeline.FixScaleCropTransform.__call__", "input_pipeline.ResizeHeightCenterCropPad.__call__",
                       "input_pipeline._assemble_post", "input_pipeline._out_slot")))
for _s, _r in [((3, 27, 45), 4.0), ((2, 3, 48, 40), 16.0)]:
    CASES.append(Case("input_freq[%s-r%g]" % (sid(_s), _r), _freq(_s, _r), ("input_pipeline._band", "input_pipeline.phot", "input_pipeline._out_slot")))


# ---- the whole model ---------------------------------------------------------------------------------------------------------------------------------
@case("model_mrfpplus_resnet50[2x64x64-bf16-all_toggles]", ())
def _model():
    """Declares no sites: it is here for the combinations -- epilogue statistics feeding the next operator, skip aliases, the head."""
    from mrfp_amd import deepv3, synth
    from mrfp_amd.config import cfg
    cfg.MODEL.ACT_DTYPE = BF16
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            model = deepv3.MRFPPlus(19, trunk="resnet-50", criterion=torch.nn.CrossEntropyLoss(ignore_index=255))
        sd = synth.synth_state_dict(synth.spec_of(model.state_dict()), seed=0, residual_gain=0.3)
        model.load_state_dict(sd)
        model = model.to(DEV).train()
    finally:
        cfg.MODEL.ACT_DTYPE = F32
    x, y = synth.synth_batch(2, 64, 64, seed=91)
    x, y = x.to(DEV), y.to(DEV)
    noise = synth.synth_noise(2, seed=92, channels=(64, 256))
    from mrfp_amd.perturb import MultiResolutionFourier
    fp = MultiResolutionFourier(radii=(3.0, 3.0, 2.0), lam=0.8)       # planes of 16, 16 and 8 pixels behind the stem, layer1, layer2
    fp.perm = torch.tensor([1, 0])
    names = [n for n, p in model.named_parameters() if p.requires_grad]

    def fn():
        cfg.MODEL.ACT_DTYPE = BF16
        try:
            model.load_state_dict(sd)
            model.rng = deepv3.InjectedRandom((True, True, True), noise)
            model.fourier_perturb = fp
            for p in model.parameters():
                p.grad = None
            loss = model(x, y, training=True)
            loss.backward()
        finally:
            cfg.MODEL.ACT_DTYPE = F32
        params = dict(model.named_parameters())
        return pc.named(("loss", loss), *(("d " + n, params[n].grad) for n in names))
    return fn


# ---- the test ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_result_does_not_depend_on_fresh_memory(case):
    fn = case.build()                                   # inputs: once, outside the poisoned blocks
    sites = pc.run_three(fn)
    missing = sorted(set(case.sites) - sites)
    assert not missing, "%s declares call sites it did not take: %s (taken: %s)" % (case.name, missing, sorted(sites))
