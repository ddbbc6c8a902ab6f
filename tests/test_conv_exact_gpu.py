"""Every convolution kernel term for term: on the ternary data of tests/conv_exact_common.py the device result must EQUAL the float64
reference -- forward, input gradient, weight gradient, bias gradient, fused statistics -- in fp32, bf16 and f16.

Why equality is owed, and the conditions under which it is (asserted here on every reference, never on a device result), are in
conv_exact_common.py; tests/test_conv_exact_cpu.py proves on the host that a scrambled fp32 summation order reproduces the reference
and that a lost product, a tap read from the neighbouring pixel, a dropped K-tile remainder, a lost weight-gradient pixel, a missing
statistics row block, a padding pixel read as its neighbour and exchanged parity classes each change the result.  So a kernel that
loses or misaddresses a single term fails here, in every type, however many channels dilute it.

One output is held to a documented alternative instead of the plain reference, still with equality: the bias gradient.
ops.channel_sums forms it as the column mean of the statistics pass times the count (two fp32 roundings around an exact sum), so it
is compared with exactly that expression of the exact sum (cx.ref_dbias_as_computed, where the code is quoted).

Every comparison is an equality (cx.mismatch: the differing elements with their positions modulo the tile sizes, and the library
entry points the failing call went through, recorded with _lib.HOOK).  There is no numeric bound in this file.

The calls go through mrfp_amd.conv / mrfp_amd.ops as in tests/test_conv_gpu.py, tests/test_depthwise_gpu.py and
tests/test_lowrank_skip_gpu.py, whose case lists these are.  Kernels that small shapes reach only behind a switch run in one child
process per switch set (the switches are read once per process), on the library as built.

Left out on purpose: the folded-BatchNorm inference packs (a float scale: not exact), the Fourier and whitening units.
"""
import ctypes
import functools
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import conv_exact_common as cx
from conv_exact_common import dname, sid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TYPES = [F32, BF16, F16]
ENTRIES, KINDS = set(), set()      # library entry points / (dtype, wgrad plan kernel, variant) reached in this process


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def wgrad_kind(d, B, H, W, C, N, ldn, R, S, Ho, Wo, st, ph, pw, dl, count):
    from mrfp_amd import _lib
    plan = (ctypes.c_int64 * 5)()
    if _lib.lib().mrfp_conv_wgrad_plan(int(d), B, H, W, C, N, ldn, R, S, Ho, Wo, st, ph, pw, dl, count, plan) != 0:
        return None
    return (int(d), int(plan[0]), int(plan[1]))


def hooked(fn):
    """-> (result of fn(), names of the library entry points it called); weight-gradient launches also record their plan kind"""
    from mrfp_amd import _lib
    names = []

    def hook(name, args):
        names.append(name)
        ENTRIES.add(name)
        if name == "mrfp_conv_wgrad":                       # (x, dy, dw, ws, dtype, B, H, W, C, Ctrue, N, ldn, R, S, Ho, Wo, stride, pads, dil)
            a = args[4:20]
            KINDS.add(wgrad_kind(a[0], a[1], a[2], a[3], a[4], *a[6:16], 1))
        elif name == "mrfp_conv_wgrad_grouped":             # (xs, dys, dws, count, ws, dtype, ...)
            a = args[5:21]
            KINDS.add(wgrad_kind(a[0], a[1], a[2], a[3], a[4], *a[6:16], args[3]))
    _lib.HOOK[0] = hook
    try:
        return fn(), names
    finally:
        _lib.HOOK[0] = None


def eq(label, got, want, names=()):
    g = got.detach().cpu()
    if tuple(g.shape) == tuple(want.shape) and torch.equal(g.to(want.dtype), want):      # (16 bit -> fp32 / float64: exact)
        return
    msg = cx.mismatch(label, got, want)
    assert msg == "", "\n%s\nentry points: %s" % (msg, sorted(set(names)))


def dev(t, T, grad=False):
    return t.to(DEV, T).contiguous(memory_format=CL).requires_grad_(grad)


def checked(label, ref, T, terms, stats=False, mult=None):
    """the conditions on one reference output (conv_exact_common): integer-valued, inside the type's limit, at most `terms` terms of
    magnitude <= 1 behind an element, per-channel sum of squares below 2^24 where statistics are taken"""
    cx.check_output(label, ref, None, T)
    cx.check_terms(label, terms)
    if stats:
        cx.check_stats(label, ref, mult)
    return ref.float()        # (integers below 2^24: the float64 reference, held in fp32 without loss)


def stat_rows(st, N):
    """ConvStats -> (total [2][N], raw row blocks [nblk][2][N]) summed / read on the host in float64"""
    tot = st.final.view(st.final_count, 2, N).double().sum(0).cpu()
    rows = st.rows[:st.row_blocks * 2 * N].view(st.row_blocks, 2, N).double().cpu()
    return tot, rows


def check_colstats(label, y, yref, names, mult=None):
    """The rows y._mrfp_colstats exposes -- per row block, per image, total -- against sum y and sum y^2 of the reference."""
    st = getattr(y, "_mrfp_colstats", None)
    assert st is not None, (label, "no fused statistics")
    B, N, Ho, Wo = yref.shape
    s, q = cx.ref_stats(yref, mult)
    tot, rows = stat_rows(st, N)
    eq(label + " total sum", tot[0], s.sum(0), names)
    eq(label + " total sum of squares", tot[1], q.sum(0), names)
    rb = st.block_rows
    if mult is not None:
        assert rb == 0 and st.elements == B * int(mult.sum()), (label, rb, st.elements)
        return
    assert st.elements == B * Ho * Wo, (label, st.elements)
    if rb < 0:                 # the weight-stationary 3x3 kernel: -rb rows per image
        assert B * (-rb) == st.row_blocks, (label, rb, st.row_blocks)
        per = rows.view(B, -rb, 2, N).sum(1)
        eq(label + " per-image sum", per[:, 0], s, names)
        eq(label + " per-image sum of squares", per[:, 1], q, names)
    else:                      # block r covers rows [r * rb, (r + 1) * rb) of the [M][N] output
        M = B * Ho * Wo
        # (a launch may own more blocks than ceil(M / rb) -- whole tiles, parity classes: those cover no row and must hold zeros)
        assert rb > 0 and st.row_blocks * rb >= M, (label, rb, st.row_blocks, M)
        flat = torch.zeros(st.row_blocks * rb, N, dtype=torch.float64)
        flat[:M] = yref.permute(0, 2, 3, 1).reshape(M, N)
        blk = flat.view(st.row_blocks, rb, N)
        eq(label + " row-block sum", rows[:, 0], blk.sum(1), names)
        eq(label + " row-block sum of squares", rows[:, 1], (blk * blk).sum(1), names)


# ---- dense convolutions: forward, dgrad, wgrad, dbias, statistics -------------------------------------------------------------------
def with_refs(d, label):
    """adds the float64 references of one dense convolution to its data, with the conditions for the strictest type"""
    x, w, b, gy = d["x"], d["w"], d["b"], d["gy"]
    st, pad, dil = d["geom"]
    B, C, H, W = x.shape
    N, _, R, S = w.shape
    d["y"] = checked(label + " y", cx.ref_forward(x, w, b, st, pad, dil), BF16, C * R * S + 1, stats=b is None)
    d["dx"] = checked(label + " dx", cx.ref_dgrad(x.shape, w, gy, st, pad, dil), BF16, N * R * S) if C != 3 else None
    d["dw"] = checked(label + " dw", cx.ref_wgrad(x, w.shape, gy, st, pad, dil), F32, gy[0, 0].numel() * B)
    if b is not None:         # the sum is exact; what the library owes is the mean-times-count expression (cx.ref_dbias_as_computed)
        checked(label + " db", cx.ref_dbias(gy), F32, gy[0, 0].numel() * B)
    d["db"] = cx.ref_dbias_as_computed(gy) if b is not None else None
    return d


@functools.lru_cache(maxsize=1)
def dense_ref(case):
    """data and references of one dense case, computed once and shared by the three types"""
    return with_refs(cx.dense_data(case), sid(case))


@functools.lru_cache(maxsize=1)
def c64_ref(case):
    B, C, H, W, N, dil, hb = case
    d = with_refs(cx.c64_data(case), sid(case))
    # (the bias-free forward of the same operands plus the addend: y without its bias, no second convolution)
    y0 = d["y"].double() - (d["b"].double().view(1, -1, 1, 1) if d["b"] is not None else 0.0)
    d["ya"] = checked(sid(case) + " addend form", y0 + d["addend"].double(), BF16, 9 * C + 1)
    return d


@functools.lru_cache(maxsize=1)
def pwk_ref(case):
    B, C, H, W, N = case
    d = with_refs(cx.pwk_data(case), sid(case))
    gate = cx.unpack_gate(d["gate_bits"], B, N, H, W)
    d["ya"] = checked(sid(case) + " addend form", d["y"].double() + d["addend"].double(), BF16, C + 1)
    d["yg"] = checked(sid(case) + " gated form", d["y"].double() + d["addend"].double() * gate.double(), BF16, C + 1)
    return d


def run_dense(case, T, r, second_backward=True, fuse_off=True):
    from mrfp_amd import conv
    st, pad, dil = r["geom"]
    label = "%s %s" % (sid(case), dname(T))
    stem = r["x"].shape[1] == 3
    xd = conv.pad_input_channels(r["x"].to(DEV), T) if stem else dev(r["x"], T, True)
    wd = r["w"].to(DEV).requires_grad_(True)
    bd = r["b"].to(DEV).requires_grad_(True) if r["b"] is not None else None
    gyd = dev(r["gy"], T)

    def run():
        y = conv.conv2d(xd, wd, bd, st, pad, dil)
        y.backward(gyd, retain_graph=second_backward)
        return y
    yd, names = hooked(run)
    assert yd.dtype == T and tuple(yd.shape) == tuple(r["y"].shape), (label, yd.dtype, tuple(yd.shape))
    eq(label + " y", yd, r["y"], names)
    if not stem:
        assert xd.grad.dtype == T
        eq(label + " dx", xd.grad, r["dx"], names)
    assert wd.grad.dtype == F32
    eq(label + " dw", wd.grad, r["dw"], names)
    if bd is not None:
        eq(label + " db", bd.grad, r["db"], names)
    else:
        check_colstats(label, yd, r["y"], names)
        if fuse_off:
            conv.FUSE_STATS[0] = False
            try:
                with torch.no_grad():
                    y2 = conv.conv2d(xd.detach(), wd.detach(), None, st, pad, dil)
            finally:
                conv.FUSE_STATS[0] = True
            assert getattr(y2, "_mrfp_colstats", None) is None
            assert torch.equal(y2, yd), (label, "the output depends on the statistics switch")
    if second_backward:
        # a second pass into the same .grad: the weight-gradient kernels run again and the sum must be exactly twice the reference
        _, names2 = hooked(lambda: yd.backward(gyd))
        eq(label + " dw after two passes", wd.grad, 2 * r["dw"], names2)
    return names


def typed(cases, big_types, shapes):
    """(case, type) pairs, the types varying fastest (one reference per case): every type for every case, except that the cases with
    an activation of 2^24 elements or more (cx.big) keep `big_types` only -- the file has to stay short, and bf16 is kept"""
    return [pytest.param(c, T, id="%s-%s" % (sid(c), dname(T))) for c in cases for T in TYPES if T in big_types or not cx.big(*shapes(c))]


def _dense_shapes(c):
    B, C, H, W, N, k, st, pad, dil, _ = c
    return (B, C, H, W), (B, N, cx.out_size(H, k, st, pad, dil), cx.out_size(W, k, st, pad, dil))


@pytest.mark.parametrize("case,T", typed(cx.CASES, (BF16,), _dense_shapes))
def test_conv_fwd_dgrad_wgrad_statistics(case, T):
    """conv.conv2d over all of CASES (the stem, bias, dilation above the image, stride-2 dgrad with class-major rows): y, dx, dw, db;
    the bias-free cases also their fused statistics (row blocks, per image, total) and y with the statistics switched off."""
    run_dense(case, T, dense_ref(case))


@pytest.mark.parametrize("T", TYPES, ids=dname)
def test_padded_logits_path(T):
    """final2 into the 32-channel padded score buffer (phys_out): the pad planes are exact zeros, everything else as above"""
    from mrfp_amd import conv
    case = next(c for c in cx.CASES if c[4] == 19)
    r = dense_ref(case)
    B, N, Ho, Wo = r["y"].shape
    xd, wd, bd = dev(r["x"], T, True), r["w"].to(DEV).requires_grad_(True), r["b"].to(DEV).requires_grad_(True)
    gy = torch.zeros(B, 32, Ho, Wo)
    gy[:, :N] = r["gy"]

    def run():
        p = conv.conv2d(xd, wd, bd, 1, 0, 1, phys_out=32)
        p.backward(dev(gy, T))
        return p
    p, names = hooked(run)
    assert tuple(p.shape) == (B, 32, Ho, Wo)
    eq("pad planes", p[:, N:], torch.zeros(B, 32 - N, Ho, Wo), names)
    eq("y", p[:, :N], r["y"], names)
    eq("dx", xd.grad, r["dx"], names)
    eq("dw", wd.grad, r["dw"], names)
    eq("db", bd.grad, r["db"], names)


# ---- weighted statistics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("case", cx.WSTAT_CASES, ids=lambda c: sid(c[:6]))
def test_resize_weighted_statistics(case, T):
    """conv2d(stat_resize=): the epilogue counts every output pixel as often as the nearest resize reads it (mrfp_conv_fwd_wstats).
    The multiplicities come from F.interpolate on an index image, not from the plan under test."""
    from mrfp_amd import conv, ops
    B, C, N, H, W, dil, rs = case
    kw = dict(scale_factor=rs["scale"]) if "scale" in rs else dict(size=rs["size"])
    idx = F.interpolate(torch.arange(H * W, dtype=torch.float64).view(1, 1, H, W), mode="nearest", **kw).long().view(-1)
    mult = torch.bincount(idx, minlength=H * W).view(H, W)
    d = cx.conv_data(B, C, H, W, N, 3, 1, dil, dil, True, cx.seed_of(case[:6]), stats=B * int(mult.sum()))
    y = checked(sid(case[:6]), cx.ref_forward(d["x"], d["w"], d["b"], 1, dil, dil), BF16, 9 * C + 1, stats=True, mult=mult)
    plan = ops.nearest_plan(H, W, device=DEV, **rs)
    hits = conv.WSTATS_HITS[0]
    yd, names = hooked(lambda: conv.conv2d(dev(d["x"], T), d["w"].to(DEV), d["b"].to(DEV), 1, dil, dil, stat_resize=plan))
    assert conv.WSTATS_HITS[0] == hits + 1 and "mrfp_conv_fwd_wstats" in names
    eq("y", yd, y, names)
    check_colstats("%s %s" % (sid(case[:6]), dname(T)), yd, y, names, mult=mult)


# ---- the weight-stationary 3x3 kernel and the long-K pointwise kernel ---------------------------------------------------------------
def run_c64(case, T):
    """forward (+ bias), statistics per image and total, dgrad, wgrad through conv.conv2d; the addend form through the C ABI"""
    from mrfp_amd import conv, _lib
    from mrfp_amd._lib import call, ptr, stream
    B, C, H, W, N, dil, hb = case
    r = c64_ref(case)
    run_dense(cx.c64_as_dense(case), T, r, second_backward=False)
    wdev = r["w"].to(DEV)
    pk = conv.get_pack(wdev, None, T, C, N)
    xd, addd = dev(r["x"], T), dev(r["addend"], T)
    out = torch.empty_like(addd)
    _, names = hooked(lambda: call("mrfp_conv_fwd", ptr(xd), ptr(pk.wf), None, ptr(out), _lib._DT[T], B, H, W, C, N, N, 3, 3, H, W, 1, dil, dil,
                                   dil, 1, ptr(addd), None, stream()))
    eq("%s %s addend form" % (sid(case), dname(T)), out, r["ya"], names)


# (these two lists exist for 16-bit kernels: their largest cases drop fp32, which only reaches the generic kernels of CASES)
@pytest.mark.parametrize("case,T", typed(cx.C64_CASES, (BF16, F16), lambda c: _dense_shapes(cx.c64_as_dense(c))))
def test_weight_stationary_3x3_kernel(case, T):
    if T != F32:
        from mrfp_amd import _lib
        B, C, H, W, N, dil, _ = case
        assert int(_lib.lib().mrfp_conv_stats_block_rows(_lib._DT[T], B, H, W, C, N, 3, 3, H, W, 1, dil, dil, dil, 1)) < 0      # this kernel
    run_c64(case, T)


@pytest.mark.parametrize("case,T", typed(cx.PWK_CASES, (BF16, F16), lambda c: _dense_shapes(cx.pwk_as_dense(c))))
def test_long_k_pointwise_kernel(case, T):
    """forward + statistics, dgrad, wgrad through conv.conv2d; the addend form and (16 bit: the entry point takes no fp32) the GATED
    addend form through the C ABI"""
    from mrfp_amd import conv, _lib
    from mrfp_amd._lib import call, ptr, stream
    B, C, H, W, N = case
    r = pwk_ref(case)
    add, ya, yg = r["addend"], r["ya"], r["yg"]
    run_dense(cx.pwk_as_dense(case), T, r, second_backward=False)
    wdev = r["w"].to(DEV)
    pk = conv.get_pack(wdev, None, T, C, N)
    xd, addd = dev(r["x"], T), dev(add, T)
    out = torch.empty_like(addd)
    label = "%s %s" % (sid(case), dname(T))
    _, names = hooked(lambda: call("mrfp_conv_fwd", ptr(xd), ptr(pk.wf), None, ptr(out), _lib._DT[T], B, H, W, C, N, N, 1, 1, H, W, 1, 0, 0, 1, 1,
                                   ptr(addd), None, stream()))
    eq(label + " addend form", out, ya, names)
    if T != F32:
        maskd = r["gate_bits"].to(DEV)
        out2 = torch.empty_like(addd)
        _, names = hooked(lambda: call("mrfp_conv_fwd_gated", ptr(xd), ptr(pk.wf), None, ptr(out2), _lib._DT[T], B, H, W, C, N, N, 1, 1, H, W,
                                       1, 0, 0, 1, 1, ptr(addd), ptr(maskd), stream()))
        eq(label + " gated addend form", out2, yg, names)


# ---- the head stand-in: shared pointwise pair + the low-rank skip gradient ----------------------------------------------------------
@functools.lru_cache(maxsize=1)
def head_ref():
    """the two-layer stand-in of tests/test_lowrank_skip_gpu.py (_head_inputs: same shapes): a 3x3 convolution 128 -> 64 with a skip alias,
    the shared 19-class pointwise classifier on a half-resolution partner and on the alias"""
    sd = cx.seed_of(("head",))
    t = dict(x=cx.ternary((2, 128, 20, 22), 32, sd), x1=cx.ternary((2, 128, 10, 11), 32, sd + 1), w3=cx.ternary((64, 128, 3, 3), 32, sd + 2),
             wf=cx.ternary((19, 128, 1, 1), 32, sd + 3), bf=cx.ternary((19,), 32, sd + 4), gy=cx.ternary((2, 64, 20, 22), 32, sd + 5),
             g1=cx.ternary((2, 32, 10, 11), 32, sd + 6), g2=cx.ternary((2, 32, 20, 22), 32, sd + 7))
    t["g1"][:, 19:] = 0          # (the pad planes of the score gradient are zero in the model)
    t["g2"][:, 19:] = 0
    g1, g2 = t["g1"][:, :19], t["g2"][:, :19]
    ref = dict(y=checked("head y", cx.ref_forward(t["x"], t["w3"], None, 1, 1, 1), BF16, 1152),
               p_low=checked("head p_low", cx.ref_forward(t["x1"], t["wf"]), BF16, 128),
               p_half=checked("head p_half", cx.ref_forward(t["x"], t["wf"], t["bf"]), BF16, 129),
               dx=checked("head dx", cx.ref_dgrad(t["x"].shape, t["w3"], t["gy"], 1, 1, 1) + cx.ref_dgrad(t["x"].shape, t["wf"], g2), BF16, 576 + 19),
               dx1=checked("head dx1", cx.ref_dgrad(t["x1"].shape, t["wf"], g1), BF16, 19),
               dw3=checked("head dw3", cx.ref_wgrad(t["x"], t["w3"].shape, t["gy"], 1, 1, 1), F32, 880),
               dwf=checked("head dwf", cx.ref_wgrad(t["x1"], t["wf"].shape, g1) + cx.ref_wgrad(t["x"], t["wf"].shape, g2), F32, 220 + 880),
               dbf=cx.ref_dbias_as_computed(g2))
    checked("head dbf", cx.ref_dbias(g2), F32, 880)
    return t, ref


@pytest.mark.parametrize("lowrank", [True, False], ids=["lowrank", "materialised"])
@pytest.mark.parametrize("T", TYPES, ids=dname)
def test_shared_pair_and_low_rank_skip_gradient(T, lowrank):
    """conv.shared_conv1x1_pair over two inputs, one of them a convolution's skip alias: both score maps, both input gradients, the
    shared weight and bias gradients.  16 bit with the switch on: the alias's gradient reaches the 3x3 dgrad as its two factors
    (mrfp_conv_fwd_lowrank, one hit); otherwise materialised and added by the epilogue.  The same reference either way."""
    from mrfp_amd import conv
    from mrfp_amd.network.mynn import HipConv2d
    t, ref = head_ref()
    conv.LOWRANK_SKIP[0] = lowrank
    try:
        x, x1 = dev(t["x"], T, True), dev(t["x1"], T, True)
        c3 = HipConv2d(128, 64, 3, padding=1, bias=False).to(DEV)
        c3.weight.data.copy_(t["w3"])
        wf, bf = t["wf"].to(DEV).requires_grad_(True), t["bf"].to(DEV).requires_grad_(True)
        hits = conv.LOWRANK_SKIP_HITS[0]

        def run():
            y, alias = c3.forward_skip(x)
            p_low, p_half = conv.shared_conv1x1_pair(x1, alias, wf, bf, 32)
            try:
                torch.autograd.backward([y, p_low, p_half], [dev(t["gy"], T), dev(t["g1"], T), dev(t["g2"], T)])
            except Exception:
                conv.backward_failed()
                raise
            return y, p_low, p_half
        (y, p_low, p_half), names = hooked(run)
    finally:
        conv.LOWRANK_SKIP[0] = True
    want = 1 if (lowrank and T != F32) else 0
    assert conv.LOWRANK_SKIP_HITS[0] - hits == want and ("mrfp_conv_fwd_lowrank" in names) == bool(want), names
    eq("y", y, ref["y"], names)
    eq("p_low", p_low[:, :19], ref["p_low"], names)
    eq("p_half", p_half[:, :19], ref["p_half"], names)
    eq("score pad planes", torch.cat([p_low[:, 19:].flatten(), p_half[:, 19:].flatten()]), torch.zeros(13 * (2 * 10 * 11 + 2 * 20 * 22)), names)
    eq("dx", x.grad, ref["dx"], names)
    eq("dx1", x1.grad, ref["dx1"], names)
    eq("dw3", c3.weight.grad, ref["dw3"], names)
    eq("dwf", wf.grad, ref["dwf"], names)
    eq("dbf", bf.grad, ref["dbf"], names)


def run_lowrank_kernel(case, T):
    """mrfp_conv_fwd_lowrank through the C ABI on a shape of tests/test_lowrank_skip_gpu.py: y = conv3x3(x) + round(dp . wf^T)"""
    from mrfp_amd import conv, _lib
    from mrfp_amd._lib import call, ptr, stream
    B, C, H, W, N, dil = case
    d = cx.lowrank_data(case)
    prod = checked(sid(case) + " product", torch.einsum("bkhw,nk->bnhw", d["dp"].double(), d["wf"].double()), BF16, 32)
    want = checked(sid(case) + " y", cx.ref_forward(d["x"], d["w"], None, 1, dil, dil, addend=prod), BF16, 9 * C + 32)
    dt_ = _lib._DT[T]
    assert int(_lib.lib().mrfp_conv_lowrank_ok(dt_, B, H, W, C, N, N, 3, 3, H, W, 1, dil, dil, dil)) == 1, case
    wdev = d["w"].to(DEV)
    pk = conv.get_pack(wdev, None, T, C, N)
    xd, dpd, wfd = dev(d["x"], T), dev(d["dp"], T), d["wf"].to(DEV, T).contiguous()
    y = dev(torch.full((B, N, H, W), float("nan")), T)
    _, names = hooked(lambda: call("mrfp_conv_fwd_lowrank", ptr(xd), ptr(pk.wf), None, ptr(y), dt_, B, H, W, C, N, N, 3, 3, H, W, 1, dil, dil, dil,
                                   1, None, None, ptr(dpd), ptr(wfd), 32, stream()))
    eq("%s %s low-rank form" % (sid(case), dname(T)), y, want, names)


# ---- grouped weight gradients -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def group_refs(case, Ct=None):
    B, C, H, W, N, k, st, pad, dil, n = case
    Ct = C if Ct is None else Ct
    out = []
    for i in range(n):
        x, gy = cx.group_data(case, i)
        out.append(checked("%s problem %d dw" % (sid(case), i), cx.ref_wgrad(x[:, :Ct], (N, Ct, k, k), gy, st, pad, dil), F32, gy[0, 0].numel() * B))
    return out


def run_group(case, T, Cp=None, Ct=None):
    """every problem of one grouped launch (a single launch for one problem) against ITS reference; operands as in
    test_grouped_wgrad_equals_the_single_launches (channel-padded NHWC buffers, pad channels zero)"""
    import test_conv_gpu as tcg
    from mrfp_amd import conv
    B, C, H, W, N, k, st, pad, dil, n = case
    Ct = C if Ct is None else Ct
    refs = group_refs(case, Ct)
    epc = 4 if T == F32 else 8
    Cp = Cp if Cp is not None else conv._round_up(C, 64 if C == 304 else epc)
    Np = conv._round_up(N, epc)
    Ho, Wo = cx.out_size(H, k, st, pad, dil), cx.out_size(W, k, st, pad, dil)
    xs, dys = [], []
    for i in range(n):
        x, gy = cx.group_data(case, i)
        xb = torch.zeros(B, H, W, Cp, device=DEV, dtype=T)
        xb[..., :Ct] = x[:, :Ct].permute(0, 2, 3, 1).to(DEV, T)
        gb = torch.zeros(B, Ho, Wo, Np, device=DEV, dtype=T)
        gb[..., :N] = gy.permute(0, 2, 3, 1).to(DEV, T)
        xs.append(xb.permute(0, 3, 1, 2))
        dys.append(gb.permute(0, 3, 1, 2))
    dws, names = hooked(lambda: tcg._wgrad_grouped(xs, dys, N, Ct, k, st, pad, dil) if n > 1 else [tcg._wgrad_single(xs[0], dys[0], N, Ct, k, st, pad, dil)])
    for i in range(n):
        eq("%s %s problem %d of %d dw" % (sid(case), dname(T), i, n), dws[i], refs[i], names)


@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("case", cx.GROUP_CASES, ids=sid)
def test_grouped_weight_gradients(case, T):
    run_group(case, T)


# ---- depthwise ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def dw_ref(case):
    B, C, H, W, s, dil = case
    d = cx.dw_data(case)
    x, w, b, gy = d["x"], d["w"], d["b"], d["gy"]
    label = sid(case)
    d["y"] = checked(label + " y", cx.ref_forward(x, w, None, s, dil, dil, groups=C), BF16, 9, stats=True)
    d["yb"] = checked(label + " y + bias", cx.ref_forward(x, w, b, s, dil, dil, groups=C), BF16, 10)
    d["y6"] = cx.ref_forward(x, w, b, s, dil, dil, groups=C, relu6=True)
    d["y1"] = cx.ref_forward(x, w, b, s, dil, dil, groups=C, relu=True)
    d["dx"] = checked(label + " dx", cx.ref_dgrad(x.shape, w, gy, s, dil, dil, groups=C), BF16, 9)
    d["dw"] = checked(label + " dw", cx.ref_wgrad(x, w.shape, gy, s, dil, dil, groups=C), F32, gy[0, 0].numel() * B)
    checked(label + " db", cx.ref_dbias(gy), F32, gy[0, 0].numel() * B)
    d["db"] = cx.ref_dbias_as_computed(gy)
    return d


@pytest.mark.parametrize("T", TYPES, ids=dname)
@pytest.mark.parametrize("case", cx.DW_CASES, ids=sid)
def test_depthwise(case, T):
    """mrfp_dwconv_fwd (with its fused statistics), _dgrad, _wgrad through ops.depthwise_conv2d; with a bias; _fwd_act with ReLU and ReLU6
    (exact on integers) and _dgrad over garbage pad channels through the C ABI"""
    from mrfp_amd import _lib, conv, ops
    B, C, H, W, s, dil = case
    r = dw_ref(case)
    label = "%s %s" % (sid(case), dname(T))
    Cp = conv._round_up(C, conv._epc(T))
    Ho, Wo = r["gy"].shape[2], r["gy"].shape[3]
    xd, wd, bd = dev(r["x"], T, True), r["w"].to(DEV).requires_grad_(True), r["b"].to(DEV).requires_grad_(True)
    gyd = dev(r["gy"], T)

    def run():
        y = ops.depthwise_conv2d(xd, wd, None, s, dil, dil)
        y.backward(gyd)
        yb = ops.depthwise_conv2d(xd.detach(), wd.detach(), bd, s, dil, dil)
        yb.backward(gyd)
        return y, yb
    (y, yb), names = hooked(run)
    assert y.dtype == T
    eq(label + " y", y, r["y"], names)
    eq(label + " dx", xd.grad, r["dx"], names)
    eq(label + " dw", wd.grad, r["dw"], names)
    eq(label + " y + bias", yb, r["yb"], names)
    eq(label + " db", bd.grad, r["db"], names)
    if Cp == C:
        st = y._mrfp_colstats
        assert st.elements == B * Ho * Wo and st.final.numel() == st.final_count * 2 * C
        tot = st.final.view(st.final_count, 2, C).double().sum(0).cpu()
        s_, q_ = cx.ref_stats(r["y"])
        eq(label + " sum", tot[0], s_.sum(0), names)
        eq(label + " sum of squares", tot[1], q_.sum(0), names)
    # the C ABI: padded buffers, pad channels of the inputs hold +-1 (they must not be read into a result)
    xb = cx.ternary((B, H, W, Cp), 48, cx.seed_of(case) + 8).to(DEV, T)
    xb[..., :C] = r["x"].permute(0, 2, 3, 1).to(DEV, T)
    w32, b32 = r["w"].to(DEV).contiguous(), r["b"].to(DEV).contiguous()
    for act, key in ((1, "y1"), (2, "y6")):
        out = torch.full((B, Ho, Wo, Cp), 7.0, device=DEV, dtype=T)
        _, names = hooked(lambda: _lib.call("mrfp_dwconv_fwd_act", xb.data_ptr(), w32.data_ptr(), b32.data_ptr(), out.data_ptr(), _lib._DT[T], B, H, W,
                                            Cp, C, Ho, Wo, s, dil, act, _lib.stream()))
        eq(label + " fwd_act %d" % act, out[..., :C].permute(0, 3, 1, 2), r[key], names)
        eq(label + " fwd_act %d pad channels" % act, out[..., C:], torch.zeros(B, Ho, Wo, Cp - C), names)
    dyb = cx.ternary((B, Ho, Wo, Cp), 48, cx.seed_of(case) + 9).to(DEV, T)
    dyb[..., :C] = r["gy"].permute(0, 2, 3, 1).to(DEV, T)
    dxb = torch.full((B, H, W, Cp), 7.0, device=DEV, dtype=T)
    _, names = hooked(lambda: _lib.call("mrfp_dwconv_dgrad", dyb.data_ptr(), w32.data_ptr(), dxb.data_ptr(), _lib._DT[T], B, H, W, Cp, C, Ho, Wo, s, dil,
                                        _lib.stream()))
    eq(label + " dgrad over padded buffers", dxb[..., :C].permute(0, 3, 1, 2), r["dx"], names)
    eq(label + " dgrad pad channels", dxb[..., C:], torch.zeros(B, H, W, Cp - C), names)


# ---- kernels that small shapes reach only behind a switch: one child process per switch set -----------------------------------------
def _child_main(name, out_path):
    kind, _env, shapes = cx.SWITCH_SETS[name]
    for sh in shapes:
        if kind == "dense":          # forward + statistics, dgrad, wgrad in bf16, as the existing children run these lists
            run_dense(sh, BF16, dense_ref(sh), second_backward=False, fuse_off=False)
        elif kind == "c64":          # the 128-channel weight-stationary kernel on small shapes, and the low-rank form on its shapes
            for T in (BF16, F16):
                run_c64(sh, T)
        else:
            case, Ct, T = cx.wgrad_child_case(kind, sh)
            run_group(case, T, Cp=case[1], Ct=Ct)
        print(sid(sh[:6]), "ok", flush=True)
    if kind == "c64":
        for case in cx.LOWRANK_CASES:
            for T in (BF16, F16):
                run_lowrank_kernel(case, T)
            print(sid(case), "low-rank ok", flush=True)
    torch.cuda.synchronize()
    json.dump(dict(entries=sorted(ENTRIES), kinds=sorted(k for k in KINDS if k is not None)), open(out_path, "w"))
    print("ok")


_CHILDREN = {}


def child(name, tmp_path_factory):
    """runs the switch set `name` in a child process, once per session -> dict(entries, kinds)"""
    if name not in _CHILDREN:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out = tmp_path_factory.mktemp("conv_exact") / (name + ".json")
        env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.path.join(root, "tests"), **cx.SWITCH_SETS[name][1])
        code = "import sys, test_conv_exact_gpu as t\nt._child_main(sys.argv[1], sys.argv[2])\n"
        r = subprocess.run([sys.executable, "-c", code, name, str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), (name, cx.SWITCH_SETS[name][1], r.stdout[-1500:], r.stderr[-4000:])
        _CHILDREN[name] = json.loads(out.read_text())
    return _CHILDREN[name]


@pytest.mark.parametrize("name", list(cx.SWITCH_SETS))
def test_switch_forced_kernels_in_subprocess(name, tmp_path_factory):
    """the generic kernels on pointwise shapes, the forced 96- and 192-row tiles, the K = 32 HALF variant, the row-reuse kernels, the
    128-channel weight-stationary kernel (with the low-rank form), the accumulator-stationary 3x3 and pointwise weight gradients, the
    256 x 128 wgrad tile: the same exact checks, in a child process with the switch set"""
    res = child(name, tmp_path_factory)
    print(name, "entry points:", res["entries"], "wgrad plan kinds (dtype, kernel, variant):", res["kinds"])
    want = {"wg3": 0, "wg1": 1, "big": 4}.get(cx.SWITCH_SETS[name][0])
    if want is not None:
        assert any(k[1] == want for k in res["kinds"]), (name, res["kinds"])


def test_wgrad_plan_kinds_cover_the_bench_layers(tmp_path_factory):
    """On the host: the (kernel, variant) pairs mrfp_conv_wgrad_plan returns over all the cases above -- at default switches for the
    in-process lists, as recorded at the launches of the children -- cover every pair it returns at default switches for the
    weight-gradient calls of the benchmark step (tests/golden/wgrad_plan.json: bench_calls, each in its own activation type)."""
    from mrfp_amd import conv
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    calls = json.load(open(os.path.join(root, "tests", "golden", "wgrad_plan.json")))["bench_calls"]
    print("entry points reached in this process so far:", sorted(ENTRIES))
    print("wgrad plan kinds launched in this process so far (dtype, kernel, variant):", sorted(k for k in KINDS if k is not None))
    mine = set()
    for name in cx.SWITCH_SETS:
        mine |= {tuple(k) for k in child(name, tmp_path_factory)["kinds"]}
    for T in TYPES:
        from mrfp_amd import _lib
        d, epc = _lib._DT[T], conv._epc(T)

        def add(B, C, H, W, N, k, st, pad, dil, n=1):
            Ho, Wo = cx.out_size(H, k, st, pad, dil), cx.out_size(W, k, st, pad, dil)
            Cp = conv._round_up(C, 64 if (C == 304 and n > 1) else epc)
            mine.add(wgrad_kind(d, B, H, W, Cp, N, conv._round_up(N, epc), k, k, Ho, Wo, st, pad, pad, dil, n))
        for c in cx.CASES:
            add(*c[:9])
        for c in cx.GROUP_CASES:
            add(*c)
        for c in cx.C64_CASES:
            add(*cx.c64_as_dense(c)[:9])
        for c in cx.PWK_CASES:
            add(*c, 1, 1, 0, 1)
    # (every bench call carries the activation type it was traced in)
    bench = {wgrad_kind(d, *g) for d, g in calls}
    assert None not in bench
    print("bench kinds", sorted(bench), "reached", sorted(k for k in mine if k is not None))
    assert bench <= mine, sorted(bench - mine)
