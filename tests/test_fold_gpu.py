"""Folded inference on the GPU (mrfp_amd/inference.py): the epilogue activation of every forward convolution family against
clamp(unfused launch) bit for bit, the fold pack against the fp32 product rounded once, folded model logits against the bars the
unfolded eval path is held to, launch accounting, no leak into training, invalidation, and the harness switches."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from mrfp_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def relerr(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- epilogue, bit-exact ---------------------------------------------------------------------------------------------------
# (name, B, H, W, C, N, k, stride, dil, bias) -- one shape per kernel family; the family a shape lands on is the launch plan's choice
CONV_CASES = [
    ("igemm_stride2", 2, 33, 35, 64, 96, 3, 2, 1, True),
    ("igemm_dilated_unaligned", 2, 24, 24, 96, 128, 3, 1, 3, True),
    ("c64_64ch", 2, 40, 48, 64, 64, 3, 1, 1, True),
    ("c64_128ch", 16, 256, 256, 128, 64, 3, 1, 2, True),          # (the 128-channel kernel takes launches of >= 8192 row strips)
    ("pw_k128", 2, 32, 32, 128, 256, 1, 1, 1, False),              # the pointwise kernels take bias-free launches
    ("pw_k256_bias_generic", 2, 32, 32, 256, 128, 1, 1, 1, True),
    ("pwk_k1024", 16, 48, 48, 1024, 256, 1, 1, 1, False),
    ("rr_row_reuse", 16, 96, 96, 256, 256, 3, 1, 1, True),
]


def _conv_pair(dtype, B, H, W, C, N, k, stride, dil, bias, ldy, addend, seed):
    from mrfp_amd import _lib
    from mrfp_amd._lib import call, ptr, stream
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32 and B * H * W > 40000:            # fp32 runs on the generic tiles anyway: a smaller batch will do
        B = max(1, 40000 // (H * W))
    x = torch.randn(B, H, W, C, generator=g).to(DEV, dtype)
    w = (torch.randn(N, C, k, k, generator=g) / (C * k * k) ** 0.5).to(DEV)
    bvec = (torch.randn(N, generator=g) * 2).to(DEV) if bias else None
    pad = dil * (k - 1) // 2
    Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    wf = torch.empty(N * k * k * C, dtype=dtype, device=DEV)
    call("mrfp_pack_weight", ptr(w), ptr(wf), None, _lib._DT[dtype], N, C, k, k, N, C, stream())
    # scale the input so that a good share of the outputs lies beyond 6, between 0 and 6, and below 0
    x = x * 4
    add = (torch.randn(B, Ho, Wo, ldy, generator=g) * 3).to(DEV, dtype) if addend else None
    outs = {}
    for act in (None, 0, 1, 2):
        y = torch.full((B, Ho, Wo, ldy), 7.5, dtype=dtype, device=DEV)      # a padded pitch keeps its sentinel
        if act is None:
            call("mrfp_conv_fwd", ptr(x), ptr(wf), ptr(bvec), ptr(y), _lib._DT[dtype], B, H, W, C, N, ldy, k, k, Ho, Wo, stride, pad, pad,
                 dil, 1, ptr(add), None, stream())
        else:
            call("mrfp_conv_fwd_act", ptr(x), ptr(wf), ptr(bvec), ptr(y), _lib._DT[dtype], B, H, W, C, N, ldy, k, k, Ho, Wo, stride, pad,
                 pad, dil, 1, ptr(add), act, stream())
        outs[act] = y
    torch.cuda.synchronize()
    return outs, N


@pytest.mark.parametrize("addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_epilogue_activation_is_clamp_of_the_plain_launch(case, dtype, addend):
    name, B, H, W, C, N, k, stride, dil, bias = case
    ldy = N + 16 if name in ("igemm_stride2", "pw_k256_bias_generic") else N          # a padded output pitch ldy > N
    outs, N = _conv_pair(dtype, B, H, W, C, N, k, stride, dil, bias, ldy, addend, seed=len(name) + 7 * addend)
    base = outs[None]
    assert torch.isfinite(base.float()).all()
    live = base[..., :N].float()
    assert (live > 6).float().mean() > 0.01 and (live < 0).float().mean() > 0.05 and ((live > 0) & (live < 6)).float().mean() > 0.05
    assert torch.equal(_bits(outs[0]), _bits(base)), "act = 0 is mrfp_conv_fwd"
    assert torch.equal(_bits(outs[1][..., :N]), _bits(torch.clamp(base[..., :N], min=0))), "ReLU"
    assert torch.equal(_bits(outs[2][..., :N]), _bits(torch.clamp(base[..., :N], min=0, max=6))), "ReLU6"
    if ldy > N:
        for a in (0, 1, 2):
            assert (outs[a][..., N:] == 7.5).all(), "the pitch padding is not written"


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_depthwise_epilogue_activation_is_clamp_of_the_plain_launch(dtype, stride):
    from mrfp_amd import _lib
    from mrfp_amd._lib import call, ptr, stream
    g = torch.Generator().manual_seed(11 + stride)
    B, H, W, C = 2, 37, 41, 96
    x = (torch.randn(B, H, W, C, generator=g) * 4).to(DEV, dtype)
    w = torch.randn(C, 1, 3, 3, generator=g).to(DEV)
    b = (torch.randn(C, generator=g) * 2).to(DEV)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    outs = {}
    for act in (None, 0, 1, 2):
        y = torch.empty(B, Ho, Wo, C, dtype=dtype, device=DEV)
        if act is None:
            call("mrfp_dwconv_fwd", ptr(x), ptr(w), ptr(b), ptr(y), _lib._DT[dtype], B, H, W, C, C, Ho, Wo, stride, 1, None, stream())
        else:
            call("mrfp_dwconv_fwd_act", ptr(x), ptr(w), ptr(b), ptr(y), _lib._DT[dtype], B, H, W, C, C, Ho, Wo, stride, 1, act, stream())
        outs[act] = y
    base = outs[None]
    assert (base.float() > 6).float().mean() > 0.01 and (base.float() < 0).float().mean() > 0.05
    assert torch.equal(_bits(outs[0]), _bits(base))
    assert torch.equal(_bits(outs[1]), _bits(torch.clamp(base, min=0)))
    assert torch.equal(_bits(outs[2]), _bits(torch.clamp(base, min=0, max=6)))


def test_activation_refuses_dgrad_launches():
    from mrfp_amd import _lib
    from mrfp_amd._lib import call, ptr, stream
    x = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device=DEV)
    wf = torch.zeros(64 * 64, dtype=torch.bfloat16, device=DEV)
    y = torch.zeros(1, 16, 16, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.MrfpHipError):
        call("mrfp_conv_fwd_act", ptr(x), ptr(wf), None, ptr(y), _lib.BF16, 1, 8, 8, 64, 64, 64, 1, 1, 16, 16, 1, 0, 0, 1, 2, None, 1, stream())
    with pytest.raises(_lib.MrfpHipError):
        call("mrfp_conv_fwd_act", ptr(x), ptr(wf), None, ptr(x), _lib.BF16, 1, 8, 8, 64, 64, 64, 1, 1, 8, 8, 1, 0, 0, 1, 1, None, 3, stream())


# ---- fold pack -------------------------------------------------------------------------------------------------------------
def _host_fold(w, cb, gamma, beta, mean, var, eps):
    """the fp32 expressions of the fold, on the host with torch: A = gamma * rsqrt(var + eps), S = beta - mean * A (+ A * conv bias).
    (torch.rsqrt, not 1 / torch.sqrt: the vectorised fp32 torch.sqrt of the host is not the correctly rounded square root -- it
    differs from the fp64 root rounded to fp32 in a fifth of the values -- while rsqrt and the device kernel both give the IEEE chain.)"""
    A = gamma * torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    S = beta - mean * A
    if cb is not None:
        S = S + A * cb
    return w * A.view(-1, 1, 1, 1), S


def _ulp_close(a, b):
    lo = torch.nextafter(b, torch.full_like(b, -float("inf")))
    hi = torch.nextafter(b, torch.full_like(b, float("inf")))
    return bool(((a >= lo) & (a <= hi)).all())


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_fold_pack_is_the_fp32_product_rounded_once(dtype, with_bias):
    from mrfp_amd import _lib
    from mrfp_amd._lib import call, ptr, stream
    g = torch.Generator().manual_seed(5)
    N, C, R = 70, 44, 3
    Npad, Cpad = 72, 48
    w = torch.randn(N, C, R, R, generator=g)
    cb = torch.randn(N, generator=g) if with_bias else None
    gamma, beta, mean = torch.randn(N, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g)
    var = torch.rand(N, generator=g) + 0.01
    var[:4] = torch.tensor([0.0, 1e-12, 1e-7, 1e-6])
    eps = 1e-5
    wf = torch.full((Npad * R * R * Cpad,), 3.0, dtype=dtype, device=DEV)
    S = torch.full((Npad,), 3.0, dtype=torch.float32, device=DEV)
    d = [t.to(DEV) if t is not None else None for t in (w, cb, gamma, beta, mean, var)]
    call("mrfp_pack_weight_folded", ptr(d[0]), ptr(wf), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), ptr(d[5]), eps, ptr(S),
         _lib._DT[dtype], N, C, R, R, Npad, Cpad, stream())
    wA, Sref = _host_fold(w, cb, gamma, beta, mean, var, eps)
    ref = torch.zeros(Npad, R, R, Cpad)
    ref[:N, :, :, :C] = wA.permute(0, 2, 3, 1)
    ref = ref.to(dtype)                                     # ONE rounding of the fp32 product
    assert torch.equal(_bits(wf.cpu().view(Npad, R, R, Cpad)), _bits(ref))
    assert _ulp_close(S[:N].cpu(), Sref) and (S[N:] == 0).all()
    # scaling the already rounded pack is a different (twice rounded) pack for the 16-bit types: the test can tell them apart
    if dtype != torch.float32:
        twice = (w.to(dtype).float() * (gamma * torch.rsqrt(var + eps)).view(-1, 1, 1, 1)).to(dtype)
        assert not torch.equal(twice, wA.to(dtype))


def _fold_pairs():
    """(conv, norm) x 3: 24 -> 40 3x3, depthwise 40 3x3, 40 -> 16 1x1 with a bias"""
    from mrfp_amd.network import mynn
    g = torch.Generator().manual_seed(9)
    mods = []
    for cin, cout, k, groups in ((24, 40, 3, 1), (40, 40, 3, 40), (40, 16, 1, 1)):
        c = mynn.HipConv2d(cin, cout, k, 1, k // 2, groups=groups, bias=(k == 1)).to(DEV)
        n = mynn.HipLocalBatchNorm2d(cout).to(DEV)
        with torch.no_grad():
            n.running_mean.copy_(torch.randn(cout, generator=g))
            n.running_var.copy_(torch.rand(cout, generator=g) + 0.05)
            n.weight.copy_(torch.randn(cout, generator=g))
            n.bias.copy_(torch.randn(cout, generator=g))
        mods.append((c, n))
    return mods


def test_fold_pack_batched_equals_single_and_depthwise_is_unrounded():
    from mrfp_amd import conv as conv_mod
    mods = _fold_pairs()
    items = []
    for c, n in mods:
        dw = c.groups != 1
        N, C = c.weight.shape[0], c.weight.shape[1]
        key = conv_mod._fold_key(c.weight, c.bias, n, torch.bfloat16, 1 if dw else C, N, dw)
        items.append((c.weight, c.bias, n, key))
    conv_mod.fold_packs_batched(items)
    for (c, n), it in zip(mods, items):
        pk = conv_mod._packs_of(c.weight).folded[it[3]]
        wA, S = _host_fold(c.weight.detach().cpu(), c.bias.detach().cpu() if c.bias is not None else None, n.weight.detach().cpu(),
                           n.bias.detach().cpu(), n.running_mean.cpu(), n.running_var.cpu(), n.eps)
        ref = wA.permute(0, 2, 3, 1).contiguous()
        if c.groups != 1:
            assert pk.wf.dtype == torch.float32 and torch.equal(pk.wf.cpu().view_as(ref), ref)        # fp32 taps, no rounding
        else:
            assert torch.equal(_bits(pk.wf.cpu().view_as(ref)), _bits(ref.to(torch.bfloat16)))
        assert _ulp_close(pk.bias.cpu(), S)


def test_a_stale_member_refolds_its_whole_registered_set_in_one_launch():
    """conv.get_folded_pack on a member of a registered set (conv.register_fold_set): ONE mrfp_pack_weights_folded_batched over
    every stale pack of the set -- three jobs here -- and no single launch; the other members then hit.  The same again after a
    bump of ops.RUNNING_STATS_EPOCH, whichever member is asked first.  A weight in no set takes one mrfp_pack_weight_folded.
    The set's packs equal those of three single launches bit for bit."""
    from mrfp_amd import _lib, ops
    from mrfp_amd import conv as conv_mod
    from mrfp_amd._lib import call, ptr, stream
    from mrfp_amd.inference import _FoldSet
    T = torch.bfloat16
    pairs = _FoldSet(_fold_pairs())
    lone = _fold_pairs()[0]
    conv_mod.register_fold_set(pairs)

    def get(c, n):
        dw = c.groups != 1
        N, C = c.weight.shape[0], c.weight.shape[1]
        assert N % 8 == 0 and (dw or C % 8 == 0)          # the set's standard geometry is the one asked for here
        return conv_mod.get_folded_pack(c.weight, c.bias, n, T, 1 if dw else C, N, depthwise=dw)

    launches = []
    prev = _lib.HOOK[0]
    _lib.HOOK[0] = lambda name, args: launches.append((name, args)) if name.startswith("mrfp_pack_weight") else None
    try:
        get(*pairs[0])
        assert [n for n, _ in launches] == ["mrfp_pack_weights_folded_batched"] and launches[0][1][2] == 3, launches
        packs = [get(c, n) for c, n in pairs]
        assert len(launches) == 1, launches
        ops.RUNNING_STATS_EPOCH[0] += 1
        get(*pairs[2])
        assert [n for n, _ in launches[1:]] == ["mrfp_pack_weights_folded_batched"] and launches[1][1][2] == 3, launches
        assert [get(c, n) for c, n in pairs] == packs and len(launches) == 2, launches
        get(*lone)
        assert [n for n, _ in launches[2:]] == ["mrfp_pack_weight_folded"], launches
        get(*lone)
        assert len(launches) == 3, launches
    finally:
        _lib.HOOK[0] = prev
    for (c, n), pk in zip(pairs, packs):
        dw = c.groups != 1
        N, C, R, S = c.weight.shape
        wf = torch.full_like(pk.wf, 3.0)
        bias = torch.full_like(pk.bias, 3.0)
        call("mrfp_pack_weight_folded", ptr(c.weight), ptr(wf), ptr(c.bias), ptr(n.weight), ptr(n.bias), ptr(n.running_mean),
             ptr(n.running_var), float(n.eps), ptr(bias), _lib.F32 if dw else _lib._DT[T], N, C, R, S, N, C, stream())
        assert pk.wf.dtype == (torch.float32 if dw else T)
        assert torch.equal(_bits(pk.wf), _bits(wf)) and torch.equal(_bits(pk.bias), _bits(bias)), tuple(c.weight.shape)


# ---- models ----------------------------------------------------------------------------------------------------------------
def _mrfp(trunk="resnet-50", dtype=torch.float32, seed=0):
    from mrfp_amd import deepv3
    from mrfp_amd.config import cfg
    cfg.MODEL.ACT_DTYPE = dtype
    m = _quiet(deepv3.MRFPPlus, 19, trunk=trunk, criterion=torch.nn.CrossEntropyLoss(ignore_index=255))
    sd = synth.synth_state_dict(synth.spec_of(m.state_dict()), seed=seed)
    m.load_state_dict(sd)
    return m.to(DEV), sd


def _eval(m, x, fold, **kw):
    from mrfp_amd.inference import fold_norms
    m.eval()
    with torch.no_grad():
        if fold:
            with fold_norms(m):
                return m(x, training=False, **kw)
        return m(x, training=False, **kw)


@pytest.fixture(autouse=True)
def _restore_dtype():
    from mrfp_amd.config import cfg
    yield
    cfg.MODEL.ACT_DTYPE = torch.float32


def test_folded_deepv3_golden_eval_logits():
    """the bars of tests/test_deepv3_gpu.py::test_golden_eval_logits, applied to the folded path"""
    import deepv3_common as dc
    from mrfp_amd.config import cfg
    from mrfp_amd.network import deepv3 as ndv3
    gold = np.load(dc.GOLDEN)
    for name in dc.CASES:
        sd, x, _, _ = dc.case_inputs(name)
        cfg.MODEL.ACT_DTYPE = torch.float32
        crit = torch.nn.CrossEntropyLoss(ignore_index=255)
        m = _quiet(getattr(ndv3, name), None, dc.NC, crit, crit)
        m.load_state_dict(sd)
        m = m.to(DEV)
        logits = _eval(m, x.to(DEV), True)
        p = name + "/"
        assert logits.shape == (dc.B, dc.NC, dc.S, dc.S) and logits.dtype == torch.float32
        np.testing.assert_allclose(dc.stats(logits), gold[p + "eval_logits_stats"], rtol=1e-3)
        assert relerr(logits[:, :4, 60:64, 60:64], gold[p + "eval_logits_crop"]) < 1e-3, name


def test_folded_mrfp_r50_eval_logits_vs_cpu_oracle():
    from oracle import mrfp_oracle as orc
    m, sd = _mrfp("resnet-50")
    x, _ = synth.synth_batch(2, 128, 128, seed=3)
    ref = orc.mrfp_forward({k: v.clone() for k, v in sd.items()}, x, training=False, bn_train=False)
    got = _eval(m, x.to(DEV), True)
    assert relerr(got, ref) < 1e-3
    assert relerr(_eval(m, x.to(DEV), False), ref) < 1e-3


@pytest.mark.parametrize("which", ["mrfp-r101", "simple"])
def test_folded_fp32_eval_logits_vs_unfolded(which):
    from mrfp_amd import deepv3
    from mrfp_amd.config import cfg
    if which == "mrfp-r101":
        m, _ = _mrfp("resnet-101")
    else:
        cfg.MODEL.ACT_DTYPE = torch.float32
        m = _quiet(deepv3.simpleDeepV3Plus, 19)
        m.load_state_dict(synth.synth_state_dict(synth.spec_of(m.state_dict()), seed=0))
        m = m.to(DEV)
    x, _ = synth.synth_batch(2, 192, 192, seed=5)
    plain = _eval(m, x.to(DEV), False)
    folded = _eval(m, x.to(DEV), True)
    assert relerr(folded, plain) < 1e-3
    assert torch.equal(_eval(m, x.to(DEV), False), plain)            # leaving the context restores the ordinary path bit for bit


def _l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).sum().sqrt() / b.pow(2).sum().sqrt()).item()


# k of the bf16 bar (see the docstring below; tools/fold_yardstick_seeds.py measures it)
BF16_K = 1.46


def test_folded_bf16_logits_are_no_further_from_fp32_than_unfolded_bf16():
    """e_plain = |bf16 unfolded - fp32 unfolded|, e_fold = |bf16 folded - fp32 unfolded| (relative L2 over the eval logits of
    MRFPPlus('resnet-50'), 2 x 256 x 256); the bar is e_fold <= k * e_plain -- the yardstick is the unfolded bf16 path, not the code
    under test.  k = the worst e_fold / e_plain ratio over the seeds of tools/fold_yardstick_seeds.py (weights and batch re-drawn per
    seed) plus the seed-to-seed spread of e_plain, (max - min) / mean.  Measured on an MI355X, seeds 0..7 (profiles/fold_eval.md):
    e_plain 1.44e-2 .. 2.47e-2 (mean 2.00e-2, spread 0.515), e_fold 1.31e-2 .. 2.24e-2, ratio 0.899 .. 0.949 -- folding removes one
    rounding per layer, so the folded logits sit CLOSER to fp32 on every seed -- k = 0.949 + 0.515 = 1.46."""
    x, _ = synth.synth_batch(2, 256, 256, seed=101)
    m32, sd = _mrfp("resnet-50", torch.float32, seed=1)
    ref = _eval(m32, x.to(DEV), False)
    del m32
    m16, _ = _mrfp("resnet-50", torch.bfloat16, seed=1)
    plain = _eval(m16, x.to(DEV), False)
    folded = _eval(m16, x.to(DEV), True)
    e_plain, e_fold = _l2(plain, ref), _l2(folded, ref)
    print("bf16 fidelity: e_plain %.4e  e_fold %.4e  ratio %.3f  (k = %.2f)" % (e_plain, e_fold, e_fold / e_plain, BF16_K))
    assert e_fold <= BF16_K * e_plain, (e_fold, e_plain)


def _eval_batches():
    x, y = synth.synth_batch(2, 256, 256, seed=1)        # the synthetic eval batches of tests/test_harness_gpu.py
    return [(x[i:i + 1].to(DEV), y[i:i + 1].to(DEV)) for i in range(2)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_harness_fold_switches(dtype):
    from mrfp_amd import harness
    m, _ = _mrfp("resnet-50", dtype)
    batches = _eval_batches()
    h0, miou0, _ = harness.evaluate(m, batches)
    h1, miou1, _ = harness.evaluate(m, batches, fold=True)
    print("evaluate mIoU: plain %.4f folded %.4f" % (100 * miou0, 100 * miou1))
    assert abs(100 * miou1 - 100 * miou0) < 0.1
    h2, miou2, _ = harness.evaluate(m, batches, fold=False)
    assert np.array_equal(h0, h2) and miou0 == miou2                  # fold=False is the path it always was; nothing stays enabled
    t0 = harness.evaluate_tta(m, batches, scales=(0.75, 1.0), flip=True)
    t1 = harness.evaluate_tta(m, batches, scales=(0.75, 1.0), flip=True, fold=True)
    print("evaluate_tta mIoU: plain %.4f folded %.4f" % (100 * t0[1], 100 * t1[1]))
    assert abs(100 * t1[1] - 100 * t0[1]) < 0.1
    t2 = harness.evaluate_tta(m, batches, scales=(0.75, 1.0), flip=True)
    assert np.array_equal(t0[0], t2[0])


# ---- launch accounting -------------------------------------------------------------------------------------------------------
def _record(m, x, fold):
    from mrfp_amd import _lib
    calls = []
    prev = _lib.HOOK[0]
    _lib.HOOK[0] = lambda name, args: calls.append((name, args))
    try:
        _eval(m, x, fold)
    finally:
        _lib.HOOK[0] = prev
    return calls


def test_launch_accounting_of_a_folded_forward():
    from mrfp_amd import _lib
    from mrfp_amd.network import mynn
    m, _ = _mrfp("resnet-50", torch.bfloat16)
    x = synth.synth_batch(2, 256, 256, seed=2)[0].to(DEV)
    _eval(m, x, True)                       # packs exist from here on
    plain, folded = _record(m, x, False), _record(m, x, True)
    names = [n for n, _ in folded]
    assert "mrfp_bn_eval_coef" not in names and "mrfp_bn_finalize" not in names
    n_in = sum(1 for mod in m.modules() if isinstance(mod, mynn.HipInstanceNorm2d))
    affine = [n for n in names if n.startswith("mrfp_affine_fwd")]
    assert len(affine) <= n_in, (affine, n_in)          # the only apply passes left belong to InstanceNorm layers
    conv_names = ("mrfp_conv_fwd", "mrfp_conv_fwd_act", "mrfp_conv_fwd_wstats", "mrfp_dwconv_fwd", "mrfp_dwconv_fwd_act")
    n_plain = sum(1 for n, _ in plain if n in conv_names)
    n_fold = sum(1 for n in names if n in conv_names)
    assert n_fold == n_plain - 8, (n_fold, n_plain)      # the unfolded forward's convolutions minus the eight HRFP ones
    assert names.count("mrfp_conv_fwd_act") == 61        # one launch per folded pair
    # no launch carries an HRFP shape: their resized maps (1.205 x, 1.2 x ... of the stem's 64 x 64) exist nowhere else in the network
    arg = _lib.ARG_NAMES["mrfp_conv_fwd_act"]
    iH, iW = arg.index("H"), arg.index("W")
    stem = 256 // 4
    hrfp_sizes = {int(stem * 1.205), int(int(stem * 1.205) * 1.2)}
    for n, a in folded:
        if n in ("mrfp_conv_fwd", "mrfp_conv_fwd_act", "mrfp_conv_fwd_wstats"):
            assert a[iH] not in hrfp_sizes and a[iW] not in hrfp_sizes, (n, a[iH], a[iW])
    assert not any(n in ("mrfp_pack_weight_folded", "mrfp_pack_weights_folded_batched") for n in names)      # the packs are cached


# ---- no leak into training ---------------------------------------------------------------------------------------------------
def test_an_enabled_fold_does_not_leak_into_training():
    from mrfp_amd.inference import fold_norms
    x, y = synth.synth_batch(2, 128, 128, seed=3)
    x, y = x.to(DEV), y.to(DEV)
    noise = {k: v.to(DEV) for k, v in synth.synth_noise(2, seed=4).items()}
    results = []
    for folded in (False, True):
        m, _ = _mrfp("resnet-50", torch.bfloat16)
        if folded:
            fold_norms(m).enable()                     # folded, evaluated, and LEFT enabled
            m.eval()
            with torch.no_grad():
                m(x, training=False)
        m.train()
        from mrfp_amd import deepv3
        m.rng = deepv3.InjectedRandom((True, True, True), noise)
        loss = m(x, y, training=True)
        loss.backward()
        from mrfp_amd import conv as conv_mod
        conv_mod.flush_wgrads()
        conv_mod.join_wgrad_stream()
        torch.cuda.synchronize()
        results.append((loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None},
                        {k: b.clone() for k, b in m.named_buffers()}))
    (l0, g0, b0), (l1, g1, b1) = results
    assert torch.equal(l0, l1)
    assert set(g0) == set(g1) and len(g0) > 100
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for k in b0:
        assert torch.equal(b0[k], b1[k]), k


# ---- invalidation ------------------------------------------------------------------------------------------------------------
def test_folded_packs_follow_load_state_dict_and_a_trainer_step():
    from mrfp_amd import deepv3
    from mrfp_amd.harness import Trainer
    from mrfp_amd.inference import fold_norms
    x, y = synth.synth_batch(2, 128, 128, seed=3)
    x, y = x.to(DEV), y.to(DEV)
    m, _ = _mrfp("resnet-50", torch.bfloat16, seed=0)
    fold_norms(m).enable()
    first = _eval(m, x, True)
    # other running statistics AND other weights
    sd2 = synth.synth_state_dict(synth.spec_of(m.state_dict()), seed=7)
    m.load_state_dict(sd2)
    second = _eval(m, x, True)
    fresh, _ = _mrfp("resnet-50", torch.bfloat16, seed=7)
    assert torch.equal(second, _eval(fresh, x, True))
    assert not torch.equal(second, first)
    # one optimizer step on both (the fused SGD kernel and the training-mode BatchNorms rewrite everything through raw pointers)
    noise = {k: v.to(DEV) for k, v in synth.synth_noise(2, seed=4).items()}
    outs = []
    for model in (m, fresh):
        model.train()
        model.rng = deepv3.InjectedRandom((True, True, True), noise)
        Trainer(model, lr=1e-2).step(x, y)
        outs.append(_eval(model, x, True))
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], second)
    never, _ = _mrfp("resnet-50", torch.bfloat16, seed=7)            # ... and equal to a model that is folded for the first time now
    never.train()
    never.rng = deepv3.InjectedRandom((True, True, True), noise)
    Trainer(never, lr=1e-2).step(x, y)
    assert torch.equal(_eval(never, x, True), outs[0])
