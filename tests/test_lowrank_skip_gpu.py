"""The low-rank epilogue operand of the weight-stationary 3x3 kernel (mrfp_conv_fwd_lowrank, csrc/conv_c64.hip) and the operator
protocol that feeds it (conv.py: _SharedConv1x1Pair.backward -> _Conv2d.backward): the input gradient of the shared pointwise
classifier on a convolution's skip alias is never written, the dgrad multiplies its two factors in registers.

The training step must compute what it computed with the materialised gradient, so the kernel keeps that path's arithmetic: the
rank-32 product is rounded to the 16-bit type (as the pointwise dgrad launch that wrote the tensor did) and then added to the fp32
accumulators, which are rounded on store.  Every case is therefore held to BIT EQUALITY with the two-launch addend form
(mrfp_conv_fwd 1x1, then mrfp_conv_fwd with the addend), and against float64, per element, no element exempt (operands already
rounded to the 16-bit type):
    |y - ref| <= u * |ref| + (K + 2) * 2^-24 * S  [+ u * (1 + u) * |dP . Wf|],   u = 2^-8 (bf16) / 2^-11 (f16),  K = 9 * C + 32,
    S = the same expression as ref on absolute values.
u * |ref| is the rounding of the stored value; an fp32 sum of K products of exactly representable 16-bit pairs carries at most K
roundings of 2^-24 relative to the running sum of magnitudes, + 2 for the initial accumulator and the final conversion.  The term in
brackets is the rounding of the product (then scaled by at most 1 + u in the final rounding); it applies to the `dense` variant alone:
in `full` the score gradient is +-2^e on one class per pixel, so dP . Wf is a scaled row of Wf and exact in the 16-bit type; with the
3x3 weights zero (`lowrank_only`, dense dP) the second rounding is exact; with dP = 0 (`conv_only`) the product is zero.
"""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, C, H, W, N, dil): the smallest shapes that reach every path of the kernel
KERNEL_CASES = [
    (2, 128, 19, 23, 256, 2),      # both column groups, ragged strip, both dilation classes, odd H
    (2, 128, 20, 70, 256, 1),      # two strips, tail
    (1, 128, 9, 130, 128, 1),      # single column group
    (2, 64, 19, 23, 128, 2),       # CB = 1
    (3, 64, 10, 140, 64, 1),       # N = 64
]
DTYPES = {"bf16": (torch.bfloat16, 2.0 ** -8), "f16": (torch.float16, 2.0 ** -11)}
VARIANTS = ("full", "conv_only", "lowrank_only", "dense")      # dP = 0 / the 3x3 weights = 0: each term alone under the same bound


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _kernel_case(case, dname, variant):
    """-> (worst |y - ref| / bound over all elements, repeated launches bit-identical and equal to the two-launch addend form)"""
    from mrfp_amd import conv, _lib
    from mrfp_amd._lib import call, ptr, stream
    B, C, H, W, N, dil = case
    dtype, u = DTYPES[dname]
    g = torch.Generator().manual_seed(1000 * H + 10 * W + C + N)
    x = torch.randn(B, C, H, W, generator=g).to(dtype)
    w = (torch.randn(N, C, 3, 3, generator=g) * 0.04).to(dtype)
    dp = torch.randn(B, 32, H, W, generator=g).to(dtype)
    wf = (torch.randn(N, 32, generator=g) * 0.2).to(dtype)
    if variant == "full":          # +-2^e on one class per pixel (every plane occurs): the product is exact in the 16-bit type
        k = torch.randint(0, 32, (B, 1, H, W), generator=g)
        v = torch.randint(-3, 1, (B, 1, H, W), generator=g).float().exp2() * (2 * torch.randint(0, 2, (B, 1, H, W), generator=g) - 1)
        dp = torch.zeros(B, 32, H, W).scatter_(1, k, v).to(dtype)
    if variant == "conv_only":
        dp = torch.zeros_like(dp)
    if variant == "lowrank_only":
        w = torch.zeros_like(w)
    x64, w64, dp64, wf64 = x.double(), w.double(), dp.double(), wf.double()
    ref = F.conv2d(x64, w64, None, 1, dil, dil) + torch.einsum("bkhw,nk->bnhw", dp64, wf64)
    S = F.conv2d(x64.abs(), w64.abs(), None, 1, dil, dil) + torch.einsum("bkhw,nk->bnhw", dp64.abs(), wf64.abs())
    bound = u * ref.abs() + (9 * C + 32 + 2) * 2.0 ** -24 * S
    if variant == "dense":
        bound = bound + u * (1 + u) * torch.einsum("bkhw,nk->bnhw", dp64, wf64).abs()
    xd, dpd, wfd = _cl(x.to(DEV)), _cl(dp.to(DEV)), wf.to(DEV).contiguous()
    wdev = w.float().to(DEV)          # (the 16-bit pack of this master is `w` exactly)
    pk = conv.get_pack(wdev, None, dtype, C, N)
    d = _lib._DT[dtype]
    assert int(_lib.lib().mrfp_conv_lowrank_ok(d, B, H, W, C, N, N, 3, 3, H, W, 1, dil, dil, dil)) == 1, case
    outs = []
    for _ in range(3):
        y = _cl(torch.full((B, N, H, W), float("nan"), dtype=dtype, device=DEV))
        call("mrfp_conv_fwd_lowrank", ptr(xd), ptr(pk.wf), None, ptr(y), d, B, H, W, C, N, N, 3, 3, H, W, 1, dil, dil, dil, 1,
             None, None, ptr(dpd), ptr(wfd), 32, stream())
        outs.append(y)
    # the addend form: the product as a tensor (pointwise launch; lr_w is that launch's forward-form pack [N][1][1][32]), then added
    prod, two = torch.empty_like(outs[0]), torch.empty_like(outs[0])
    call("mrfp_conv_fwd", ptr(dpd), ptr(wfd), None, ptr(prod), d, B, H, W, 32, N, N, 1, 1, H, W, 1, 0, 0, 1, 1, None, None, stream())
    call("mrfp_conv_fwd", ptr(xd), ptr(pk.wf), None, ptr(two), d, B, H, W, C, N, N, 3, 3, H, W, 1, dil, dil, dil, 1, ptr(prod), None,
         stream())
    outs.append(two)
    err = (outs[0].double().cpu() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
    if bool(((bound == 0) & (err > 0)).any()) or not bool(torch.isfinite(outs[0]).all()):
        ratio = float("inf")
    return ratio, all(torch.equal(outs[0], o) for o in outs[1:])


def _child_main(out_path):
    res = {}
    for dname in DTYPES:
        for case in KERNEL_CASES:
            for variant in VARIANTS:
                ratio, same = _kernel_case(case, dname, variant)
                key = "%s|%s|%s" % (dname, "x".join(map(str, case)), variant)
                print(key, "worst err / bound = %.4f" % ratio, "bit-identical" if same else "NOT BIT-IDENTICAL", flush=True)
                res[key] = [ratio, same]
    torch.cuda.synchronize()
    json.dump(res, open(out_path, "w"))
    print("ok")


@pytest.fixture(scope="module")
def kernel_results(tmp_path_factory):
    """Every kernel case in ONE child process with MRFP_CONV_C128=2 (the switch is read once per process: the small 128-channel shapes
    otherwise stay on the implicit-GEMM tiles)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path_factory.mktemp("lowrank") / "kernel.json"
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.path.join(root, "tests"), MRFP_CONV_C128="2")
    code = "import sys, test_lowrank_skip_gpu as t\nt._child_main(sys.argv[1])\n"
    r = subprocess.run([sys.executable, "-c", code, str(out)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-1500:], r.stderr[-2000:])
    return json.loads(out.read_text())


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dname", list(DTYPES))
def test_kernel_against_fp64(kernel_results, dname, case, variant):
    ratio, same = kernel_results["%s|%s|%s" % (dname, "x".join(map(str, case)), variant)]
    print("worst |y - ref| / bound = %.4f" % ratio)
    assert ratio <= 1.0, ratio
    assert same, "repeated launches or the two-launch addend form differ"


# ---- refusals: an error, and nothing launched (the output keeps its fill) ---------------------------------------------------------
def _refusal_operands(dtype=torch.bfloat16, C=64, N=128, dil=2):
    from mrfp_amd import conv
    B, H, W = 2, 19, 23
    g = torch.Generator().manual_seed(5)
    x = _cl(torch.randn(B, C, H, W, generator=g).to(DEV, dtype))
    w = (torch.randn(N, C, 3, 3, generator=g) * 0.05).to(DEV)
    dp = _cl(torch.randn(B, 32, H, W, generator=g).to(DEV, dtype))
    wf = torch.randn(N, 32, generator=g).to(DEV, dtype)
    pk = conv.get_pack(w, None, dtype, C, N)
    y = _cl(torch.full((B, N, H, W), 7.0, dtype=dtype, device=DEV))
    return (B, C, H, W, N, dil), x, pk, dp, wf, y


def _refused(geom, x, pk, dp, wf, y, d, lr_k=32, addend=None):
    from mrfp_amd import _lib
    from mrfp_amd._lib import ptr, stream
    B, C, H, W, N, dil = geom
    with pytest.raises(_lib.MrfpHipError):
        _lib.call("mrfp_conv_fwd_lowrank", ptr(x), ptr(pk.wf), None, ptr(y), d, B, H, W, C, N, N, 3, 3, H, W, 1, dil, dil, dil, 1,
                  ptr(addend), None, ptr(dp), ptr(wf), lr_k, stream())
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()), "a refused call launched something"


def test_refusals():
    from mrfp_amd import _lib
    geom, x, pk, dp, wf, y = _refusal_operands()
    B, C, H, W, N, dil = geom
    ok = _lib.lib().mrfp_conv_lowrank_ok
    assert int(ok(_lib.BF16, B, H, W, C, N, N, 3, 3, H, W, 1, dil, dil, dil)) == 1
    _refused(geom, x, pk, dp, wf, y, _lib.BF16, lr_k=16)
    _refused(geom, x, pk, dp, wf, y, _lib.BF16, lr_k=64)
    _refused(geom, x, pk, dp, wf, y, _lib.BF16, addend=torch.zeros_like(y))
    # fp32
    assert int(ok(_lib.F32, B, H, W, C, N, N, 3, 3, H, W, 1, dil, dil, dil)) == 0
    g32 = _refusal_operands(torch.float32)
    _refused(*g32, _lib.F32)
    # shapes the launch plan does not send to the weight-stationary kernel: dilation 3, 96 input channels, a small 128-channel launch
    for kw in (dict(dil=3), dict(C=96), dict(C=128, N=256)):
        gq = _refusal_operands(**kw)
        Bq, Cq, Hq, Wq, Nq, dq = gq[0]
        assert int(ok(_lib.BF16, Bq, Hq, Wq, Cq, Nq, Nq, 3, 3, Hq, Wq, 1, dq, dq, dq)) == 0, kw
        _refused(*gq, _lib.BF16)
    # ... and the valid call still runs
    _lib.call("mrfp_conv_fwd_lowrank", x.data_ptr(), pk.wf.data_ptr(), None, y.data_ptr(), _lib.BF16, B, H, W, C, N, N, 3, 3, H, W,
              1, dil, dil, dil, 1, None, None, dp.data_ptr(), wf.data_ptr(), 32, _lib.stream())
    torch.cuda.synchronize()
    assert not bool((y == 7.0).all())


# ---- the autograd path: a two-layer stand-in for the MRFP+ head ---------------------------------------------------------------------
def _head_inputs(dtype=torch.bfloat16, onehot=False, x_grad=True):
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    t = dict(x=rnd(2, 128, 20, 22), x1=rnd(2, 128, 10, 11), w3=rnd(64, 128, 3, 3) * 0.04, wf=rnd(19, 128, 1, 1) * 0.2,
             bf=rnd(19) * 0.1, gy=rnd(2, 64, 20, 22), g1=rnd(2, 32, 10, 11), g2=rnd(2, 32, 20, 22))
    if onehot:
        # the score gradient of every pixel is +-2^e on ONE class: dP . Wf is then a scaled row of Wf, exact in the 16-bit type
        k = torch.randint(0, 19, (2, 1, 20, 22), generator=g)
        v = torch.randint(-3, 1, (2, 1, 20, 22), generator=g).float().exp2() * (2 * torch.randint(0, 2, (2, 1, 20, 22), generator=g) - 1)
        t["g2"] = torch.zeros(2, 32, 20, 22).scatter_(1, k, v)
    t["g1"][:, 19:] = 0        # (the pad planes of the score gradient are zero in the model; the pack's pad columns are zero anyway)
    t["g2"][:, 19:] = 0
    for k in ("x", "x1", "gy", "g1", "g2"):
        t[k] = _cl(t[k].to(dtype))
    for k in ("w3", "wf"):
        t[k] = t[k].to(dtype).float()       # masters that the 16-bit pack represents exactly
    t["x_grad"] = x_grad
    return t


def _head_run(t, lowrank, second_consumer=None, measure=False):
    """forward_skip 3x3 conv 128 -> 64, then the shared pointwise pair on a half-resolution partner and the alias; returns the
    gradients (x, x1, w3, wf, bf), the hit count and the peak of allocated bytes inside backward."""
    from mrfp_amd import conv
    from mrfp_amd.network.mynn import HipConv2d
    conv.LOWRANK_SKIP[0] = lowrank
    try:
        x = t["x"].to(DEV).requires_grad_(t["x_grad"])
        x1 = t["x1"].to(DEV).requires_grad_(True)
        c3 = HipConv2d(128, 64, 3, padding=1, bias=False).to(DEV)
        c3.weight.data.copy_(t["w3"])
        wf = t["wf"].to(DEV).requires_grad_(True)
        bf = t["bf"].to(DEV).requires_grad_(True)
        y, alias = c3.forward_skip(x)
        p_low, p_half = conv.shared_conv1x1_pair(x1, alias, wf, bf, 32)
        outs, grads = [y, p_low, p_half], [t["gy"].to(DEV), t["g1"].to(DEV), t["g2"].to(DEV)]
        if second_consumer is not None:
            z = second_consumer(alias)
            outs.append(z)
            grads.append(torch.ones_like(z))
        hits = conv.LOWRANK_SKIP_HITS[0]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        try:
            torch.autograd.backward(outs, grads)
        except Exception:
            conv.backward_failed()
            raise
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        res = dict(x=x.grad, x1=x1.grad, w3=c3.weight.grad, wf=wf.grad, bf=bf.grad)
        return res, conv.LOWRANK_SKIP_HITS[0] - hits, peak
    finally:
        conv.LOWRANK_SKIP[0] = True


def _x_grad_bound(t, u):
    """(float64 input gradient of the stand-in, the per-element kernel bound for it, |g2 . Wf|): the dgrad is a 3x3 convolution of gy with the
    flipped, transposed weight (C = 64 dgrad input channels: K = 9 * 64 + 32) plus g2 . Wf"""
    gy, g2, w3, wf = t["gy"].double(), t["g2"].double()[:, :19], t["w3"].double(), t["wf"].double()[:, :, 0, 0]
    wt = w3.flip(2, 3).transpose(0, 1)
    prod = torch.einsum("bkhw,kc->bchw", g2, wf)
    ref = F.conv2d(gy, wt, None, 1, 1, 1) + prod
    S = F.conv2d(gy.abs(), wt.abs(), None, 1, 1, 1) + torch.einsum("bkhw,kc->bchw", g2.abs(), wf.abs())
    return ref, u * ref.abs() + (9 * 64 + 32 + 2) * 2.0 ** -24 * S, prod.abs()


def test_autograd_hit_memory_and_gradients():
    """Switch on: one hit, one tensor of the alias's size fewer inside backward; on against off: every gradient EQUAL, the input
    gradient included (which is inside "twice the bound" with room to spare: the kernel keeps the materialised path's arithmetic).
    Against float64: a score gradient of +-2^e on one class per pixel (dP . Wf exact in the 16-bit type) under the kernel bound, dense
    random operands under the bound with the product's own rounding added (module docstring)."""
    t = _head_inputs()
    _head_run(t, True)
    _head_run(t, False)        # (both paths once before measuring: the weight-gradient workspace is grown on first use)
    on, hits_on, peak_on = _head_run(t, True)
    off, hits_off, peak_off = _head_run(t, False)
    assert hits_on == 1 and hits_off == 0
    alias_bytes = t["x"].numel() * 2
    print("peak bytes allocated in backward: on %d, off %d, alias %d" % (peak_on, peak_off, alias_bytes))
    # (the stand-in is a scalar: one 512-byte block of the caching allocator in place of the alias-sized tensor)
    assert peak_off - peak_on >= alias_bytes - 512
    u = 2.0 ** -8
    ref, bound, prod = _x_grad_bound(t, u)
    err = (on["x"].double().cpu() - ref).abs()
    dense = bound + u * (1 + u) * prod
    print("dense operands: worst |dx - ref| / bound = %.4f" % float((err / dense).max()))
    assert bool((err <= dense).all())
    for k in ("x", "w3", "wf", "bf", "x1"):
        assert torch.equal(on[k], off[k]), k
    tp = _head_inputs(onehot=True)
    onp, hits, _ = _head_run(tp, True)
    offp, _, _ = _head_run(tp, False)
    assert hits == 1
    refp, boundp, _ = _x_grad_bound(tp, u)
    errp = (onp["x"].double().cpu() - refp).abs()
    print("one class per pixel: worst |dx - ref| / bound = %.4f" % float((errp / boundp).max()))
    assert bool((errp <= boundp).all())
    for k in ("x", "w3", "wf", "bf", "x1"):
        assert torch.equal(onp[k], offp[k]), k


def test_fallbacks_equal_the_switch_off_path():
    from mrfp_amd import ops
    # a second consumer of the alias, through an operator of mrfp_amd.ops: the gradient is materialised
    t = _head_inputs()
    other = _cl(torch.ones(2, 128, 20, 22, dtype=torch.bfloat16, device=DEV))
    second = lambda alias: ops.add(alias, other)      # noqa: E731
    on, hits, _ = _head_run(t, True, second)
    off, _, _ = _head_run(t, False, second)
    assert hits == 0
    for k in on:
        assert torch.equal(on[k], off[k]), k
    # an fp32 run
    t32 = _head_inputs(torch.float32)
    on, hits, _ = _head_run(t32, True)
    off, _, _ = _head_run(t32, False)
    assert hits == 0
    for k in on:
        assert torch.equal(on[k], off[k]), k
    # a convolution whose input needs no gradient
    tn = _head_inputs(x_grad=False)
    on, hits, _ = _head_run(tn, True)
    off, _, _ = _head_run(tn, False)
    assert hits == 0 and on["x"] is None and off["x"] is None
    for k in ("x1", "w3", "wf", "bf"):
        assert torch.equal(on[k], off[k]), k


def test_a_consumer_that_bypasses_the_use_count_raises():
    from mrfp_amd import _lib
    t = _head_inputs()
    with pytest.raises(_lib.MrfpHipError):
        _head_run(t, True, lambda alias: alias * 2.0)        # a raw torch operator on the alias: autograd sums into an untagged tensor
    # (and the switch-off path takes the same graph)
    off, hits, _ = _head_run(t, False, lambda alias: alias * 2.0)
    assert hits == 0 and off["x"] is not None
