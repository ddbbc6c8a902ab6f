"""Boundary label relaxation and the joint-weighted soft-NLL loss on the GPU (csrc/relax.hip: mrfp_relax_labels, mrfp_multihot_pack,
mrfp_relax_word_counts, mrfp_relax_class_weights, mrfp_soft_nll_*, mrfp_upsample_soft_nll_*) against the restatements of
relaxed_common (numpy translation-and-OR, float64 counts / weights, the float64 torch loss in the published shape) and against what
the reference's own transform wrote (tests/golden/relaxed.npz).

Words, counts and class weights are compared for equality.  The loss bounds are those of test_loss_gpu.py (the same arithmetic
family): loss relative 1e-5 (fp32) / 2e-3 (16-bit), gradient 2e-5 / 1.5e-2 of the tensor maximum.  Inputs are rounded to the
activation dtype first; the gradient scale is 0.7, and 4096 for float16."""
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

import relaxed_common as rc
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
GC = rc.GOLDEN_C


def dname(d):
    return str(d).replace("torch.", "")


def ops():
    from mrfp_amd import ops as o
    return o


def relerr(a, b):
    """max |a - b| over max |b|.  Where the true gradient is 0 (every set holds every class) the float64 reference comes out as
    rounding noise of ~1e-17; the floor of 1e-9 -- seven orders below the gradients of these tests, s / (valid + 1) >= 1e-2 -- keeps
    that noise from becoming the yardstick."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-9)).item()


def bwd_scale(dtype):
    return 4096.0 if dtype == F16 else 0.7


def pad32(x, dtype):
    B, C, Hi, Wi = x.shape
    P = torch.zeros(B, 32, Hi, Wi)
    P[:, :C] = x
    return P.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)


def check(ld, gd, lref, gref, dtype, what):
    """A reference loss of exactly 0 (every set holds every class: C = 2 relaxed over a 4 x 4 map) has no relative error: the bound is
    then on the loss itself, against 1."""
    le = abs(ld.item() - lref.item()) / (abs(lref.item()) or 1.0)
    ge = relerr(gd, gref)
    print("%s: loss %.6g ref %.6g relerr %.3g gradient relerr %.3g" % (what, ld.item(), lref.item(), le, ge))
    assert math.isfinite(ld.item()) and le < LOSS_TOL[dtype] and ge < GRAD_TOL[dtype], (what, le, ge)


def weights_of(kind, B, C, seed):
    return None if kind == "none" else rc.make_weights(C, seed, rows=B if kind == "per_image" else None)


def dev(w):
    return None if w is None else w.to(DEV)


# ---- relaxation -------------------------------------------------------------------------------------------------------------------
def strict_sets(C):
    return (None, [0, C - 1], list(range(C)))


@pytest.mark.parametrize("C", [2, 19, 31])
@pytest.mark.parametrize("border", [0, 1, 2, 8])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 3), (3, 5, 7), (2, 33, 47), (1, 64, 256), (2, 67, 130)], ids=str)
def test_relax_labels_equals_numpy(shape, border, C):
    """Every word and every count, for no strict class, two, and all of them.  The maps hold -1, C and 255, full rows / columns of 255
    on the tile seams (row 32, column 64), and with B > 1 an all-ignored image; at border 8 the window is larger than the first three
    images."""
    B, H, W = shape
    y = rc.make_label_maps(B, H, W, C, 1000 + H * W + C, all_ignored_image=1 if B > 1 else None)
    yd = y.to(DEV)
    for strict in strict_sets(C):
        words, counts = ops().relax_labels(yd, C, border, strict, want_counts=True)
        assert words.dtype == torch.int32 and tuple(words.shape) == shape and counts.dtype == torch.int64 and tuple(counts.shape) == (B, C + 1)
        want = rc.np_relax(y.numpy(), C, border, strict)
        np.testing.assert_array_equal(words.cpu().numpy(), want, err_msg=str((shape, border, C, strict)))
        np.testing.assert_array_equal(counts.cpu().numpy(), rc.np_counts(want, C))
        assert torch.equal(ops().relax_labels(yd, C, border, strict), words)           # without the counts: the same words
        assert torch.equal(ops().relaxed_counts(words, C), counts)
    if B > 1:
        assert (want[1].view(np.uint32) == 1 << C).all()


def test_relax_labels_walks_several_tiles():
    """A workgroup of mrfp_relax_labels takes one 32 x 64 tile at a time and the grid holds at most 2048 // B workgroups per image.
    The smallest case with more tiles than workgroups: B = 1025 is the first batch size whose cap is 1 (2048 // 1025), and a
    33 x 2 image is the smallest with two tiles (rows 0..31 and row 32) -- every workgroup walks both, 67 650 labels in all."""
    from mrfp_amd import _lib
    B, H, W, C = 1025, 33, 2, 19
    assert int(_lib.lib().mrfp_relax_nblocks(B, H, W)) == B and int(_lib.lib().mrfp_relax_nblocks(1024, H, W)) == 2 * 1024
    y = rc.make_label_maps(B, H, W, C, 77, all_ignored_image=3)
    for border in (1, 8):
        words, counts = ops().relax_labels(y.to(DEV), C, border, [5], want_counts=True)
        want = rc.np_relax(y.numpy(), C, border, [5])
        np.testing.assert_array_equal(words.cpu().numpy(), want)
        np.testing.assert_array_equal(counts.cpu().numpy(), rc.np_counts(want, C))


def test_golden_relaxation():
    """The reference's own transform: its label maps through relax_labels give its words; its raw multi-hot bytes pack to its words;
    to_multihot(relax_labels(x)) gives its bytes."""
    from mrfp_amd import input_pipeline
    from mrfp_amd.config import cfg
    g = rc.golden()
    for name in rc.GOLDEN_MAPS + ("tiny",):
        lab = torch.from_numpy(g[name + "_lab"].astype(np.int64)).to(DEV)
        for border in rc.GOLDEN_BORDERS:
            for sname, strict in rc.GOLDEN_STRICT.items():
                got = ops().relax_labels(lab[None], GC, border, strict)[0]
                np.testing.assert_array_equal(got.cpu().numpy(), g[rc.golden_key(name, border, sname)], err_msg=str((name, border, sname)))
    mh = torch.from_numpy(g["tiny_multihot"]).to(DEV)
    np.testing.assert_array_equal(ops().pack_multihot(mh[None])[0].cpu().numpy(), g[rc.golden_key("tiny", 1, "none")])
    tiny = torch.from_numpy(g["tiny_lab"].astype(np.int64)).to(DEV)
    t = input_pipeline.RelaxedBoundaryTarget(GC)                   # border / strict classes from cfg at call time: 1, None
    assert (cfg.BORDER_WINDOW, cfg.STRICTBORDERCLASS) == (1, None)
    out = t.to_multihot(t(tiny))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (GC + 1, 5, 7)
    np.testing.assert_array_equal(out.cpu().numpy(), g["tiny_multihot"])
    t2 = input_pipeline.RelaxedBoundaryTarget(GC, border=2, strict_classes=[5, 11])
    np.testing.assert_array_equal(t2(tiny[None]).cpu().numpy()[0], g[rc.golden_key("tiny", 2, "s5_11")])


@pytest.mark.parametrize("C", [2, 19, 31])
@pytest.mark.parametrize("shape", [(2, 8, 12), (3, 5, 7), (1, 1, 1), (2, 33, 130)], ids=str)
def test_pack_multihot_round_trip(shape, C):
    """pack_multihot(unpack(words)) == words and its counts are the words' counts, on random words over all C + 1 bits, with set bytes
    of 1, 255 and a mix (any non-zero byte is set); H * W a multiple of 4 (one 32-bit load per plane) and not."""
    B, H, W = shape
    rng = np.random.default_rng(C * 100 + H)
    words = rng.integers(0, 1 << (C + 1), shape, dtype=np.int64).astype(np.uint32).view(np.int32)
    words[0, 0, 0] = 0
    for set_value in (1, 255, None):
        mh = rc.unpack(words, C, 1 if set_value is None else set_value)
        if set_value is None:
            mh = (mh * rng.integers(1, 256, mh.shape)).astype(np.uint8)
        got, counts = ops().pack_multihot(torch.from_numpy(mh).to(DEV), want_counts=True)
        np.testing.assert_array_equal(got.cpu().numpy(), words)
        np.testing.assert_array_equal(counts.cpu().numpy(), rc.np_counts(words, C))


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("kind", ["mixed", "one_image_ignored", "all_ignored"])
def test_relaxed_class_weights_equal_numpy(kind, norm, batch):
    """ops.relaxed_class_weights == the float64 numpy rule rounded once, EQUAL not close (the bar of
    test_loss_gpu.test_label_class_weights_equal_numpy).  The ignore plane counts in the total; a class no word carries gets 1."""
    y = rc.make_label_maps(2, 33, 47, GC, 91, all_ignored_image=1 if kind == "one_image_ignored" else None)
    if kind == "all_ignored":
        y[:] = 255
    _, counts = ops().relax_labels(y.to(DEV), GC, 1, None, want_counts=True)
    n = rc.np_counts(rc.np_relax(y.numpy(), GC, 1), GC)
    np.testing.assert_array_equal(counts.cpu().numpy(), n)
    for ub in (1.0, 0.3):
        got = ops().relaxed_class_weights(counts, ub, norm, batch)
        want = rc.np_weights(n, ub, norm, batch)
        assert got.dtype == F32 and tuple(got.shape) == ((GC,) if batch else (2, GC))
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    if kind == "all_ignored":
        assert (want == 1.0).all()
    if kind == "one_image_ignored" and not batch:
        assert (want[1] == 1.0).all() and want[0, GC - 1] == 1.0 and (want[0, :GC - 1] != 1.0).any()


# ---- the loss ---------------------------------------------------------------------------------------------------------------------
DENSE = [(2, 19, 12, 10), (1, 19, 7, 9), (3, 5, 4, 6), (2, 8, 3, 3), (2, 31, 5, 7)]


def relaxed_of(y, C, border):
    """(words on the device from ops.relax_labels, the same as numpy for the restatement)."""
    words = ops().relax_labels(y.to(DEV), C, border)
    return words, words.cpu().numpy()


@pytest.mark.parametrize("wkind", ["none", "shared", "per_image"])
@pytest.mark.parametrize("border", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("shape", DENSE, ids=str)
def test_dense_soft_nll(shape, dtype, border, wkind):
    """ops.soft_nll against the float64 restatement in the published shape; targets from relax_labels of maps in 2 x 3 cells (k from 1
    to several; ignored pixels inside the 255 corner of the larger maps); shared weights have one class exactly 0, per-image rows each their own."""
    B, C, H, W = shape
    y = rc.make_label_maps(B, H, W, C, 100 + sum(shape), cell=(2, 3))
    x = rc.make_logits(B, C, H, W, dtype, 200 + sum(shape))
    w = weights_of(wkind, B, C, 300 + sum(shape))
    words, wnp = relaxed_of(y, C, border)
    s = bwd_scale(dtype)
    xc = x.double().requires_grad_(True)
    lref = rc.ref_loss(xc, wnp, C, None if w is None else w.double())
    (lref * s).backward()
    xd = x.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)
    ld = ops().soft_nll(xd, words, C, weight=dev(w))
    (ld * s).backward()
    assert ld.dtype == F32 and xd.grad.dtype == dtype
    check(ld, xd.grad, lref, xc.grad, dtype, "dense %s %s border %d %s" % (shape, dname(dtype), border, wkind))


FUSED = [((3, 4), (9, 13)), ((6, 5), (24, 17)), ((1, 1), (4, 4))]


@pytest.mark.parametrize("wkind", ["none", "shared", "per_image"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("C", [2, 19, 31])
@pytest.mark.parametrize("case", FUSED, ids=str)
def test_fused_upsample_soft_nll(case, C, dtype, wkind):
    """ops.upsample_soft_nll == Upsample() then the restatement on the CPU, for border 1 and 2; scores at pitch 32, the gradient of the
    pad channels exactly 0."""
    low, out = case
    B = 2
    x = rc.make_logits(B, C, low[0], low[1], dtype, 400 + C + sum(out), 2.0)
    y = rc.make_label_maps(B, out[0], out[1], C, 500 + C + sum(out), cell=(2, 3))
    w = weights_of(wkind, B, C, 600 + C)
    s = bwd_scale(dtype)
    for border in (1, 2):
        words, wnp = relaxed_of(y, C, border)
        xc = x.double().requires_grad_(True)
        lref = rc.ref_loss(orc.upsample_bilinear_ac(xc, out), wnp, C, None if w is None else w.double())
        (lref * s).backward()
        Pd = pad32(x, dtype)
        ld = ops().upsample_soft_nll(Pd, words, out, C, weight=dev(w))
        (ld * s).backward()
        check(ld, Pd.grad[:, :C], lref, xc.grad, dtype, "fused %s C=%d %s border %d %s" % (case, C, dname(dtype), border, wkind))
        assert float(Pd.grad[:, C:].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
def test_confident_wrong_pixels(dtype):
    """Logits -80 on every class of the set and +80 on the others: softmax over the set underflows in float32 (exp(-160)), the two
    log-sum-exps do not.  Loss and gradient are finite and within the same bounds; the float64 restatement is finite there."""
    B, C, H, W = 2, 19, 9, 11
    y = rc.make_label_maps(B, H, W, C, 31, cell=(2, 3))
    words, wnp = relaxed_of(y, C, 1)
    in_set = torch.from_numpy(rc.unpack(wnp, C)[:, :C].astype(bool))
    x = torch.where(in_set, torch.tensor(-80.0), torch.tensor(80.0)).to(dtype).float()
    w = rc.make_weights(C, 33, rows=B)
    xc = x.double().requires_grad_(True)
    lref = rc.ref_loss(xc, wnp, C, w.double())
    (lref * 0.7).backward()
    assert math.isfinite(lref.item()) and torch.isfinite(xc.grad).all() and lref.item() > 100.0
    xd = x.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)
    ld = ops().soft_nll(xd, words, C, weight=w.to(DEV))
    (ld * 0.7).backward()
    assert torch.isfinite(xd.grad).all()
    check(ld, xd.grad, lref, xc.grad, dtype, "confident wrong %s" % dname(dtype))


@pytest.mark.parametrize("kind", ["dense", "fused"])
def test_all_ignored_image_inside_a_batch(kind):
    """Image 1 is all 255: its gradient rows are exactly zero, the batch loss is finite (it adds 0 / (0 + 1)), and image 0's loss and
    gradient are what they are when it runs alone."""
    C, out = 19, (24, 17)
    low = out if kind == "dense" else (6, 5)
    y = rc.make_label_maps(2, out[0], out[1], C, 41, all_ignored_image=1)
    x = rc.make_logits(2, C, low[0], low[1], F32, 42)
    w = rc.make_weights(C, 43).to(DEV)

    def run(xs, ys):
        words = ops().relax_labels(ys.to(DEV), C, 2)
        if kind == "dense":
            xd = xs.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
            ld = ops().soft_nll(xd, words, C, weight=w)
        else:
            xd = pad32(xs, F32)
            ld = ops().upsample_soft_nll(xd, words, out, C, weight=w)
        (ld * 0.7).backward()
        return ld.detach(), xd.grad
    lb, gb = run(x, y)
    la, ga = run(x[:1], y[:1])
    assert math.isfinite(lb.item()) and float(gb[1].abs().max()) == 0.0 and float(gb[0].abs().max()) > 0.0
    assert torch.equal(gb[0], ga[0]) and abs(lb.item() - la.item()) <= LOSS_TOL[F32] * abs(la.item())


# ---- above the workgroup cap: 3 x 419 x 419 = 526 683 pixels > 2048 * 256, 682 workgroups per image ----------------------------------
BIG_B, BIG_C, BIG_LOW, BIG_S = 3, 19, 105, 419


@functools.lru_cache(maxsize=None)
def big_case(kind, dtype):
    """Inputs and the float64 reference (loss, gradient), computed once per (kind, dtype) and not modified."""
    side = BIG_S if kind == "dense" else BIG_LOW
    x = rc.make_logits(BIG_B, BIG_C, side, side, dtype, 700 + side, 2.0)
    y = rc.make_label_maps(BIG_B, BIG_S, BIG_S, BIG_C, 701)
    w = rc.make_weights(BIG_C, 702, rows=BIG_B)
    wnp = rc.np_relax(y.numpy(), BIG_C, 1)
    xc = x.double().requires_grad_(True)
    full = xc if kind == "dense" else orc.upsample_bilinear_ac(xc, (BIG_S, BIG_S))
    lref = rc.ref_loss(full, wnp, BIG_C, w.double())
    (lref * 0.7).backward()
    return x, y, w, wnp, lref.detach(), xc.grad


def run_big(kind, dtype):
    x, y, w, wnp, _, _ = big_case(kind, dtype)
    words = ops().relax_labels(y.to(DEV), BIG_C, 1)
    if kind == "dense":
        xd = x.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)
        ld = ops().soft_nll(xd, words, BIG_C, weight=w.to(DEV))
    else:
        xd = pad32(x, dtype)
        ld = ops().upsample_soft_nll(xd, words, (BIG_S, BIG_S), BIG_C, weight=w.to(DEV))
    (ld * 0.7).backward()
    return words, ld.detach(), xd.grad


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
@pytest.mark.parametrize("kind", ["dense", "fused"])
def test_above_the_workgroup_cap_with_per_image_weights(kind, dtype):
    """B = 3 at 419 x 419: the loss grid is (682, 3), every workgroup walks a second pixel in part of its threads, the finalize kernel
    reduces 682 partials per image; relax_labels runs 14 x 7 tiles per image; per-image weights [3,19]."""
    from mrfp_amd import _lib
    x, y, w, wnp, lref, gref = big_case(kind, dtype)
    assert int(_lib.lib().mrfp_soft_nll_nblocks(BIG_B, BIG_S * BIG_S)) == 3 * 682
    words, ld, grad = run_big(kind, dtype)
    np.testing.assert_array_equal(words.cpu().numpy(), wnp)
    if kind == "fused":
        assert float(grad[:, BIG_C:].abs().max()) == 0.0
    check(ld, grad[:, :BIG_C], lref, gref, dtype, "big %s %s" % (kind, dname(dtype)))


def test_two_runs_are_bit_identical():
    """Per-workgroup partials + a finalize kernel in a fixed order, no floating-point atomics: the fused form in bf16 twice gives the
    same bits, loss and gradient, at the many-workgroup shape and at a small one."""
    got = [run_big("fused", BF16) for _ in range(2)]
    assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][2], got[1][2]) and math.isfinite(got[0][1].item())
    x = rc.make_logits(2, 19, 6, 5, BF16, 55, 2.0)
    words = ops().relax_labels(rc.make_label_maps(2, 24, 17, 19, 56).to(DEV), 19, 2)
    w = rc.make_weights(19, 57, rows=2).to(DEV)
    small = []
    for _ in range(2):
        Pd = pad32(x, BF16)
        ld = ops().upsample_soft_nll(Pd, words, (24, 17), 19, weight=w)
        ld.backward()
        small.append((ld.detach(), Pd.grad))
    assert torch.equal(small[0][0], small[1][0]) and torch.equal(small[0][1], small[1][1])


def test_operator_refusals():
    from mrfp_amd import _lib
    o = ops()
    x = rc.make_logits(2, 19, 6, 5, F32, 81).to(DEV).contiguous(memory_format=CL)
    words = o.relax_labels(rc.make_label_maps(2, 6, 5, 19, 82).to(DEV), 19)
    bad = [dict(relaxed=words.long()), dict(relaxed=words[:1]), dict(relaxed=words.cpu()), dict(weight=torch.ones(19)),
           dict(weight=torch.ones(18, device=DEV)), dict(weight=torch.ones(3, 19, device=DEV)), dict(weight=torch.ones(19, device=DEV).double())]
    for kw in bad:
        rel = kw.pop("relaxed", words)
        with pytest.raises(_lib.MrfpHipError):
            o.soft_nll(x, rel, 19, **kw)
        with pytest.raises(_lib.MrfpHipError):
            o.upsample_soft_nll(x, rel, (6, 5), 19, **kw)
    with pytest.raises(_lib.MrfpHipError):
        o.soft_nll(x, words, 18)


def test_refusals_through_the_c_abi_launch_nothing():
    """C = 32, border = 9, a wstride that is neither 0 nor C, a null pointer, on device buffers: each returns the error and the
    output buffers keep their fill."""
    from mrfp_amd import _lib
    from mrfp_amd._lib import ptr
    L = _lib.lib()
    y = rc.make_label_maps(2, 4, 4, 19, 5).to(DEV)
    words = torch.full((2, 4, 4), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((2, 33), -7, dtype=torch.int64, device=DEV)
    x = torch.zeros(2, 4, 4, 32, device=DEV)
    f = torch.full((64,), -7.0, device=DEV)
    d = torch.full((2, 4, 4, 32), -7.0, device=DEV)
    calls = [
        ("mrfp_relax_labels", (ptr(y), 2, 4, 4, 32, 1, 0, ptr(words), ptr(counts), None), b"1 <= C <= 31"),
        ("mrfp_relax_labels", (ptr(y), 2, 4, 4, 19, 9, 0, ptr(words), ptr(counts), None), b"border"),
        ("mrfp_relax_labels", (None, 2, 4, 4, 19, 1, 0, ptr(words), ptr(counts), None), b"null pointer"),
        ("mrfp_multihot_pack", (ptr(x), 2, 16, 32, ptr(words), ptr(counts), None), b"1 <= C <= 31"),
        ("mrfp_soft_nll_fwd", (ptr(x), ptr(words), 0, 2, 16, 19, ptr(f), 7, ptr(f), ptr(f), None), b"wstride"),
        ("mrfp_soft_nll_bwd", (ptr(x), ptr(words), ptr(f), None, ptr(d), 0, 2, 16, 32, None, 0, None), b"1 <= C <= 31"),
        ("mrfp_upsample_soft_nll_fwd", (ptr(x), 32, ptr(words), 0, 2, 4, 4, 4, 4, 19, ptr(f), 5, ptr(f), ptr(f), None), b"wstride"),
        ("mrfp_upsample_soft_nll_bwd", (ptr(x), 32, ptr(words), ptr(f), None, None, 20, 0, 2, 4, 4, 4, 4, 19, None, 0, None), b"null pointer"),
    ]
    for name, args, text in calls:
        assert getattr(L, name)(*args) == -1 and text in L.mrfp_last_error(), (name, L.mrfp_last_error())
    torch.cuda.synchronize()
    assert (words == -7).all() and (counts == -7).all() and (f == -7.0).all() and (d == -7.0).all()


# ---- the criterion ----------------------------------------------------------------------------------------------------------------
def test_criterion_takes_the_three_target_forms_and_stays_on_the_device(monkeypatch):
    """ImgWtLossSoftNLL(19, border=2, strict_classes=[5, 11]) on (2,19,24,20) logits: the int64 label map, the words and the uint8
    multi-hot give the same loss within LOSS_TOL[F32], and it is the float64 restatement with numpy's weights; during forward and
    backward torch.cuda.synchronize, Tensor.cpu and Tensor.item raise."""
    from mrfp_amd.loss import ImgWtLossSoftNLL
    B, C, H, W = 2, 19, 24, 20
    y = rc.make_label_maps(B, H, W, C, 95)
    x = rc.make_logits(B, C, H, W, F32, 96)
    wnp = rc.np_relax(y.numpy(), C, 2, [5, 11])
    forms = {"labels": y.to(DEV), "words": torch.from_numpy(wnp).to(DEV), "multihot": torch.from_numpy(rc.unpack(wnp, C)).to(DEV)}
    for batch_weights in (False, True):
        crit = ImgWtLossSoftNLL(C, upper_bound=0.8, batch_weights=batch_weights, border=2, strict_classes=[5, 11]).to(DEV)
        w = torch.from_numpy(rc.np_weights(rc.np_counts(wnp, C), 0.8, False, batch_weights)).double()
        xc = x.double().requires_grad_(True)
        lref = rc.ref_loss(xc, wnp, C, w)
        lref.backward()
        losses = {}
        for form, target in forms.items():
            xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)

            def boom(*a, **k):
                raise AssertionError("host synchronisation inside the criterion")
            with monkeypatch.context() as mp:
                mp.setattr(torch.cuda, "synchronize", boom)
                mp.setattr(torch.Tensor, "cpu", boom)
                mp.setattr(torch.Tensor, "item", boom)
                ld = crit(xd, target)
                ld.backward()
            check(ld, xd.grad, lref, xc.grad, F32, "ImgWtLossSoftNLL %s batch_weights=%s" % (form, batch_weights))
            losses[form] = ld.item()
        for form in ("words", "multihot"):
            assert abs(losses[form] - losses["labels"]) <= LOSS_TOL[F32] * abs(losses["labels"]), losses


# ---- the criterion on a model -----------------------------------------------------------------------------------------------------
class Restated(nn.Module):
    """A module the criterion helper does not recognise: the model takes the stock path and hands it the full-resolution fp32
    logits; it evaluates the float64 restatement on them with stock torch."""

    def __init__(self, C, border):
        super().__init__()
        self.C, self.border = C, border

    def forward(self, logits, y):
        wnp = rc.np_relax(y.cpu().numpy(), self.C, self.border)
        w = torch.from_numpy(rc.np_weights(rc.np_counts(wnp, self.C), 1.0, False, False)).double()
        return rc.ref_loss(logits.double(), wnp, self.C, w).float()


@pytest.fixture(scope="module")
def model():
    from mrfp_amd import deepv3
    from mrfp_amd.config import cfg
    try:
        cfg.MODEL.ACT_DTYPE = BF16
        spec = json.load(open(os.path.join(HERE, "golden", "state_dict_spec.json")))
        with contextlib.redirect_stdout(io.StringIO()):
            m = deepv3.MRFPPlus(19, criterion=nn.CrossEntropyLoss(ignore_index=255))
        m.load_state_dict(synth.synth_state_dict([(k, tuple(s)) for k, s in spec["MRFPPlus"]], seed=0))
        m = m.to(DEV).train()
        m.rng = deepv3.InjectedRandom((True, True, True), synth.synth_noise(2, seed=2))
        x, y = synth.synth_batch(2, 128, 128, seed=3)
        yield m, x.to(DEV), y.to(DEV)
    finally:
        cfg.MODEL.ACT_DTYPE = torch.float32


def _train_step(m, x, y, crit):
    """One forward + backward with `crit` as the criterion -> (loss, d final2.weight, entry points launched, upsample sizes asked)."""
    from mrfp_amd import _lib, ops as o
    m.criterion = crit.to(DEV)
    m.zero_grad(set_to_none=True)
    names, sizes = [], []
    orig = o.upsample_bilinear

    def spy(t, size, *a, **k):
        sizes.append(tuple(size))
        return orig(t, size, *a, **k)
    hook = _lib.HOOK[0]
    _lib.HOOK[0] = lambda n, args: names.append(n)
    o.upsample_bilinear = spy
    try:
        loss = m(x, y, training=True)
        loss.backward()
    finally:
        _lib.HOOK[0] = hook
        o.upsample_bilinear = orig
    return loss.detach().float().clone(), m.final2[0].weight.grad.detach().float().clone(), names, sizes


def test_model_criterion_runs_on_the_fused_kernels(model, monkeypatch):
    """MRFPPlus (bf16 activations, 2 x 128 x 128) with criterion=ImgWtLossSoftNLL(19, border=1): with the criterion's own forward
    patched to raise the step still runs -- mrfp_relax_labels, mrfp_upsample_soft_nll_fwd / _bwd were launched, the dense form was
    not, and nothing upsampled the class scores to the input size (the loss path allocates no full-resolution logits).  Loss and
    d final2.weight agree with the stock-torch float64 restatement on the model's own full-resolution logits within the 16-bit
    bounds."""
    from mrfp_amd.loss import ImgWtLossSoftNLL
    m, x, y = model
    crit = ImgWtLossSoftNLL(19, border=1)

    def boom(self, *a, **k):
        raise AssertionError("the model called the criterion's forward: it left the fused loss kernels")
    with monkeypatch.context() as mp:
        mp.setattr(ImgWtLossSoftNLL, "forward", boom)
        loss, grad, names, sizes = _train_step(m, x, y, crit)
    assert math.isfinite(loss.item()) and torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    for n in ("mrfp_relax_labels", "mrfp_relax_class_weights", "mrfp_upsample_soft_nll_fwd", "mrfp_upsample_soft_nll_bwd"):
        assert n in names, n
    assert "mrfp_soft_nll_fwd" not in names and not [n for n in names if "_ce_" in n] and (128, 128) not in sizes
    sloss, sgrad, snames, ssizes = _train_step(m, x, y, Restated(19, 1))
    assert (128, 128) in ssizes and not [n for n in snames if "soft_nll" in n]
    le, ge = abs(loss.item() - sloss.item()) / abs(sloss.item()), relerr(grad, sgrad)
    print("fused %.6f restated %.6f relerr %.3g, d final2.weight relerr %.3g" % (loss.item(), sloss.item(), le, ge))
    assert le < LOSS_TOL[BF16] and ge < GRAD_TOL[BF16], (le, ge)


def test_plain_criterion_still_takes_the_plain_launches(model):
    m, x, y = model
    loss, _, names, sizes = _train_step(m, x, y, nn.CrossEntropyLoss(ignore_index=255))
    assert math.isfinite(loss.item()) and "mrfp_upsample_ce_fwd" in names and "mrfp_upsample_ce_bwd" in names
    assert not [n for n in names if "soft_nll" in n or "relax" in n or "_ce_w_" in n] and (128, 128) not in sizes


def test_trainer_step_with_the_criterion(model):
    """harness.Trainer takes a step on a model constructed around the criterion: finite loss, the fused launches, parameters move."""
    from mrfp_amd import _lib, harness
    from mrfp_amd.loss import ImgWtLossSoftNLL
    m, x, y = model
    m.criterion = ImgWtLossSoftNLL(19, border=1).to(DEV)
    m.zero_grad(set_to_none=True)
    tr = harness.Trainer(m, lr=1e-3, max_iter=10)
    before = m.final2[0].weight.detach().clone()
    names = []
    hook = _lib.HOOK[0]
    _lib.HOOK[0] = lambda n, args: names.append(n)
    try:
        loss = tr.step(x, y)
    finally:
        _lib.HOOK[0] = hook
    assert math.isfinite(loss.item()) and "mrfp_upsample_soft_nll_fwd" in names and "mrfp_upsample_soft_nll_bwd" in names
    assert not torch.equal(m.final2[0].weight.detach(), before)
