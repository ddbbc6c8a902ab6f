"""The online-hard-example-mining cross entropy on the GPU (csrc/ohem.hip: mrfp_select_kth, mrfp_ohem_target,
mrfp_upsample_ohem_target; ops.select_kth / ohem_target / ohem_cross_entropy / upsample_ohem_cross_entropy; loss.OhemCrossEntropy2d).

What must be exact and what is approximate are tested apart.
  * The select: bit for bit against torch.sort on the host.
  * The selection: the rule (ohem_common.rule) applied on the host to the DEVICE's own probability plane must give the device's
    masked target, N, kept count, theta bits and mode exactly, in every regime.
  * The probability plane: against exp(z_t - lse) in fp64 on the kernel's own logits (dense: the stored values; fused:
    predict_common.restated_z), in fp32 ulps of the expected value.  The kernel uses expf and an fp64 denominator and quotient, so the
    error does not grow with |ln p|: what is left is expf's own error on the numerator, the relative error of the denominator (a
    sum of such terms) and the final rounding.  Measured maximum over the cases below: 1.611 ulp (profiles/ohem.md); the bound is
    twice that, rounded up.
  * Loss and gradient: bit-identical to the cross-entropy operators on the masked target (they ARE those operators).
  * End to end against an fp64 rule that never sees the device plane, on inputs whose thresholds sit in gaps >= 1e-3 relative.
"""
import contextlib
import functools
import io
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import ohem_common as oc
import predict_common as pc
from mrfp_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
PROB_ULP = 4.0

# (name, kind, B, C, (Hi, Wi) or None, (H, W), ld)
DENSE = ("dense", "dense", 2, 19, None, (33, 47), None)
FUSED = ("fused", "fused", 2, 19, (9, 12), (33, 47), 32)
CAPPED = ("capped", "fused", 3, 19, (105, 105), (419, 419), 32)        # 682 workgroups per image, 175 561 pixels: a workgroup walks two trips
C1 = ("c1", "dense", 2, 1, None, (9, 11), None)
C64 = ("c64", "fused", 2, 64, (4, 5), (9, 11), 64)
CASES = {c[0]: c for c in (DENSE, FUSED, CAPPED, C1, C64)}


def ops():
    from mrfp_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """-> (host scores in the kernel's layout: dense [B,H,W,C], fused [B,Hi,Wi,ld] with huge pad channels; labels int64 [B,H,W];
    the kernel's own class vectors as float32 numpy [B,H,W,C]).  Computed once per process, never modified."""
    _, kind, B, C, low, (H, W), ld = CASES[name]
    seed = sum(map(ord, name)) + 7 * pc.DTYPES.index(dtype)
    y = oc.labels(B, H, W, C, 1000 + seed)
    g = torch.Generator().manual_seed(seed)
    if kind == "dense":
        z = (4.0 * torch.randn(B, H, W, C, generator=g)).to(dtype)
        return z, y, z.float().numpy()
    z = (4.0 * torch.randn(B, low[0], low[1], ld, generator=g)).to(dtype)
    z[..., C:] = 65504.0 if dtype == F16 else 1e30
    return z, y, pc.restated_z(z, C, H, W)


def on_device(z):
    return z.to(DEV).permute(0, 3, 1, 2)          # logical [B,C,H,W] over the same NHWC storage


def run_target(name, dtype, thresh, min_kept, y=None, z=None):
    _, kind, B, C, low, size, ld = CASES[name]
    z0, y0, _ = inputs(name, dtype)
    z, y = z0 if z is None else z, y0 if y is None else y
    kw = dict(size=size, channels=C) if kind == "fused" else {}
    masked, prob, state = ops().ohem_target(on_device(z), y.to(DEV), oc.IGNORE, thresh, min_kept, want_prob=True, want_state=True, **kw)
    assert masked.dtype == torch.int64 and prob.dtype == F32 and state.dtype == torch.int32 and tuple(state.shape) == (4,)
    assert tuple(masked.shape) == tuple(prob.shape) == tuple(y.shape)
    return masked.cpu().numpy(), prob.cpu().numpy(), state.cpu().numpy().view(np.uint32).tolist()


def check_selection(name, dtype, thresh, min_kept, want_mode, y=None, z=None):
    """the device's masked target and state == the rule applied on the host to the device's own plane"""
    _, _, B, C, _, _, _ = CASES[name]
    yy = (inputs(name, dtype)[1] if y is None else y).numpy()
    masked, prob, state = run_target(name, dtype, thresh, min_kept, y, z)
    want, N, kept, theta, mode = oc.rule(prob, yy, C, thresh, min_kept)
    assert mode == want_mode, (mode, want_mode)                     # the case is in the regime it was built for
    assert state == [N, kept, oc.theta_bits(theta), mode], (state, N, kept, theta, mode)
    assert np.array_equal(masked, want)
    assert np.array_equal(prob.view(np.uint32) == 0x40000000, ~oc.valid_mask(yy, C))
    return masked, prob, N, kept


# ---- the select -------------------------------------------------------------------------------------------------------------------
def _planes(kind, n, g):
    if kind == "uniform":
        return torch.rand(n, generator=g)
    if kind == "equal":
        return torch.full((n,), 0.3125)
    if kind == "duplicates":                        # 90 % of the elements are one of three values
        x = torch.rand(n, generator=g)
        pick = torch.rand(n, generator=g)
        vals = torch.tensor([0.125, 0.7, 0.70000005])
        return torch.where(pick < 0.9, vals[torch.randint(0, 3, (n,), generator=g)], x)
    if kind == "low_bit":                           # two neighbouring floats: only the last radix pass tells them apart
        bits = torch.full((n,), 0x3f333333, dtype=torch.int32) + torch.randint(0, 2, (n,), generator=g, dtype=torch.int32)
        return bits.view(torch.float32)
    if kind == "sentinels":
        x = torch.rand(n, generator=g)
        x[torch.rand(n, generator=g) < 0.3] = 2.0
        x[0] = 0.5                                  # at least one element counts
        return x
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["uniform", "equal", "duplicates", "low_bit", "sentinels"])
def test_select_kth_equals_sort_bit_for_bit(kind):
    g = torch.Generator().manual_seed(len(kind))
    for n in (1, 255, 256, 257, 70001):
        x = _planes(kind, n, g)
        live = torch.sort(x[x != 2.0]).values
        xd = x.to(DEV)
        for k in sorted({1, max(1, len(live) // 2), len(live)}):
            got = ops().select_kth(xd, k)
            assert got.dtype == F32 and got.dim() == 0 and got.is_cuda
            assert got.cpu().view(torch.int32).item() == live[k - 1].view(torch.int32).item(), (kind, n, k)
    if kind == "sentinels":                         # a rank above the live elements: NaN
        assert math.isnan(ops().select_kth(xd, len(live) + 1).item())
    if kind == "uniform":                           # NaN sorts last, as torch.sort
        x[::7] = float("nan")
        want = torch.sort(x).values
        for k in (1, n - n // 7 - 1, n):
            got = ops().select_kth(x.to(DEV), k).cpu()
            assert (math.isnan(got.item()) and math.isnan(want[k - 1].item())) or got.view(torch.int32).item() == want[k - 1].view(torch.int32).item()
        assert math.isnan(ops().select_kth(x.to(DEV), n).item())
        with pytest.raises(Exception, match="select_kth"):
            ops().select_kth(xd, 0)
        with pytest.raises(Exception, match="select_kth"):
            ops().select_kth(xd.double(), 1)


# ---- the selection, on the device's own plane -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=pc.dname)
@pytest.mark.parametrize("name", ["dense", "fused"])
def test_selection_is_exact_in_every_regime(name, dtype):
    """4 * randn scores over 19 classes: most p are small (the median is near 3e-4), so count(p <= 0.7) is nearly N and the k-th regime
    needs a thresh far below; the labels hold -1, C and 200 beside 255."""
    _, _, B, C, _, (H, W), _ = CASES[name]
    y = inputs(name, dtype)[1]
    N = int(oc.valid_mask(y.numpy(), C).sum())
    assert all(int((y == v).sum()) > 0 for v in (255, -1, C, 200)) and 1000 < N < B * H * W
    check_selection(name, dtype, 0.7, N + 1, oc.KEEP_ALL)                     # min_kept > N
    _, _, _, kept = check_selection(name, dtype, 0.7, 300, oc.THRESH)         # count(p <= thresh) >= min_kept
    assert 300 <= kept < N
    _, _, _, kept = check_selection(name, dtype, 1e-6, N // 2, oc.KTH)        # q > thresh
    assert kept >= N // 2
    check_selection(name, dtype, 0.001, N, oc.KTH)                            # the largest p
    check_selection(name, dtype, 0.001, 1, oc.THRESH)
    _, _, _, kept = check_selection(name, dtype, 0.3, 0, oc.THRESH)           # min_kept = 0
    assert 0 < kept < N
    check_selection(name, dtype, 0.0, 0, oc.THRESH)
    check_selection(name, dtype, 1.0, N, oc.THRESH)
    dead = torch.tensor([255, -1, C, 200])[torch.arange(B * H * W) % 4].reshape(B, H, W)
    masked, _, n, kept = check_selection(name, dtype, 0.7, 10, oc.KEEP_ALL, y=dead)      # all labels ignored
    assert n == 0 and kept == 0 and (masked == oc.IGNORE).all()


@pytest.mark.parametrize("name,dtype", [("capped", BF16), ("c1", F32), ("c64", BF16), ("c64", F32)], ids=str)
def test_selection_capped_grid_one_class_and_sixty_four(name, dtype):
    _, _, B, C, _, _, _ = CASES[name]
    N = int(oc.valid_mask(inputs(name, dtype)[1].numpy(), C).sum())
    if C == 1:                                       # p == 1 everywhere: the k-th smallest is 1 > thresh, every pixel ties at it
        _, prob, _, kept = check_selection(name, dtype, 0.5, 5, oc.KTH)
        assert kept == N and (prob[prob != 2.0] == 1.0).all()
        check_selection(name, dtype, 1.0, N // 3, oc.THRESH)
    else:
        check_selection(name, dtype, 0.7, N // 3, oc.THRESH)
        check_selection(name, dtype, 1e-6, N - N // 7, oc.KTH)
    check_selection(name, dtype, 0.7, N + 1, oc.KEEP_ALL)


def test_selection_keeps_every_tie_at_q():
    """Five pixels with the same class vector and label tie at one p; min_kept is put on the second of them in the device's own
    order, so q is the tied value and the kept count exceeds min_kept by three."""
    name, dtype = "dense", F32
    z0, y0, _ = inputs(name, dtype)
    z, y = z0.clone(), y0.clone()
    C = 19
    spots = [(0, 3, 5), (0, 20, 40), (1, 0, 0), (1, 32, 46), (1, 17, 9)]
    for b, h, w in spots:
        z[b, h, w] = z[0, 10, 10]
        y[b, h, w] = 4
    _, prob, _ = run_target(name, dtype, 0.0, 0, y, z)
    tied = prob[tuple(zip(*spots))]
    assert (tied == tied[0]).all()
    live = np.sort(prob[oc.valid_mask(y.numpy(), C)])
    first = int(np.searchsorted(live, tied[0], side="left"))
    ties = int((live == tied[0]).sum())
    assert ties >= 5
    masked, _, N, kept = check_selection(name, dtype, 0.0, first + 2, oc.KTH, y, z)
    assert kept == first + ties > first + 2 and all(masked[s] == 4 for s in spots)


def test_nan_scores_are_never_kept():
    name, dtype = "dense", F32
    z0, y0, _ = inputs(name, dtype)
    z, y = z0.clone(), y0.clone()
    z[0, 5, 5, 3] = float("nan")
    z[1, 7, 7] = float("nan")
    y[0, 5, 5], y[1, 7, 7] = 3, 2
    N = int(oc.valid_mask(y.numpy(), 19).sum())
    for thresh, k, mode in ((0.7, 10, oc.THRESH), (0.0001, N - 5, oc.KTH), (0.2, N, oc.THRESH), (0.7, N + 1, oc.KEEP_ALL)):
        masked, prob, _, _ = check_selection(name, dtype, thresh, k, mode, y, z)
        assert prob.view(np.uint32)[0, 5, 5] == 0x7fc00000 and prob.view(np.uint32)[1, 7, 7] == 0x7fc00000
        assert (masked[0, 5, 5] == 3) == (mode == oc.KEEP_ALL)


# ---- the probability plane --------------------------------------------------------------------------------------------------------
PROB_CASES = [(n, d) for n in ("dense", "fused") for d in pc.DTYPES] + [("capped", BF16), ("c1", F32), ("c64", BF16), ("c64", F32)]


@pytest.mark.parametrize("name,dtype", PROB_CASES, ids=str)
def test_probability_plane_in_ulps(name, dtype):
    _, _, B, C, _, _, _ = CASES[name]
    _, y, zk = inputs(name, dtype)
    _, prob, _ = run_target(name, dtype, 0.7, 100)
    valid = oc.valid_mask(y.numpy(), C)
    assert np.array_equal(prob.view(np.uint32) == 0x40000000, ~valid)          # sentinels exactly where the pixel is invalid
    want = oc.true_class_prob(zk, y.numpy(), C)[valid]
    got = prob[valid].astype(np.float64)
    ulp = np.abs(got - want) / np.spacing(want.astype(np.float32)).astype(np.float64)
    print("prob %s %s: max %.3f ulp, mean %.3f; smallest p %.3g" % (name, pc.dname(dtype), ulp.max(), ulp.mean(), want.min()))
    assert ulp.max() <= PROB_ULP
    assert (got >= 0).all() and (got <= 1.0).all()


# ---- loss and gradient --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=pc.dname)
@pytest.mark.parametrize("name", ["dense", "fused"])
def test_loss_and_gradient_are_the_cross_entropy_of_the_masked_target(name, dtype, weighted):
    o = ops()
    _, kind, B, C, _, size, _ = CASES[name]
    z, y, _ = inputs(name, dtype)
    yd = y.to(DEV)
    w = (0.5 + torch.rand(C, generator=torch.Generator().manual_seed(5))).to(DEV) if weighted else None
    N = int(oc.valid_mask(y.numpy(), C).sum())
    s = 4096.0 if dtype == F16 else 0.7
    for thresh, k in ((0.3, 0), (0.001, N // 2)):
        a = on_device(z).detach().requires_grad_(True)
        b = on_device(z).detach().requires_grad_(True)
        if kind == "dense":
            masked = o.ohem_target(a, yd, oc.IGNORE, thresh, k)
            la = o.ohem_cross_entropy(a, yd, oc.IGNORE, thresh=thresh, min_kept=k, weight=w)
            lb = o.cross_entropy(b, masked, oc.IGNORE, weight=w)
        else:
            masked = o.ohem_target(a, yd, oc.IGNORE, thresh, k, size=size, channels=C)
            la = o.upsample_ohem_cross_entropy(a, yd, size, C, oc.IGNORE, thresh=thresh, min_kept=k, weight=w)
            lb = o.upsample_cross_entropy(b, masked, size, C, oc.IGNORE, weight=w)
        (la * s).backward()
        (lb * s).backward()
        assert la.dtype == F32 and math.isfinite(la.item()) and a.grad.dtype == dtype
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(a.grad, b.grad)
        dropped = masked == oc.IGNORE
        assert 0 < int(dropped.sum()) < dropped.numel() and float(a.grad.abs().max()) > 0
        if kind == "dense":                          # a dropped pixel's gradient row is all zeros, a kept one's is not
            rows = a.grad.permute(0, 2, 3, 1).abs().amax(-1)
            assert float(rows[dropped].max()) == 0.0 and float(rows[~dropped].min()) > 0.0
        else:
            assert float(a.grad[:, C:].abs().max()) == 0.0


def test_nothing_kept_is_nan_as_torch():
    z, y, _ = inputs("dense", F32)
    dead = torch.full_like(y, oc.IGNORE).to(DEV)
    assert math.isnan(ops().ohem_cross_entropy(on_device(z), dead, oc.IGNORE, thresh=0.7, min_kept=10).item())


# ---- end to end against an fp64 rule that never sees the device plane ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=pc.dname)
def test_end_to_end_against_fp64(dtype):
    """Logits 2.5 * randn + 3 on the true class, rounded to the dtype.  On the host: thresh is the midpoint of the widest relative gap
    of the sorted fp64 p inside [0.6, 0.8], min_kept sits under the widest gap of the window [n0 + 50, n0 + 600] above
    n0 = count(p <= 0.7); both gaps are at least 1e-3 relative -- four orders above the plane's error -- before anything runs on the
    device.  Then the masked target is the fp64 rule's exactly and the loss is within predict_common.LOSS_TOL of fp64."""
    B, C, H, W = 2, 19, 33, 47
    y = oc.labels(B, H, W, C, 31)
    x = oc.logits(B, C, H, W, dtype, 32 + pc.DTYPES.index(dtype), y=y)
    p64 = oc.true_class_prob(x.double().permute(0, 2, 3, 1).numpy(), y.numpy(), C)
    live = np.sort(p64[oc.valid_mask(y.numpy(), C)])
    lo, hi = int(np.searchsorted(live, 0.6)), int(np.searchsorted(live, 0.8)) - 1
    i, gap_t = oc.widest_gap(live, lo, hi)
    thresh = 0.5 * (live[i] + live[i + 1])
    n0 = int((live <= 0.7).sum())
    assert n0 + 150 < len(live)                                        # the window ends at the last valid rank (N - n0 is ~300 here)
    j, gap_k = oc.widest_gap(live, n0 + 50 - 1, n0 + 600 - 1)          # live[j] is the (j + 1)-th smallest
    min_kept = j + 1
    print("end to end %s: thresh %.6f (gap %.3g), min_kept %d (gap %.3g), N %d" % (pc.dname(dtype), thresh, gap_t, min_kept, gap_k, len(live)))
    assert gap_t >= 1e-3 and gap_k >= 1e-3 and 0.6 <= thresh <= 0.8
    want, N, kept, theta, mode = oc.rule(p64, y.numpy(), C, thresh, min_kept)
    xd = x.to(DEV).contiguous(memory_format=CL)
    masked, state = ops().ohem_target(xd, y.to(DEV), oc.IGNORE, thresh, min_kept, want_state=True)
    assert np.array_equal(masked.cpu().numpy(), want)
    assert state.cpu().tolist()[:2] == [N, kept] and int(state[3]) == mode
    loss = ops().ohem_cross_entropy(xd, y.to(DEV), oc.IGNORE, thresh=thresh, min_kept=min_kept)
    ref = F.cross_entropy(x.double(), torch.from_numpy(want), ignore_index=oc.IGNORE)
    err = abs(loss.item() - ref.item()) / abs(ref.item())
    print("  loss %.9g vs fp64 %.9g, relative error %.3g (bound %.0e)" % (loss.item(), ref.item(), err, pc.LOSS_TOL[dtype]))
    assert err < pc.LOSS_TOL[dtype]


# ---- reproducibility and capture ------------------------------------------------------------------------------------------------------
def _fused_step(P, yd, size, C, thresh, k, w=None):
    masked, prob, state = ops().ohem_target(P, yd, oc.IGNORE, thresh, k, size=size, channels=C, want_prob=True, want_state=True)
    loss = ops().upsample_ohem_cross_entropy(P, yd, size, C, oc.IGNORE, thresh=thresh, min_kept=k, weight=w)
    grad, = torch.autograd.grad(loss, P)
    return prob, state, masked, loss.detach(), grad


def test_two_runs_are_bit_identical():
    name, dtype = "capped", BF16
    _, _, B, C, _, size, _ = CASES[name]
    z, y, _ = inputs(name, dtype)
    N = int(oc.valid_mask(y.numpy(), C).sum())
    for thresh, k in ((0.7, 1000), (0.0001, N - N // 5)):
        runs = [_fused_step(on_device(z).detach().requires_grad_(True), y.to(DEV), size, C, thresh, k) for _ in range(2)]
        for a, b in zip(*runs):
            assert torch.equal(a.view(torch.int32) if a.dtype == F32 else a, b.view(torch.int32) if b.dtype == F32 else b)
        assert math.isfinite(runs[0][3].item())


def test_graph_capture_replays_into_another_regime():
    """upsample_ohem_cross_entropy forward + backward captured in one graph on data in the k-th regime (thresh 0: no p is below it).
    Replays on new scores and labels land in keep-all (fewer valid pixels than min_kept), in the thresh regime (the true class 200
    below the others: p == 0 <= thresh on every pixel) and back in the k-th one, and each equals the eager run exactly: the regime
    is decided by the kernels, not at capture time."""
    name, dtype = "fused", BF16
    _, _, B, C, low, size, ld = CASES[name]
    z, y, _ = inputs(name, dtype)
    k, thresh = 2000, 0.0
    few = torch.full_like(y, oc.IGNORE)
    few[:, :20] = y[:, :20]                                           # 2 x 20 x 47 labels: under 2000 valid pixels
    z2 = inputs(name, F16)[0].float().to(dtype)
    z2[..., C:] = 1e30
    z4 = torch.zeros_like(z)
    z4[..., 4] = -200.0
    z4[..., C:] = 1e30
    y4 = torch.full_like(y, 4)
    data = [(z2, few, oc.KEEP_ALL), (z4, y4, oc.THRESH), (z, y, oc.KTH)]
    P = on_device(z.clone()).detach().requires_grad_(True)
    yd = y.clone().to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # warm-up outside the capture
        l0 = ops().upsample_ohem_cross_entropy(P, yd, size, C, oc.IGNORE, thresh=thresh, min_kept=k)
        torch.autograd.grad(l0, P)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = ops().upsample_ohem_cross_entropy(P, yd, size, C, oc.IGNORE, thresh=thresh, min_kept=k)
        grad, = torch.autograd.grad(loss, P)
    Pe = on_device(z.clone()).detach().requires_grad_(True)
    assert int(_fused_step(Pe, y.to(DEV), size, C, thresh, k)[1][3]) == oc.KTH          # the captured regime
    for zz, yy, mode in data:
        with torch.no_grad():
            P.copy_(on_device(zz))
            yd.copy_(yy.to(DEV))
        graph.replay()
        Pe = on_device(zz.clone()).detach().requires_grad_(True)
        _, state, _, le, ge = _fused_step(Pe, yy.to(DEV), size, C, thresh, k)
        assert int(state[3]) == mode, (state, mode)
        assert math.isfinite(le.item()) and float(ge.abs().max()) > 0
        assert torch.equal(loss.view(torch.int32), le.view(torch.int32)) and torch.equal(grad, ge), mode


# ---- the criterion on a model -----------------------------------------------------------------------------------------------------
def test_model_takes_the_criterion_on_both_heads():
    """DeepMobileNetV3PlusD, 2 x 96 x 128, criterion = criterion_aux = OhemCrossEntropy2d(min_kept=2000): training forward + backward
    run on the fused kernels (the main head never upsamples its scores to the input size); each head's loss equals the same model's
    loss with the plain criterion on the masked target ohem_target returned for that head's scores."""
    import deepv3_common as dc
    from mrfp_amd import _lib, ops as o
    from mrfp_amd.config import cfg
    from mrfp_amd.loss import OhemCrossEntropy2d
    from mrfp_amd.network import deepv3, wider_resnet
    B, H, W = 2, 96, 128
    cfg.MODEL.ACT_DTYPE = F32
    crit = OhemCrossEntropy2d(min_kept=2000)
    with contextlib.redirect_stdout(io.StringIO()):
        m = deepv3.DeepMobileNetV3PlusD(None, 19, crit, crit)
    m.load_state_dict(synth.synth_state_dict(dc.spec("DeepMobileNetV3PlusD"), seed=0))
    m = m.to(DEV).train()
    x, y = synth.synth_batch(B, H, W, seed=51)
    x, y = x.to(DEV), y.to(DEV)
    keep = ((torch.rand(B, 512, generator=torch.Generator().manual_seed(52)) >= dc.DSN_P).float() / (1.0 - dc.DSN_P))

    def step(gts, aux_gts):
        names, sizes, taps = [], [], []
        up, tgt, hook = o.upsample_bilinear, o.ohem_target, _lib.HOOK[0]

        def spy_up(t, size, *a, **k):
            sizes.append(tuple(size))
            return up(t, size, *a, **k)

        def spy_target(logits, target, *a, **k):
            out = tgt(logits, target, *a, **k)
            taps.append(out)
            return out
        m.zero_grad(set_to_none=True)
        wider_resnet.DROP_MASKS.injected = {"dsn": keep}
        _lib.HOOK[0] = lambda n, args: names.append(n)
        o.upsample_bilinear, o.ohem_target = spy_up, spy_target
        try:
            l1, l2 = m(x, gts=gts, aux_gts=aux_gts)
            (l1 + l2).backward()
        finally:
            o.upsample_bilinear, o.ohem_target, _lib.HOOK[0] = up, tgt, hook
            wider_resnet.DROP_MASKS.injected = None
        grad = m.final2[0].weight.grad.detach().clone()
        return l1.detach(), l2.detach(), grad, names, sizes, taps

    l1, l2, grad, names, sizes, taps = step(y, y)
    assert math.isfinite(l1.item()) and math.isfinite(l2.item()) and torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    for n in ("mrfp_upsample_ohem_target", "mrfp_ohem_target", "mrfp_upsample_ce_fwd", "mrfp_upsample_ce_bwd", "mrfp_ce_fwd", "mrfp_ce_bwd"):
        assert n in names, n
    assert (H, W) not in sizes and len(taps) == 2
    main = next(t for t in taps if tuple(t.shape) == (B, H, W))
    aux = next(t for t in taps if tuple(t.shape) != (B, H, W))
    assert 2000 <= int((main != 255).sum()) <= int((y != 255).sum()) and int((aux != 255).sum()) < 2000      # aux: min_kept > N, keep-all
    m.criterion = m.criterion_aux = nn.CrossEntropyLoss(ignore_index=255)
    p1, p2, pgrad, pnames, psizes, ptaps = step(main, aux)
    assert not ptaps and not [n for n in pnames if "ohem" in n] and (H, W) not in psizes
    assert torch.equal(l1, p1) and torch.equal(l2, p2) and torch.isfinite(pgrad).all()
