"""The stable segmented radix sort (csrc/sort.hip) and the Lovasz-Softmax loss (csrc/lovasz.hip) on the GPU.

sort_pairs: exactly numpy.argsort(kind="stable"), at the sizes where the kernels change path (T = mrfp_sort_tile_items(): below, at
and above one tile, several tiles, and more tiles per segment than one sweep of a scan workgroup, mrfp_sort_scan_sweep()).

The loss: against the float64 numpy restatement of lovasz_common at relative 1e-5 -- every term e_i g_i is non-negative, so nothing
cancels; the error is per-term rounding plus second-order effects of swapped near-ties (the fp32 restatement on the CPU is at 1e-7).
The gradient: against the float64 formula evaluated in the DEVICE'S OWN ORDER (a stable sort of ops.lovasz_errors' planes by (-e, flat
index)), so near-ties between fp32 and fp64 errors cannot swap ranks, at the per-element bars of the region loss's tests
(test_region_loss_gpu.GRAD_TOL: 2e-5 / 1.5e-2 / 1.5e-2 of the tensor maximum), which are the fused cross entropy's as well.  Inputs
are rounded to the activation dtype first."""
import contextlib
import functools
import io
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import lovasz_common as lv
import poison_common as pc
from mrfp_amd import synth
from test_region_loss_gpu import GRAD_TOL                   # the region loss's per-element bars, reused

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
LOSS_BAR = 1e-5
LOW, SIZE = (10, 13), (37, 53)


def dname(d):
    return str(d).replace("torch.", "")


def ops():
    from mrfp_amd import ops as o
    return o


def lib():
    from mrfp_amd import _lib
    return _lib.lib()


# ---- sort_pairs ---------------------------------------------------------------------------------------------------------------------
def as_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


def check_sort(keys, payload, offsets=None, bits=32):
    """keys, payload: uint32 arrays.  The device result equals the stable numpy sort of each segment on the low `bits` bits."""
    n = keys.shape[0]
    off = None if offsets is None else torch.tensor(offsets, dtype=torch.int64, device=DEV)
    k, p = ops().sort_pairs(as_i32(keys), as_i32(payload), off, bits)
    k, p = as_u32(k), as_u32(p)
    mask = np.uint32((1 << bits) - 1) if bits < 32 else np.uint32(0xFFFFFFFF)
    bounds = [0, n] if offsets is None else list(offsets)
    wk, wp = np.empty_like(keys), np.empty_like(payload)
    for a, b in zip(bounds[:-1], bounds[1:]):
        order = np.argsort(keys[a:b] & mask, kind="stable")
        wk[a:b], wp[a:b] = keys[a:b][order], payload[a:b][order]
    assert np.array_equal(k, wk) and np.array_equal(p, wp), (n, bits, offsets, int((k != wk).sum()), int((p != wp).sum()))


def sort_sizes():
    T, sweep = int(lib().mrfp_sort_tile_items()), int(lib().mrfp_sort_scan_sweep())
    # the last: more tiles in the segment than one sweep of a scan workgroup covers (kSortScanSweep tiles of kSortTile items), so the
    # scan carries a running sum from one sweep into the next
    return T, [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5], sweep * T + T + 3


def make_keys(kind, n, rng):
    if kind == "random":
        return (rng.integers(0, 1 << 32, n, dtype=np.uint64) | (1 << 31)).astype(np.uint32)          # the top bit set: no signed compare
    if kind == "equal":
        return np.full(n, 0x9E3779B9, dtype=np.uint32)
    if kind == "three":
        return rng.choice(np.array([0x00000001, 0x80000000, 0xFFFFFFFF], dtype=np.uint32), n)
    if kind == "ascending":
        return (np.arange(n, dtype=np.uint64) * 4099 + 7).astype(np.uint32)
    if kind == "descending":
        return (0xFFFFFFF0 - np.arange(n, dtype=np.uint64) * 4099).astype(np.uint32)
    assert kind == "bits30"
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)                             # garbage above bit 30


@pytest.mark.parametrize("kind", ["random", "equal", "three", "ascending", "descending", "bits30"])
def test_sort_pairs_equals_the_stable_numpy_sort(kind):
    T, sizes, big = sort_sizes()
    rng = np.random.default_rng(7)
    bits = 30 if kind == "bits30" else 32
    for n in sizes + ([big] if kind in ("random", "three", "bits30") else []):
        keys = make_keys(kind, n, rng)
        payload = np.arange(n, dtype=np.uint32)              # the input position: with equal keys the payload order must be preserved
        check_sort(keys, payload, None, bits)
    # an odd number of passes (the last one writes the outputs from the alternate buffers) and a single partial digit
    for b in (1, 5, 8, 9, 17, 24):
        keys = make_keys("random" if kind != "equal" else "equal", 2 * T + 9, rng)
        check_sort(keys, rng.integers(0, 1 << 32, 2 * T + 9, dtype=np.uint64).astype(np.uint32), None, b)


def test_sort_pairs_segments():
    """Unequal segments: a zero-length one, boundaries that are not tile-aligned, one of several tiles, one-element ones."""
    T, _, _ = sort_sizes()
    rng = np.random.default_rng(8)
    offsets = [0, 5, 5, 6, T + 7, T + 7, 4 * T + 70, 4 * T + 71, 5 * T]
    n = offsets[-1]
    for kind, bits in (("random", 32), ("three", 32), ("bits30", 30), ("equal", 32)):
        check_sort(make_keys(kind, n, rng), np.arange(n, dtype=np.uint32), offsets, bits)
    # equal segments, as the loss uses them
    check_sort(make_keys("three", 6 * 1000, rng), np.arange(6000, dtype=np.uint32), [1000 * i for i in range(7)], 30)
    # more segments than the scan grid has rows
    m = 40
    check_sort(make_keys("random", 37 * m, rng), np.arange(37 * m, dtype=np.uint32), [37 * i for i in range(m + 1)], 32)
    # the inputs are not written
    k = as_i32(make_keys("random", T + 1, rng))
    k0 = k.clone()
    ops().sort_pairs(k, k, None, 24)
    ops().sort_pairs(k, k, None, 32)
    assert torch.equal(k, k0)


# ---- the loss -------------------------------------------------------------------------------------------------------------------------
def chunk(dtype):
    return 16 // torch.empty((), dtype=dtype).element_size()


def on_device(x, dtype, ld=None):
    """Dense logits (ld None) or scores zero-padded to pitch ld, channels-last on the device, requiring a gradient."""
    if ld is not None:
        P = torch.zeros(x.shape[0], ld, x.shape[2], x.shape[3])
        P[:, :x.shape[1]] = x
        x = P
    return x.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)


def padded(C, dtype):
    """A score pitch with pad channels behind C rounded up to a chunk."""
    e = chunk(dtype)
    return (C + e - 1) // e * e + e


def bwd_scale(dtype):
    """0.7, or the 4096 loss scale of the float16 tests (1/#pixels gradients survive float16)."""
    return 4096.0 if dtype == F16 else 0.7


def upsampled(xc, size):
    return F.interpolate(xc, size, mode="bilinear", align_corners=True)


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def run_device(x, y, dtype, size=None, **kw):
    """-> (loss, gradient of the device tensor, error planes [C,B,H,W]) of the dense operator, or with `size` of the fused one."""
    C = x.shape[1]
    xd = on_device(x, dtype, None if size is None else padded(C, dtype))
    yd = y.to(DEV)
    if size is None:
        l = ops().lovasz_softmax(xd, yd, 255, **kw)
        planes = ops().lovasz_errors(xd, yd, 255)
    else:
        l = ops().upsample_lovasz_softmax(xd, yd, size, C, 255, **kw)
        planes = ops().lovasz_errors(xd, yd, 255, size=size, channels=C)
    (l * bwd_scale(dtype)).backward()
    assert l.dtype == F32 and xd.grad.dtype == dtype
    return l.detach(), xd.grad, planes


def check_case(x, y, dtype, size, what, **kw):
    """Loss within LOSS_BAR of the float64 reference; gradient within the region loss's bar of the float64 formula in the device's
    order (fused: taken to dP by autograd through F.interpolate(align_corners=True)); ignored rows and pad channels exactly zero."""
    C = x.shape[1]
    l, g, planes = run_device(x, y, dtype, size, **kw)
    xc = x.double().requires_grad_(True)
    z = xc if size is None else upsampled(xc, size)
    want = lv.ref_lovasz(z.detach().numpy(), y.numpy(), kw.get("classes", "present"), kw.get("per_image", False))
    _, gz = lv.ref_lovasz(z.detach().numpy(), y.numpy(), kw.get("classes", "present"), kw.get("per_image", False),
                          order_errors=planes.cpu().numpy(), want_grad=True)
    z.backward(torch.from_numpy(gz) * bwd_scale(dtype))
    le = abs(l.item() - want) / abs(want) if want != 0.0 else abs(l.item())
    ge = relerr(g[:, :C], xc.grad)
    print("%s: loss %.9g reference %.9g relerr %.3g; gradient relerr %.3g" % (what, l.item(), want, le, ge))
    assert math.isfinite(l.item()) and bool(torch.isfinite(g.float()).all())
    assert le < LOSS_BAR, (what, l.item(), want, le)
    assert ge < GRAD_TOL[dtype], (what, ge)
    if g.shape[1] > C:
        assert float(g[:, C:].abs().max()) == 0.0, what
    if size is None:
        invalid = ((y < 0) | (y >= C) | (y == 255)).to(DEV)
        assert int(invalid.sum()) > 0 and float(g.permute(0, 2, 3, 1)[invalid].abs().max()) == 0.0, what
    return l, g, planes


@pytest.mark.parametrize("C", [3, 19, 64])
def test_error_planes_against_the_fp64_softmax(C):
    """lovasz_errors of dense fp32 logits against |f - softmax64|; the bar is 4 x the largest deviation of torch.softmax in fp32 on the
    same inputs from the same float64 values: the same operations in a different order.  Invalid pixels hold the sentinel."""
    x, y = lv.make_case(2, C, SIZE[0], SIZE[1], F32, 100 + C)
    planes = ops().lovasz_errors(on_device(x, F32).detach(), y.to(DEV), 255).cpu().numpy().astype(np.float64)
    assert planes.shape == (C, 2) + SIZE
    p64 = lv.softmax64(x.numpy())
    valid = ((y >= 0) & (y < C) & (y != 255)).numpy()
    fg = np.stack([(y.numpy() == c) for c in range(C)], 1)
    e64 = np.abs(fg - p64).transpose(1, 0, 2, 3)
    e32 = np.abs(fg - torch.softmax(x, 1).numpy().astype(np.float64)).transpose(1, 0, 2, 3)
    bar = 4.0 * np.abs(e32 - e64)[:, valid].max()
    got = np.abs(planes - e64)[:, valid].max()
    print("C=%d: error planes deviate from float64 by %.3g; torch.softmax in fp32 by %.3g; bar %.3g" % (C, got, bar / 4.0, bar))
    assert got <= bar, (C, got, bar)
    assert np.all(planes[:, ~valid] == ops().LOVASZ_SENTINEL) and planes[:, valid].min() >= 0.0 and planes[:, valid].max() <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("C", [3, 19, 33])
def test_loss_and_gradient(C, dtype):
    """B = 2, 37 x 53 (dense, and fused from 10 x 13 scores with pad channels), ~10 % ignored, class C - 1 absent."""
    x, y = lv.make_case(2, C, SIZE[0], SIZE[1], dtype, 200 + C)
    check_case(x, y, dtype, None, "dense C=%d %s" % (C, dname(dtype)))
    x, y = lv.make_case(2, C, SIZE[0], SIZE[1], dtype, 300 + C, scale=2.0, low=LOW)
    check_case(x, y, dtype, SIZE, "fused C=%d %s" % (C, dname(dtype)))


def test_several_tiles_per_segment():
    """B = 2, 160 x 200, C = 5: 64 000 pixels per class segment -- several sort tiles and several coefficient tiles; per image too."""
    T = int(lib().mrfp_sort_tile_items())
    assert 2 * 160 * 200 > 8 * T and 160 * 200 > 4 * T
    x, y = lv.make_case(2, 5, 160, 200, F32, 400)
    check_case(x, y, F32, None, "dense 160x200")
    check_case(x, y, F32, None, "dense 160x200 per image", per_image=True)
    x, y = lv.make_case(2, 5, 160, 200, BF16, 401, scale=2.0, low=(40, 50))
    check_case(x, y, BF16, (160, 200), "fused 160x200")


@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
def test_all_classes_and_per_image_with_a_blank_image(fused):
    """classes='all' (the absent class C - 1 adds the largest p_c of the scope, and has a gradient); per_image with image 1 entirely
    ignored: the mean over the two images that count, image 1's gradient exactly zero."""
    C, size, low = 19, SIZE if fused else None, LOW if fused else None
    x, y = lv.make_case(3, C, SIZE[0], SIZE[1], F32, 500, scale=2.0, low=low, blank_image=1)
    assert int((y == C - 1).sum()) == 0
    la, _, _ = check_case(x, y, F32, size, "all classes", classes="all")
    lp, _, _ = check_case(x, y, F32, size, "present classes")
    assert la.item() != lp.item()
    for cl in ("present", "all"):
        _, g, _ = check_case(x, y, F32, size, "per image, %s" % cl, classes=cl, per_image=True)
        if not fused:
            assert float(g[1].abs().max()) == 0.0 and float(g[0].abs().max()) > 0.0 and float(g[2].abs().max()) > 0.0


@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
def test_everything_ignored_gives_zero_loss_and_gradient(fused):
    C = 19
    x = torch.randn(2, C, LOW[0], LOW[1])
    size = SIZE if fused else LOW
    y = torch.full((2,) + size, 255, dtype=torch.int64)
    y[0, 0, 0], y[1, 2, 3] = -1, C
    for cl in ("present", "all"):
        for per_image in (False, True):
            l, g, _ = run_device(x, y, BF16, size if fused else None, classes=cl, per_image=per_image)
            assert l.item() == 0.0 and float(g.abs().max()) == 0.0 and not bool(torch.isnan(g.float()).any()), (cl, per_image)


def test_a_single_class_present_and_one_class():
    # every valid pixel has label 2 of 5
    x, y = lv.make_case(2, 5, SIZE[0], SIZE[1], F32, 600)
    y[(y >= 0) & (y < 5)] = 2
    check_case(x, y, F32, None, "single class present")
    check_case(x, y, F32, None, "single class present, all", classes="all")
    # C = 1: p = 1 everywhere, every error 0: loss 0 and a zero gradient, finite
    x, y = lv.make_case(2, 1, SIZE[0], SIZE[1], F32, 601)
    assert int((y == 0).sum()) > 0
    for size, xs in ((None, x), (SIZE, x[:, :, :LOW[0], :LOW[1]].contiguous())):
        l, g, planes = run_device(xs, y, F32, size)
        assert l.item() == 0.0 and float(g.abs().max()) == 0.0
        assert lv.ref_lovasz(np.zeros((2, 1) + SIZE), y.numpy()) == 0.0


@functools.lru_cache(maxsize=None)
def tie_case():
    """bf16 scores scaled by 30: a good part of the pixels sit at p in {0, 1} exactly, so whole runs of errors are tied."""
    g = torch.Generator().manual_seed(700)
    x = (torch.randn(2, 19, LOW[0], LOW[1], generator=g) * 30.0).to(BF16).float()
    y = lv.lc.make_labels(2, 19, SIZE[0], SIZE[1], g)
    return x, y


def test_ties():
    x, y = tie_case()
    l, g, planes = check_case(x, y, BF16, SIZE, "ties")
    valid = ((y >= 0) & (y < 19) & (y != 255)).numpy()
    pv = planes.cpu().numpy()[:, valid.reshape(2, *SIZE)]
    tied = int(((pv == 0.0) | (pv == 1.0)).any(0).sum())
    print("ties: %d of %d valid pixels have an error of exactly 0 or 1 in some class" % (tied, int(valid.sum())))
    assert tied > 100
    # two runs: the same bits
    l2, g2, _ = run_device(x, y, BF16, SIZE)
    assert torch.equal(l.view(torch.int32), l2.view(torch.int32)) and torch.equal(pc.bits(g), pc.bits(g2))
    # and the same bits over poisoned fresh memory (workspace, saved buffers, gradient rows)
    def fn():
        a, b, _ = run_device(x, y, BF16, SIZE)
        c, d, _ = run_device(upsampled(x, SIZE), y, BF16, None, per_image=True)
        return pc.named(loss=a, dP=b, dense_loss=c, dlogits=d)
    sites = pc.run_three(fn)
    assert {"ops._region_forward", "ops._Scores.grad"} <= sites
    a, b, _ = run_device(x, y, BF16, SIZE)
    assert torch.equal(a.view(torch.int32), l.view(torch.int32)) and torch.equal(pc.bits(b), pc.bits(g))


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_fused_equals_dense(dtype):
    """upsample_lovasz_softmax(P) against lovasz_softmax of the full-resolution fp32 logits, at the loss bar.  fp32 scores: the logits
    are ops.upsample_bilinear(P).float().  16-bit scores: upsample_bilinear would round its output to 16 bits -- other logits than the
    fused kernel's fp32 interpolation sees, 2^-9 apart, which is no property of the loss kernels -- so the logits are the fp32
    interpolation of the same 16-bit scores (F.interpolate(P.float(), align_corners=True))."""
    C = 19
    x, y = lv.make_case(2, C, SIZE[0], SIZE[1], dtype, 800, scale=2.0, low=LOW)
    for kw in (dict(), dict(classes="all", per_image=True)):
        P = on_device(x, dtype, padded(C, dtype)).detach()
        lf = ops().upsample_lovasz_softmax(P, y.to(DEV), SIZE, C, 255, **kw)
        if dtype == F32:
            full = ops().upsample_bilinear(P, SIZE, channels=C).float()
        else:
            full = upsampled(P[:, :C].float(), SIZE)
        assert tuple(full.shape) == (2, C) + SIZE and full.dtype == F32
        ld = ops().lovasz_softmax(full, y.to(DEV), 255, **kw)
        err = abs(lf.item() - ld.item()) / abs(ld.item())
        print("fused %.9g dense %.9g relerr %.3g (%s %s)" % (lf.item(), ld.item(), err, dname(dtype), kw))
        assert err < LOSS_BAR, (dtype, kw, err)


def test_capture_forward_and_backward_in_one_graph():
    """Forward + backward captured on one stream (a chain: no parallel branches), replayed twice, on new scores the second time: the
    bits of the eager run.  Class presence is decided on the device, so the replay with another class set needs no new capture."""
    C = 19
    x, y = lv.make_case(2, C, SIZE[0], SIZE[1], BF16, 900, scale=2.0, low=LOW)
    x2, y2 = lv.make_case(2, C, SIZE[0], SIZE[1], BF16, 901, scale=2.0, low=LOW)
    y2[y2 == 3] = 255                                                   # class 3 leaves the present set
    P = on_device(x, BF16, padded(C, BF16)).detach().requires_grad_(True)
    yd = y.clone().to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up outside the capture
        l0 = ops().upsample_lovasz_softmax(P, yd, SIZE, C, 255)
        torch.autograd.grad(l0, P)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = ops().upsample_lovasz_softmax(P, yd, SIZE, C, 255)
        grad, = torch.autograd.grad(loss, P)
    for xx, yy in ((x, y), (x, y), (x2, y2)):
        with torch.no_grad():
            P.copy_(on_device(xx, BF16, padded(C, BF16)))
            yd.copy_(yy.to(DEV))
        graph.replay()
        Pe = on_device(xx, BF16, padded(C, BF16))
        le = ops().upsample_lovasz_softmax(Pe, yy.to(DEV), SIZE, C, 255)
        ge, = torch.autograd.grad(le, Pe)
        assert math.isfinite(le.item()) and float(ge.abs().max()) > 0
        assert torch.equal(loss.view(torch.int32), le.view(torch.int32)) and torch.equal(pc.bits(grad), pc.bits(ge))


# ---- the criterion on a model -----------------------------------------------------------------------------------------------------
def test_model_takes_ce_plus_lovasz_on_the_fused_path():
    """DeepMobileNetV3PlusD, 2 x 64 x 64, criterion = SumLoss((1.0, CE), (0.5, LovaszSoftmax2d())): training forward + backward run on the
    fused kernels (the main head never upsamples its scores to the input size), the loss is finite, and it equals 1.0 x the same
    model's loss with the cross entropy alone + 0.5 x its loss with the Lovasz criterion alone, each through loss.fused_loss."""
    import deepv3_common as dc
    from mrfp_amd import _lib, conv, loss as L, ops as o
    from mrfp_amd.network import deepv3, wider_resnet
    B, H, W = 2, 64, 64
    ce, lov = nn.CrossEntropyLoss(ignore_index=255), L.LovaszSoftmax2d()
    both = L.SumLoss((1.0, ce), (0.5, lov))
    assert L.fused_ce_kwargs(both) is not None
    with contextlib.redirect_stdout(io.StringIO()):
        m = deepv3.DeepMobileNetV3PlusD(None, dc.NC, both, ce)
    m.load_state_dict(synth.synth_state_dict(dc.spec("DeepMobileNetV3PlusD"), seed=0))
    m = m.to(DEV).train()
    x, y = synth.synth_batch(B, H, W, seed=61)
    x, y = x.to(DEV), y.to(DEV)
    keep = ((torch.rand(B, 512, generator=torch.Generator().manual_seed(62)) >= dc.DSN_P).float() / (1.0 - dc.DSN_P))

    def step(criterion):
        names, sizes = [], []
        up, hook = o.upsample_bilinear, _lib.HOOK[0]

        def spy_up(t, size, *a, **k):
            sizes.append(tuple(size))
            return up(t, size, *a, **k)
        m.criterion = criterion
        m.zero_grad(set_to_none=True)
        wider_resnet.DROP_MASKS.injected = {"dsn": keep}
        _lib.HOOK[0] = lambda n, args: names.append(n)
        o.upsample_bilinear = spy_up
        try:
            l1, l2 = m(x, gts=y, aux_gts=y)
            (l1 + 0.4 * l2).backward()
        finally:
            o.upsample_bilinear, _lib.HOOK[0] = up, hook
            wider_resnet.DROP_MASKS.injected = None
        grad = m.final2[0].weight.grad.detach().clone()
        return l1.detach(), grad, names, sizes

    try:
        ls, grad, names, sizes = step(both)
        for n in ("mrfp_upsample_lovasz_fwd", "mrfp_upsample_lovasz_bwd", "mrfp_upsample_ce_fwd", "mrfp_upsample_ce_bwd"):
            assert n in names, n
        assert (H, W) not in sizes                                   # the full-resolution logits were never written
        assert math.isfinite(ls.item()) and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
        lc_, _, _, _ = step(ce)
        ll, gl, lnames, _ = step(lov)
        assert "mrfp_upsample_lovasz_fwd" in lnames and bool(torch.isfinite(gl).all()) and float(gl.abs().max()) > 0
        assert torch.equal(ls, 1.0 * lc_ + 0.5 * ll), (ls.item(), lc_.item(), ll.item())
    finally:
        conv.backward_failed()
