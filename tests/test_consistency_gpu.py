"""The two-view consistency losses on the GPU (csrc/consist.hip) against the float64 torch restatements of consistency_common on the
CPU: dense logits and fused views (referenced as F.interpolate(P[:, :C].double(), size, mode="bilinear", align_corners=True)), the
criterion on a model, Trainer(loss_fn=) and harness.ConsistencyStep.

Bounds: the family's own (test_region_loss_gpu.LOSS_TOL / GRAD_TOL) -- loss relative 1e-5 (fp32) / 2e-3 (16-bit), gradient 2e-5 /
1.5e-2 of the tensor maximum.  Inputs follow the input rule of consistency_common (rounded to the activation dtype; ambiguous pixels
of kind 'hard' taken out), the two views are independent draws.

Shapes: C in {2, 19, 24, 25, 64} (two class-pad boundaries and the maximum built); dense 5 x 7 (less than one wave) and 33 x 65
(several workgroups per image and a tail); fused 5 x 7 -> 17 x 25 and 1 x 9 -> 6 x 33 with the score pitch equal to and larger than C
rounded to a chunk; a teacher of another geometry (3 x 4, another pitch); B = 3 with one image entirely ignored; one capped-grid case
where a workgroup walks its image more than once.  Kinds x T x thresholds x normalize: the Latin arrangement COMBOS."""
import contextlib
import functools
import io
import math

import pytest
import torch

import consistency_common as cc
from mrfp_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
LOSS_TOL = {F32: 1e-5, BF16: 2e-3, F16: 2e-3}          # test_region_loss_gpu.LOSS_TOL / GRAD_TOL
GRAD_TOL = {F32: 2e-5, BF16: 1.5e-2, F16: 1.5e-2}
CLASSES = [2, 19, 24, 25, 64]
DENSE = [(5, 7), (33, 65)]
FUSED = [((5, 7), (17, 25)), ((1, 9), (6, 33))]
# every kind with both temperatures; every threshold with both normalisations and both temperatures
COMBOS = [("kl", 1.0, None, "kept"), ("js", 2.0, None, "kept"), ("hard", 1.0, 0.3, "kept"), ("hard", 2.0, 0.5, "valid"),
          ("kl", 2.0, None, "valid"), ("js", 1.0, None, "valid"), ("hard", 2.0, 0.9, "kept"), ("hard", 1.0, 0.3, "valid"),
          ("hard", 1.0, 0.5, "kept"), ("hard", 2.0, 0.9, "valid")]


def dname(d):
    return str(d).replace("torch.", "")


def ops():
    from mrfp_amd import ops as o
    return o


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


def bwd_scale(dtype):
    """0.7, or the 4096 loss scale of the float16 tests (1/#pixels gradients survive float16)."""
    return 4096.0 if dtype == F16 else 0.7


def chunk(dtype):
    return 16 // torch.empty((), dtype=dtype).element_size()


def pitches(C, dtype):
    e = chunk(dtype)
    cr = (C + e - 1) // e * e
    return [cr, cr + 2 * e]


def on_device(x, dtype, ld=None, grad=True):
    """Dense logits (ld None) or scores zero-padded to pitch ld, channels-last on the device."""
    if ld is not None:
        P = torch.zeros(x.shape[0], ld, x.shape[2], x.shape[3])
        P[:, :x.shape[1]] = x
        x = P
    return x.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(grad)


def reference(xs, xt, valid, size, combo, scale, grad_s=True, grad_t=None):
    """-> (loss, counts, d student, d teacher or None) of the float64 restatement, the backward seeded with `scale`."""
    kind, T, thr, norm = combo
    grad_t = kind == "js" if grad_t is None else grad_t
    a, b = xs.double().requires_grad_(grad_s), xt.double().requires_grad_(grad_t)
    za, zb = (a, b) if size is None else (cc.upsampled(a, size), cc.upsampled(b, size))
    l, counts = cc.ref_consistency(za, zb, valid, kind, T, 0.0 if thr is None else thr, norm, want_counts=True)
    (l * scale).backward()
    return l.detach(), counts, a.grad, b.grad


def device(xs, xt, valid, size, C, combo, dtype, ld_s=None, ld_t=None, scale=1.0, grad_s=True, grad_t=None):
    kind, T, thr, norm = combo
    grad_t = kind == "js" if grad_t is None else grad_t
    a, b = on_device(xs, dtype, ld_s, grad_s), on_device(xt, dtype, ld_t, grad_t)
    kw = dict(kind=kind, temperature=T, threshold=0.0 if thr is None else thr, normalize=norm, want_counts=True)
    v = None if valid is None else valid.to(DEV)
    if size is None:
        l, counts = ops().consistency_loss(a, b, v, **kw)
    else:
        l, counts = ops().upsample_consistency_loss(a, b, size, C, v, **kw)
    (l * scale).backward()
    assert l.dtype == F32 and counts.dtype == torch.int64 and counts.is_cuda and tuple(counts.shape) == (2,)
    return l.detach(), tuple(int(c) for c in counts.cpu()), a, b


def check_grad(t, gref, C, dtype, what):
    assert t.grad is not None and t.grad.dtype == dtype, what
    ge = relerr(t.grad[:, :C], gref)
    print("%s: gradient relerr %.3g" % (what, ge))
    assert ge < GRAD_TOL[dtype], (what, ge)
    assert float(t.grad[:, C:].abs().max() if t.shape[1] > C else 0.0) == 0.0, what          # pad channels: exactly zero


def run(C, dtype, seed, what, combos, size=None, low_s=None, low_t=None, ld_s=None, ld_t=None, B=2, blank_image=None):
    H, W = size if size is not None else low_s
    for combo in combos:
        kind, T, thr, norm = combo
        thr = None if thr is None else cc.threshold_for(C, thr)
        combo = (kind, T, thr, norm)
        xs, xt, valid = cc.make_views(B, C, H, W, dtype, seed, low_s=low_s if size is not None else None,
                                      low_t=low_t if size is not None else None, threshold=thr, blank_image=blank_image)
        s = bwd_scale(dtype)
        lref, cref, gs, gt = reference(xs, xt, valid, size, combo, s)
        l, counts, a, b = device(xs, xt, valid, size, C, combo, dtype, ld_s, ld_t, s)
        name = "%s %s T=%g thr=%s %s" % (what, kind, T, thr, norm)
        assert counts == cref, (name, counts, cref)
        if cref[1] == 0:          # nobody confident in a small case: the empty denominator
            assert l.item() == 0.0 and lref.item() == 0.0 and float(a.grad.abs().max()) == 0.0, name
            continue
        le = abs(l.item() - lref.item()) / abs(lref.item())
        print("%s: loss %.6g relerr %.3g, counted %d kept %d" % (name, lref.item(), le, *cref))
        assert le < LOSS_TOL[dtype], (name, le)
        check_grad(a, gs, C, dtype, name + " student")
        if kind == "js":
            check_grad(b, gt, C, dtype, name + " teacher")
        else:
            assert b.grad is None, name
        if blank_image is not None:
            assert float(a.grad[blank_image].abs().max()) == 0.0 and float(a.grad.abs().max()) > 0.0, name


# ---- parity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("hw", DENSE, ids=str)
@pytest.mark.parametrize("C", CLASSES)
def test_dense(C, hw, dtype):
    run(C, dtype, 1000 + C + hw[0], "dense C=%d %s %s" % (C, hw, dname(dtype)), COMBOS, low_s=hw)


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("case", FUSED, ids=str)
@pytest.mark.parametrize("C", CLASSES)
def test_fused(C, case, dtype):
    low, size = case
    for k, ld in enumerate(pitches(C, dtype)):
        combos = [c for i, c in enumerate(COMBOS) if (i + i // 4) % 2 == k]          # every kind at either pitch
        run(C, dtype, 2000 + C + size[0], "fused C=%d %s ld=%d %s" % (C, case, ld, dname(dtype)), combos, size=size, low_s=low,
            low_t=low, ld_s=ld, ld_t=ld)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
@pytest.mark.parametrize("combo", [COMBOS[4], COMBOS[1], COMBOS[3]], ids=lambda c: c[0])
def test_a_teacher_of_another_geometry(combo, dtype):
    """The distillation case: the student's scores are 5 x 7 at the tight pitch, the teacher's 3 x 4 at a wider one."""
    C = 19
    tight, wide = pitches(C, dtype)
    run(C, dtype, 3000, "teacher 3x4 %s" % dname(dtype), [combo], size=(17, 25), low_s=(5, 7), low_t=(3, 4), ld_s=tight, ld_t=wide)
    run(C, dtype, 3001, "student 3x4 %s" % dname(dtype), [combo], size=(17, 25), low_s=(3, 4), low_t=(5, 7), ld_s=wide, ld_t=tight)


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
def test_one_image_entirely_ignored(fused, dtype):
    """B = 3, image 1 all 255, labels -1 and C present: the means skip it and its gradient rows are exactly 0."""
    if fused:
        run(19, dtype, 4000, "blank image fused %s" % dname(dtype), COMBOS[:4], size=(17, 25), low_s=(5, 7), low_t=(5, 7), ld_s=24,
            ld_t=24, B=3, blank_image=1)
    else:
        run(19, dtype, 4001, "blank image dense %s" % dname(dtype), COMBOS[:4], low_s=(33, 65), B=3, blank_image=1)


# ---- the capped grid: B = 64, 96 x 96, C = 3 -- ce_w_blocks_x gives 32 workgroups per image = 8 192 threads < 9 216 pixels ------------
CAP_B, CAP_S, CAP_C = 64, 96, 3
CAP_COMBOS = [("kl", 2.0, None, "kept"), ("js", 1.0, None, "kept"), ("hard", 1.0, 0.9, "valid")]


@functools.lru_cache(maxsize=None)
def capped_case(fused):
    """Inputs and float64 references of the capped-grid case, computed once and not modified."""
    low = (24, 24) if fused else None
    out = []
    for combo in CAP_COMBOS:
        xs, xt, valid = cc.make_views(CAP_B, CAP_C, CAP_S, CAP_S, BF16, 5000, low_s=low, low_t=low, threshold=combo[2])
        out.append((combo, xs, xt, valid, reference(xs, xt, valid, (CAP_S, CAP_S) if fused else None, combo, 1.0)))
    return out


@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
def test_capped_grid_and_two_runs(fused):
    """A workgroup walks its image more than once; two runs give identical bits for the loss, the gradients and the counts."""
    from mrfp_amd import _lib
    assert _lib.lib().mrfp_consist_nblocks(CAP_B, CAP_S * CAP_S) == 32 * CAP_B and 32 * 256 < CAP_S * CAP_S
    size, ld = ((CAP_S, CAP_S), 8) if fused else (None, None)
    for combo, xs, xt, valid, (lref, cref, gs, gt) in capped_case(fused):
        l1, c1, a1, b1 = device(xs, xt, valid, size, CAP_C, combo, BF16, ld, ld)
        l2, c2, a2, b2 = device(xs, xt, valid, size, CAP_C, combo, BF16, ld, ld)
        name = "capped %s %s" % ("fused" if fused else "dense", combo[0])
        assert torch.equal(l1.view(torch.int32), l2.view(torch.int32)) and c1 == c2 == cref, name
        assert torch.equal(a1.grad, a2.grad), name
        le = abs(l1.item() - lref.item()) / abs(lref.item())
        print("%s: loss relerr %.3g" % (name, le))
        assert le < LOSS_TOL[BF16], (name, le)
        check_grad(a1, gs, CAP_C, BF16, name + " student")
        if combo[0] == "js":
            assert torch.equal(b1.grad, b2.grad), name
            check_grad(b1, gt, CAP_C, BF16, name + " teacher")


# ---- behaviour ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
def test_js_gives_a_gradient_only_to_the_views_that_require_one(fused):
    C, dtype, combo = 19, BF16, ("js", 2.0, None, "kept")
    size, low, ld = ((17, 25), (5, 7), 32) if fused else (None, (33, 65), None)
    H, W = size if fused else low
    xs, xt, valid = cc.make_views(2, C, H, W, dtype, 6000, low_s=low if fused else None, low_t=low if fused else None)
    for grad_s, grad_t in ((True, False), (False, True)):
        _, _, gs, gt = reference(xs, xt, valid, size, combo, 0.7, grad_s, grad_t)
        l, _, a, b = device(xs, xt, valid, size, C, combo, dtype, ld, ld, 0.7, grad_s, grad_t)
        assert (a.grad is None) == (not grad_s) and (b.grad is None) == (not grad_t)
        check_grad(a if grad_s else b, gs if grad_s else gt, C, dtype, "js one view %s %s" % (grad_s, grad_t))
    for kind in ("kl", "hard"):          # a teacher that requires a gradient is still a constant of these kinds
        l, _, a, b = device(xs, xt, valid, size, C, (kind, 1.0, None, "kept"), dtype, ld, ld, 1.0, True, True)
        assert a.grad is not None and b.grad is None


@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
def test_extreme_logits_give_finite_values_inside_the_bounds(fused):
    """fp32 logits of +-80 with a different dominant class per view at about half of the pixels: confident, disagreeing views."""
    B, C = 2, 19
    h, w = (5, 7) if fused else (9, 11)
    size = (17, 25) if fused else None
    g = torch.Generator().manual_seed(7)
    ks = torch.randint(0, C, (B, h, w), generator=g)
    agree = torch.rand(B, h, w, generator=g) < 0.5
    kt = torch.where(agree, ks, (ks + 1 + torch.randint(0, C - 1, (B, h, w), generator=g)) % C)
    # (the dominant logit is 80 - u, u in [0, 1): halfway between two low-resolution pixels two dominant classes would tie exactly)
    xs = torch.full((B, C, h, w), -80.0).scatter_(1, ks[:, None], 80.0 - torch.rand(B, 1, h, w, generator=g))
    xt = torch.full((B, C, h, w), -80.0).scatter_(1, kt[:, None], 80.0 - torch.rand(B, 1, h, w, generator=g))
    if fused:          # (the input rule of kind 'hard': an interpolated near-tie may resolve either way in fp32)
        z = cc.upsampled(xt.double(), size)
        top = z.topk(2, dim=1).values
        valid = torch.where((top[:, 0] - top[:, 1]) < cc.MARGIN, 255, 0)
        assert float((valid == 255).double().mean()) <= cc.MAX_EXCLUDED
    else:
        valid = None
    for combo in (("kl", 1.0, None, "kept"), ("kl", 2.0, None, "kept"), ("js", 1.0, None, "kept"), ("js", 2.0, None, "kept"),
                  ("hard", 1.0, 0.0, "kept")):
        lref, cref, gs, gt = reference(xs, xt, valid, size, combo, 1.0)
        l, counts, a, b = device(xs, xt, valid, size, C, combo, F32, 20 if fused else None, 20 if fused else None)
        assert math.isfinite(l.item()) and bool(torch.isfinite(a.grad).all()) and counts == cref, combo
        le = abs(l.item() - lref.item()) / abs(lref.item())
        print("extreme %s T=%g: loss %.6g relerr %.3g" % (combo[0], combo[1], lref.item(), le))
        assert le < LOSS_TOL[F32], (combo, le)
        check_grad(a, gs, C, F32, "extreme %s student" % combo[0])
        if combo[0] == "js":
            assert bool(torch.isfinite(b.grad).all())
            check_grad(b, gt, C, F32, "extreme js teacher")


@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
def test_an_empty_denominator_gives_zero_loss_and_gradients(fused):
    C = 19
    size, low, ld = ((17, 25), (5, 7), 24) if fused else (None, (5, 7), None)
    H, W = size if fused else low
    xs, xt, valid = cc.make_views(2, C, H, W, BF16, 8000, low_s=low if fused else None, low_t=low if fused else None)
    blank = torch.full_like(valid, 255)
    blank[0, 0, 0], blank[1, 2, 3] = -1, C
    n = int(((valid >= 0) & (valid < C)).sum())
    cases = [((kind, 2.0, None, norm), blank, (0, 0)) for kind in cc.KINDS for norm in ("kept", "valid")]
    cases += [(("hard", 1.0, 1.0, norm), valid, (n, 0)) for norm in ("kept", "valid")]          # a threshold above every confidence
    for combo, v, want in cases:
        l, counts, a, b = device(xs, xt, v, size, C, combo, BF16, ld, ld)
        assert l.item() == 0.0 and counts == want, (combo, l.item(), counts)
        assert float(a.grad.abs().max()) == 0.0, combo
        if combo[0] == "js":
            assert float(b.grad.abs().max()) == 0.0, combo


def test_no_valid_map_counts_every_pixel_and_the_module_is_the_operator():
    from mrfp_amd import loss as L
    C, size, low = 19, (17, 25), (5, 7)
    xs, xt, _ = cc.make_views(2, C, size[0], size[1], BF16, 9000, low_s=low, low_t=(3, 4))
    combo = ("kl", 2.0, None, "kept")
    lref, cref, gs, _ = reference(xs, xt, None, size, combo, 1.0)
    l, counts, a, _ = device(xs, xt, None, size, C, combo, BF16, 24, 32)
    assert counts == cref == (2 * 17 * 25,) * 2 and abs(l.item() - lref.item()) < LOSS_TOL[BF16] * lref.item()
    check_grad(a, gs, C, BF16, "no valid map")
    crit = L.ConsistencyLoss2d("kl", temperature=2.0)
    a2, b2 = on_device(xs, BF16, 24), on_device(xt, BF16, 32, grad=False)
    lm = crit(L.ScoreMap(a2, size, C), L.ScoreMap(b2, size, C))
    lm.backward()
    assert torch.equal(lm.detach(), l) and torch.equal(a2.grad, a.grad)
    xd, xe = cc.make_views(2, C, 5, 7, BF16, 9001)[:2]
    d1, d2 = on_device(xd, BF16), on_device(xe, BF16, grad=False)
    assert torch.equal(crit(d1, d2).detach(), ops().consistency_loss(on_device(xd, BF16), d2, kind="kl", temperature=2.0).detach())


def test_refusals_launch_nothing():
    from mrfp_amd import _lib, loss as L
    E = _lib.MrfpHipError
    assert _lib.lib().mrfp_consist_max_classes() == ops().CONSIST_MAX_CLASSES == max(CLASSES)
    assert _lib.lib().mrfp_consist_loss_floats() == 6
    names, hook = [], _lib.HOOK[0]
    _lib.HOOK[0] = lambda n, args: names.append(n)
    try:
        dense = torch.zeros(2, 19, 17, 25, device=DEV).contiguous(memory_format=CL)
        P = torch.zeros(2, 24, 5, 7, device=DEV).contiguous(memory_format=CL)
        crit = L.ConsistencyLoss2d("js")
        with pytest.raises(E, match="mixed"):
            crit(L.ScoreMap(P, (17, 25), 19), dense)
        with pytest.raises(E, match="mixed"):
            crit(dense, L.ScoreMap(P, (17, 25), 19))
        with pytest.raises(E, match="one dtype"):
            ops().consistency_loss(dense, dense.bfloat16())
        with pytest.raises(E, match="one dtype"):
            ops().upsample_consistency_loss(P, P.half(), (17, 25), 19)
        big = torch.zeros(1, 65, 3, 3, device=DEV).contiguous(memory_format=CL)
        with pytest.raises(E, match="<= 64"):
            ops().consistency_loss(big, big)
        with pytest.raises(E, match="<= 64"):
            ops().upsample_consistency_loss(torch.zeros(1, 72, 3, 3, device=DEV), torch.zeros(1, 72, 3, 3, device=DEV), (5, 5), 65)
        with pytest.raises(E, match="GPU"):
            ops().consistency_loss(dense, dense.cpu())
        assert names == []
        # the entry itself refuses a wider C, with the limit in the message, before its launch
        buf = torch.zeros(64, device=DEV)
        with pytest.raises(E, match="1 <= C <= 64"):
            _lib.call("mrfp_consist_fwd", big.data_ptr(), big.data_ptr(), None, 0, 1, 9, 65, 0, 1.0, 0.0, 0, buf[8:].data_ptr(),
                      buf.data_ptr(), _lib.stream())
        torch.cuda.synchronize()
        assert float(buf.abs().max()) == 0.0
    finally:
        _lib.HOOK[0] = hook


# ---- model and Trainer: the smallest configuration of test_region_loss_gpu's model test ------------------------------------------------
class _DeepWrap(torch.nn.Module):
    """A network/deepv3.py factory behind the call Trainer makes: returns the factory's [main_loss, aux_loss]."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, img, label, training=True):
        return self.net(img, gts=label, aux_gts=label)


@contextlib.contextmanager
def model_setup():
    """-> (build(seed) -> a DeepMobileNetV3PlusD on the device, x, y): fp32 activations and an injected dropout mask, restored after."""
    import deepv3_common as dc
    from mrfp_amd import conv
    from mrfp_amd.config import cfg
    from mrfp_amd.network import deepv3, wider_resnet
    x, y = synth.synth_batch(2, 64, 64, seed=31)
    keep = (torch.rand(2, 512, generator=torch.Generator().manual_seed(32)) >= dc.DSN_P).float() / (1.0 - dc.DSN_P)

    def build(seed=0):
        sd = synth.synth_state_dict(dc.spec("DeepMobileNetV3PlusD"), seed=seed)
        crit = torch.nn.CrossEntropyLoss(ignore_index=255)
        with contextlib.redirect_stdout(io.StringIO()):
            m = deepv3.DeepMobileNetV3PlusD(None, dc.NC, crit, crit)
        m.load_state_dict(sd)
        return m.to(DEV)
    before = cfg.MODEL.ACT_DTYPE
    cfg.MODEL.ACT_DTYPE = F32
    wider_resnet.DROP_MASKS.injected = {"dsn": keep}
    try:
        yield build, x.to(DEV), y.to(DEV)
    finally:
        wider_resnet.DROP_MASKS.injected = None
        cfg.MODEL.ACT_DTYPE = before
        conv.backward_failed()


def grads_of(m):
    from mrfp_amd import conv
    conv.join_wgrad_stream()
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def test_keep_scores_changes_no_bit_and_the_kept_scores_backpropagate():
    import deepv3_common as dc
    from mrfp_amd import loss as L
    with model_setup() as (build, x, y):
        runs = []
        for keep_scores in (False, True):
            m = build().train()
            m.keep_scores = keep_scores
            out = m(x, gts=y, aux_gts=y)
            (out[0] + out[1]).backward()
            runs.append((out[0].detach().clone(), out[1].detach().clone(), grads_of(m), m))
        (l0, a0, g0, m0), (l1, a1, g1, m1) = runs
        assert m0.last_scores is None and isinstance(m1.last_scores, L.ScoreMap)
        assert torch.equal(l0, l1) and torch.equal(a0, a1) and g0.keys() == g1.keys() and len(g0) > 100
        for n in g0:
            assert torch.equal(g0[n].view(torch.int32), g1[n].view(torch.int32)), n
        sm = m1.last_scores
        assert sm.size == (64, 64) and sm.channels == dc.NC and sm.P.requires_grad and sm.P.shape[2] < 64 and sm.P.shape[3] < 64
        assert sm.P.shape[1] % 8 == 0 and sm.P.shape[1] >= dc.NC
        # a second criterion over the kept scores: crit(model.last_scores, teacher scores) reaches the parameters
        m = build().train()
        m.keep_scores = True
        teacher = build(seed=1).eval()
        m(x, gts=y, aux_gts=y)
        with torch.no_grad():
            Pt = teacher(x, training=False, low_res=True)
        cons = L.ConsistencyLoss2d("kl", temperature=2.0)(m.last_scores, L.ScoreMap(Pt, (64, 64), dc.NC), y)
        assert math.isfinite(cons.item()) and cons.item() > 0.0
        cons.backward()
        g = grads_of(m)
        f2 = g["final2.0.weight"]
        assert bool(torch.isfinite(f2).all()) and float(f2.abs().max()) > 0.0
        first = [n for n in g if n.startswith("layer0")]
        assert first and any(float(g[n].abs().max()) > 0.0 for n in first)


def test_a_pass_through_loss_fn_is_the_plain_trainer_bit_for_bit():
    from mrfp_amd.harness import Trainer
    with model_setup() as (build, x, y):
        def two_steps(**kw):
            tr = Trainer(_DeepWrap(build()).train(), lr=1e-2, loss_weights=(1.0, 0.4), **kw)
            losses = [tr.step(x, y).detach().clone() for _ in range(2)]
            torch.cuda.synchronize()
            return losses, tr.opt.flat_p.detach().clone()
        l0, p0 = two_steps()
        l1, p1 = two_steps(loss_fn=lambda m, i, l: m(i, l, training=True))
        assert all(torch.equal(a, b) for a, b in zip(l0, l1)) and torch.equal(p0.view(torch.int32), p1.view(torch.int32))
        assert bool(torch.isfinite(p0).all())


def test_one_consistency_step_with_a_second_model_as_teacher():
    from mrfp_amd import _lib, loss as L
    from mrfp_amd.harness import ConsistencyStep, Trainer
    with model_setup() as (build, x, y):
        teacher = build(seed=1).eval()
        state = {k: v.detach().clone() for k, v in teacher.state_dict().items()}
        step = ConsistencyStep(L.ConsistencyLoss2d("js", temperature=2.0), weight=0.5, teacher=teacher)
        seen = []

        def recorded(m, i, l):
            out = step(m, i, l)
            seen.append(out)
            return out
        model = _DeepWrap(build()).train()
        tr = Trainer(model, lr=1e-2, loss_weights=(1.0, 0.4, 1.0), loss_fn=recorded)
        p0 = tr.opt.flat_p.detach().clone()
        names, hook = [], _lib.HOOK[0]
        _lib.HOOK[0] = lambda n, args: names.append(n)
        try:
            loss = tr.step(x, y)
            torch.cuda.synchronize()
        finally:
            _lib.HOOK[0] = hook
        assert "mrfp_upsample_consist_fwd" in names and "mrfp_upsample_consist_bwd" in names
        assert len(seen) == 1 and isinstance(seen[0], list) and len(seen[0]) == 3          # [main, aux, weight * consistency]
        main, aux, cons = (float(t.detach()) for t in seen[0])
        assert all(math.isfinite(v) for v in (main, aux, cons)) and 0.0 < cons <= 0.5 * 4.0 * math.log(2.0)
        assert abs(float(loss.detach()) - (main + 0.4 * aux + cons)) <= 1e-5 * abs(main + 0.4 * aux + cons)
        assert model.net.keep_scores is False and model.net.last_scores is None          # nothing is retained behind the step
        p1 = tr.opt.flat_p.detach()
        assert bool(torch.isfinite(p1).all()) and not torch.equal(p0, p1)
        after = teacher.state_dict()
        assert after.keys() == state.keys()
        for k, v in state.items():
            assert torch.equal(after[k], v), k
        assert all(p.grad is None for p in teacher.parameters())
