"""The two-view consistency losses without a GPU: the float64 restatements of consistency_common pinned against torch's own
functions and an independent numpy loop, the properties of the definitions, and the wiring -- header entries, argument refusals
before the library is touched, ConsistencyLoss2d as a model's criterion, Trainer(loss_fn=).enable_graph()."""
import contextlib
import io
import math

import pytest
import torch
import torch.nn.functional as F

import consistency_common as cc


def views(seed=0, B=2, C=3, H=4, W=5, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    zs = (torch.randn(B, C, H, W, generator=g) * scale).double()
    zt = (torch.randn(B, C, H, W, generator=g) * scale).double()
    valid = torch.randint(0, C, (B, H, W), generator=g)
    valid[0, 0, 0], valid[1, 2, 3], valid[1, 0, 1], valid[0, 3, 4] = 255, 255, -1, C
    return zs, zt, valid


# ---- the restatements ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1.0, 2.0])
def test_kl_is_torch_kl_div(T):
    zs, zt, _ = views(1, C=19)
    n = zs.shape[0] * zs.shape[2] * zs.shape[3]
    want = F.kl_div(F.log_softmax(zs / T, 1), F.softmax(zt / T, 1), reduction="sum") * T * T / n
    got = cc.ref_consistency(zs, zt, None, "kl", T)
    assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item())


def test_hard_with_threshold_zero_is_cross_entropy_against_the_argmax():
    zs, zt, valid = views(2, C=19)
    got, (n, nk) = cc.ref_consistency(zs, zt, None, "hard", threshold=0.0, want_counts=True)
    want = F.cross_entropy(zs, zt.argmax(1))
    assert n == nk == zs.shape[0] * zs.shape[2] * zs.shape[3]
    assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item())
    y = torch.where(cc.counted_mask(valid, 19, valid.shape), zt.argmax(1), torch.full_like(valid, 255))
    got = cc.ref_consistency(zs, zt, valid, "hard")
    want = F.cross_entropy(zs, y, ignore_index=255)
    assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item())


@pytest.mark.parametrize("masked", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("kind,T,threshold,normalize", [
    ("kl", 1.0, 0.0, "kept"), ("kl", 2.0, 0.0, "kept"), ("js", 1.0, 0.0, "kept"), ("js", 2.0, 0.0, "kept"),
    ("hard", 1.0, 0.0, "kept"), ("hard", 1.0, 0.5, "kept"), ("hard", 1.0, 0.5, "valid"), ("hard", 2.0, 0.9, "kept"),
    ("hard", 1.0, 0.9, "valid")])
def test_the_three_kinds_against_a_numpy_loop(kind, T, threshold, normalize, masked):
    zs, zt, valid = views(3)
    assert tuple(zs.shape) == (2, 3, 4, 5)
    valid = valid if masked else None
    got, counts = cc.ref_consistency(zs, zt, valid, kind, T, threshold, normalize, want_counts=True)
    want, wcounts = cc.np_consistency(zs.numpy(), zt.numpy(), None if valid is None else valid.numpy(), kind, T, threshold, normalize)
    assert counts == wcounts and counts[0] == (36 if masked else 40)
    if kind == "hard" and threshold > 0.0:
        assert 0 < counts[1] < counts[0]            # the threshold does select
    assert abs(got.item() - want) <= 1e-12 * abs(want)


def test_hard_takes_the_first_maximum():
    zt = torch.zeros(1, 4, 1, 2, dtype=torch.float64)
    zt[0, :, 0, 0] = torch.tensor([1.0, 3.0, 3.0, 0.0])
    zt[0, :, 0, 1] = torch.tensor([2.0, 2.0, 2.0, 2.0])
    assert cc.first_argmax(zt).flatten().tolist() == [1, 0]
    zs = torch.randn(1, 4, 1, 2, dtype=torch.float64)
    want = F.cross_entropy(zs, torch.tensor([[[1, 0]]]))
    assert abs(cc.ref_consistency(zs, zt, None, "hard").item() - want.item()) < 1e-12


def test_fused_views_are_restated_on_the_upsampled_scores():
    g = torch.Generator().manual_seed(4)
    Ps = torch.randn(2, 19, 5, 7, generator=g).double().requires_grad_(True)
    Pt = torch.randn(2, 19, 3, 4, generator=g).double()
    l = cc.ref_consistency(cc.upsampled(Ps, (17, 25)), cc.upsampled(Pt, (17, 25)), None, "kl", 2.0)
    l.backward()
    assert tuple(Ps.grad.shape) == (2, 19, 5, 7) and float(Ps.grad.abs().max()) > 0.0
    corner = F.interpolate(Ps.detach(), (17, 25), mode="bilinear", align_corners=True)[:, :, 0, 0]
    assert torch.equal(corner, Ps.detach()[:, :, 0, 0])          # align-corners


# ---- properties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1.0, 2.0])
def test_js_is_symmetric_in_its_views_and_bounded(T):
    zs, zt, valid = views(5, C=19)
    a = cc.ref_consistency(zs, zt, valid, "js", T).item()
    b = cc.ref_consistency(zt, zs, valid, "js", T).item()
    assert abs(a - b) <= 1e-14 and 0.0 < a <= T * T * math.log(2.0)
    xs, xt = zs.clone().requires_grad_(True), zt.clone().requires_grad_(True)
    cc.ref_consistency(xs, xt, valid, "js", T).backward()
    ys, yt = zs.clone().requires_grad_(True), zt.clone().requires_grad_(True)
    cc.ref_consistency(yt, ys, valid, "js", T).backward()
    assert torch.allclose(xs.grad, ys.grad, rtol=0, atol=1e-15) and torch.allclose(xt.grad, yt.grad, rtol=0, atol=1e-15)


@pytest.mark.parametrize("kind", ["kl", "js"])
def test_identical_views_give_zero_and_a_zero_gradient(kind):
    zs, _, valid = views(6, C=19)
    x = zs.clone().requires_grad_(True)
    l = cc.ref_consistency(x, zs.clone(), valid, kind, 2.0)
    l.backward()
    assert abs(l.item()) < 1e-15 and float(x.grad.abs().max()) < 1e-15


def test_the_teacher_is_a_constant_of_kl_and_hard():
    zs, zt, _ = views(7)
    for kind in ("kl", "hard"):
        xs, xt = zs.clone().requires_grad_(True), zt.clone().requires_grad_(True)
        cc.ref_consistency(xs, xt, None, kind).backward()
        assert xt.grad is None and float(xs.grad.abs().max()) > 0.0
    xs, xt = zs.clone().requires_grad_(True), zt.clone().requires_grad_(True)
    cc.ref_consistency(xs, xt, None, "js").backward()
    assert float(xt.grad.abs().max()) > 0.0


def test_kl_gradient_is_T_over_N_times_p_minus_q():
    zs, zt, valid = views(8)
    T = 2.0
    x = zs.clone().requires_grad_(True)
    cc.ref_consistency(x, zt, valid, "kl", T).backward()
    m = cc.counted_mask(valid, 3, valid.shape)
    want = (T / int(m.sum())) * (F.softmax(zs / T, 1) - F.softmax(zt / T, 1)) * m[:, None]
    assert torch.allclose(x.grad, want, rtol=0, atol=1e-15)


@pytest.mark.parametrize("kind", cc.KINDS)
def test_an_empty_denominator_gives_zero_and_a_zero_gradient(kind):
    zs, zt, valid = views(9)
    x = zs.clone().requires_grad_(True)
    l, counts = cc.ref_consistency(x, zt, torch.full_like(valid, 255), kind, want_counts=True)
    l.backward()
    assert l.item() == 0.0 and counts == (0, 0) and float(x.grad.abs().max()) == 0.0
    if kind == "hard":          # nobody is confident
        for normalize in ("kept", "valid"):
            x = zs.clone().requires_grad_(True)
            l, counts = cc.ref_consistency(x, zt, valid, kind, threshold=1.0, normalize=normalize, want_counts=True)
            l.backward()
            assert l.item() == 0.0 and counts == (36, 0) and float(x.grad.abs().max()) == 0.0


def test_extreme_logits_are_finite_in_the_restatement():
    zs = torch.full((1, 5, 1, 3), -80.0, dtype=torch.float64)
    zt = zs.clone()
    zs[:, 0], zt[:, 1] = 80.0, 80.0
    for kind, want in (("kl", 160.0), ("js", math.log(2.0)), ("hard", 160.0)):
        x = zs.clone().requires_grad_(True)
        l = cc.ref_consistency(x, zt, None, kind)
        l.backward()
        assert math.isfinite(l.item()) and bool(torch.isfinite(x.grad).all())
        assert abs(l.item() - want) <= 1e-9 * want, (kind, l.item())


@pytest.mark.parametrize("C", [2, 19, 24, 25, 64])
def test_the_input_rule_takes_few_pixels_out(C):
    """The condition the GPU cases rely on, on the shapes they use: at most 2 % of the pixels are excluded (make_views asserts it)."""
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        for thr in (0.3, 0.5, 0.9):
            cc.make_views(2, C, 33, 65, dtype, 100 + C, threshold=cc.threshold_for(C, thr))
            cc.make_views(2, C, 17, 25, dtype, 200 + C, low_s=(5, 7), low_t=(5, 7), threshold=cc.threshold_for(C, thr))
            cc.make_views(2, C, 6, 33, dtype, 300 + C, low_s=(1, 9), low_t=(1, 9), threshold=cc.threshold_for(C, thr))


def test_sixteen_bit_dense_cases_do_contain_ties():
    _, xt, _ = cc.make_views(2, 64, 33, 65, torch.bfloat16, 164, threshold=0.5)
    top = xt.topk(2, dim=1).values
    assert int((top[:, 0] == top[:, 1]).sum()) > 0


# ---- wiring ----------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("mrfp_consist_fwd", "mrfp_consist_bwd", "mrfp_upsample_consist_fwd", "mrfp_upsample_consist_bwd")


def test_the_header_declares_the_entries_with_named_arguments():
    from mrfp_amd import _lib
    protos = _lib.parse_header()
    for name in ENTRIES + ("mrfp_consist_nblocks", "mrfp_consist_ws_floats", "mrfp_consist_loss_floats", "mrfp_consist_max_classes"):
        assert name in protos and name in _lib.ARG_NAMES, name
    names = _lib.ARG_NAMES
    assert names["mrfp_consist_fwd"][:3] == ["logits_s", "logits_t", "valid"] and names["mrfp_consist_fwd"][-3:] == ["ws", "loss", "stream"]
    for e in ENTRIES:
        for arg in ("valid", "dtype", "B", "C", "kind", "temperature", "threshold", "stream"):
            assert arg in names[e], (e, arg)
    for e in ENTRIES[2:]:
        for arg in ("P_s", "ld_s", "Hi_s", "Wi_s", "P_t", "ld_t", "Hi_t", "Wi_t", "H", "W"):
            assert arg in names[e], (e, arg)
    for e in (ENTRIES[1], ENTRIES[3]):
        for arg in ("loss", "gscale", "dlogits_s", "dlogits_t"):
            assert arg in names[e], (e, arg)
    assert "Cd" in names[ENTRIES[3]] and "normalize" in names[ENTRIES[0]] and "normalize" in names[ENTRIES[2]]


def test_every_argument_refusal_comes_before_the_library(monkeypatch):
    from mrfp_amd import _lib, loss as L, ops

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "call", lambda *a: no_library())
    monkeypatch.setattr(ops, "call", lambda *a: no_library())
    E = _lib.MrfpHipError
    s, t = torch.zeros(2, 19, 5, 7), torch.zeros(2, 19, 5, 7)
    y = torch.zeros(2, 5, 7, dtype=torch.int64)
    for kw in (dict(kind="mse"), dict(kind=None), dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")),
               dict(temperature=float("inf")), dict(temperature="warm"), dict(threshold=-0.1), dict(threshold=1.5),
               dict(threshold=float("nan")), dict(normalize="all"), dict(normalize=None)):
        with pytest.raises(E):
            ops.consistency_loss(s, t, **kw)
        with pytest.raises(E):
            ops.upsample_consistency_loss(torch.zeros(2, 24, 5, 7), torch.zeros(2, 24, 5, 7), (17, 25), 19, **kw)
        with pytest.raises(E):
            L.ConsistencyLoss2d(**kw)
    with pytest.raises(E, match="4-D"):
        ops.consistency_loss(s[0], t)
    with pytest.raises(E, match="one dtype"):
        ops.consistency_loss(s, t.bfloat16())
    with pytest.raises(E, match="one dtype"):
        ops.consistency_loss(s.double(), t.double())
    with pytest.raises(E, match="one shape"):
        ops.consistency_loss(s, torch.zeros(2, 19, 5, 8))
    with pytest.raises(E, match="<= 64"):
        ops.consistency_loss(torch.zeros(1, 65, 3, 3), torch.zeros(1, 65, 3, 3))
    with pytest.raises(E, match="<= 64"):
        ops.upsample_consistency_loss(torch.zeros(1, 72, 3, 3), torch.zeros(1, 72, 3, 3), (5, 5), 65)
    with pytest.raises(E, match="valid"):
        ops.consistency_loss(s, t, y.int())
    with pytest.raises(E, match="valid"):
        ops.consistency_loss(s, t, y[:, :4])
    with pytest.raises(E, match="batch size"):
        ops.upsample_consistency_loss(torch.zeros(2, 24, 5, 7), torch.zeros(3, 24, 3, 4), (17, 25), 19)
    with pytest.raises(E, match="channel-padded"):
        ops.upsample_consistency_loss(torch.zeros(2, 24, 5, 7), torch.zeros(2, 19, 3, 4), (17, 25), 19)
    with pytest.raises(E, match="channel-padded"):
        ops.upsample_consistency_loss(torch.zeros(2, 16, 5, 7), torch.zeros(2, 24, 3, 4), (17, 25), 19)
    with pytest.raises(E, match="valid"):
        ops.upsample_consistency_loss(torch.zeros(2, 24, 5, 7), torch.zeros(2, 24, 3, 4), (17, 25), 19, y)
    with pytest.raises(E, match="GPU"):          # the last refusal: everything else is in order, the tensors live on the host
        ops.consistency_loss(s, t, y)
    with pytest.raises(E, match="GPU"):
        ops.upsample_consistency_loss(torch.zeros(2, 24, 5, 7), torch.zeros(2, 32, 3, 4), (17, 25), 19)
    crit = L.ConsistencyLoss2d("js", temperature=2.0)
    with pytest.raises(E, match="mixed"):
        crit(L.ScoreMap(torch.zeros(2, 24, 5, 7), (17, 25), 19), torch.zeros(2, 19, 17, 25))
    with pytest.raises(E, match="one output size"):
        crit(L.ScoreMap(torch.zeros(2, 24, 5, 7), (17, 25), 19), L.ScoreMap(torch.zeros(2, 24, 5, 7), (17, 26), 19))
    assert ops.CONSIST_MAX_CLASSES == 64 and ops.CONSIST_KINDS == {"kl": 0, "js": 1, "hard": 2}


def test_consistency_loss_is_no_inputs_targets_criterion():
    from mrfp_amd import deepv3, loss as L
    crit = L.ConsistencyLoss2d("hard", threshold=0.9, normalize="valid")
    assert L.fused_ce_kwargs(crit) is None and L.fused_loss(crit, None, None) is None
    assert L.fused_ce_kwargs(L.SumLoss((1.0, torch.nn.CrossEntropyLoss()), (0.5, crit))) is None
    with pytest.raises(TypeError, match="not an \\(inputs, targets\\) criterion"):
        crit(torch.zeros(2, 19, 5, 7), torch.zeros(2, 5, 7, dtype=torch.int64))

    class Bare(deepv3._DeepLabBase):
        pass
    for attr in ("criterion", "criterion_aux"):
        with pytest.raises(TypeError, match="ConsistencyLoss2d"):
            setattr(Bare(), attr, crit)
    m = Bare()
    m.criterion = torch.nn.CrossEntropyLoss(ignore_index=255)          # an ordinary criterion is still a registered submodule
    assert "criterion" in dict(m.named_children()) and m.keep_scores is False and m.last_scores is None
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(TypeError, match="harness.ConsistencyStep"):
            deepv3.simpleDeepV3Plus(19, criterion=crit)
        from mrfp_amd.network import deepv3 as factories
        with pytest.raises(TypeError, match="ConsistencyLoss2d"):
            factories.DeepMobileNetV3PlusD(None, 19, torch.nn.CrossEntropyLoss(), crit)
        for cls in (deepv3.MRFPPlus, deepv3.simpleDeepV3Plus, factories.DeepV3Plus):
            assert cls.keep_scores is False and issubclass(cls, deepv3._DeepLabBase)


def test_trainer_takes_a_loss_fn_and_graph_mode_refuses_it():
    from mrfp_amd import _lib, loss as L
    from mrfp_amd.harness import ConsistencyStep, Trainer
    for bad in (3, "step", [1]):
        with pytest.raises(ValueError, match="loss_fn"):
            Trainer(torch.nn.Linear(5, 3), loss_fn=bad)
    assert Trainer(torch.nn.Linear(5, 3)).loss_fn is None
    tr = Trainer(torch.nn.Linear(5, 3), loss_fn=lambda m, i, l: m(i).sum())
    with pytest.raises(_lib.MrfpHipError, match="loss_fn"):
        tr.enable_graph()
    step = ConsistencyStep(L.ConsistencyLoss2d("kl"), weight=0.5)
    assert step.weight == 0.5 and step.teacher is None and step.valid_from_labels
    with pytest.raises(_lib.MrfpHipError, match="loss_fn"):
        Trainer(torch.nn.Linear(5, 3), loss_fn=step).enable_graph()
    with pytest.raises(TypeError):
        ConsistencyStep(torch.nn.CrossEntropyLoss())
    with pytest.raises(ValueError):
        ConsistencyStep(L.ConsistencyLoss2d(), weight=float("nan"))
    with pytest.raises(TypeError, match="no head"):
        step(torch.nn.Linear(5, 3), torch.zeros(1, 5), None)
