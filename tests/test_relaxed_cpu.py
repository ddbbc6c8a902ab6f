"""No-GPU checks of boundary label relaxation and the joint-weighted soft-NLL loss: the numpy restatement against what the
reference's own transform wrote (tests/golden/relaxed.npz), the translation reading of scipy.ndimage.shift, the float64 loss
restatement in the published shape against the closed form the kernels compute, the criterion routing, and the refusals that need no
device."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import relaxed_common as rc
from mrfp_amd import _lib, build

C = rc.GOLDEN_C
NEW = ("mrfp_relax_nblocks", "mrfp_relax_labels", "mrfp_multihot_pack", "mrfp_relax_word_counts", "mrfp_relax_class_weights",
       "mrfp_soft_nll_nblocks", "mrfp_soft_nll_loss_floats", "mrfp_soft_nll_fwd", "mrfp_soft_nll_bwd", "mrfp_upsample_soft_nll_fwd",
       "mrfp_upsample_soft_nll_bwd")


@pytest.fixture(scope="module")
def cdll():
    build.build()
    return _lib.lib()


def golden_cases():
    return [(n, b, s) for n in rc.GOLDEN_MAPS + ("tiny",) for b in rc.GOLDEN_BORDERS for s in rc.GOLDEN_STRICT]


def test_numpy_relaxation_equals_the_reference_transform():
    """Every word of every golden case: 5 label maps x border 0, 1, 2 x STRICTBORDERCLASS None / [5, 11]."""
    g = rc.golden()
    for name, border, sname in golden_cases():
        want = g[rc.golden_key(name, border, sname)]
        got = rc.np_relax(g[name + "_lab"], C, border, rc.GOLDEN_STRICT[sname])
        assert want.dtype == np.int32 and got.dtype == np.int32
        np.testing.assert_array_equal(got, want, err_msg=str((name, border, sname)))
    # the cases say something: relaxation sets several bits, the strict classes keep one, the all-255 map is the ignore bit alone
    k = lambda w: rc.unpack(w, C).sum(-3)
    assert k(g[rc.golden_key("blocky", 0, "none")]).max() == 1 and k(g[rc.golden_key("blocky", 2, "none")]).max() >= 3
    lab = g["lines_lab"]
    strict = g[rc.golden_key("lines", 2, "s5_11")]
    assert (k(strict)[(lab == 5) | (lab == 11)] == 1).all() and (k(g[rc.golden_key("lines", 2, "none")])[lab == 5] > 1).any()
    assert (g[rc.golden_key("all255", 1, "none")] == 1 << C).all()
    np.testing.assert_array_equal(rc.unpack(g[rc.golden_key("tiny", 1, "none")], C), g["tiny_multihot"])
    assert g["tiny_multihot"].shape == (C + 1, 5, 7) and g["tiny_multihot"].dtype == np.uint8


def test_spline_shift_at_integer_offsets_is_a_translation():
    """scipy.ndimage.shift(order=3, cval=C) -- the reference's call -- on the golden label maps (255 -> C first, as the reference
    does) equals the constant-fill translation for every offset of a border-3 window."""
    from scipy.ndimage import shift
    g = rc.golden()
    for name in rc.GOLDEN_MAPS + ("tiny",):
        a = g[name + "_lab"].copy()
        a[a == 255] = C
        H, W = a.shape
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                want = np.full_like(a, C)
                ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
                yo, xo = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0))
                want[ys, xs] = a[yo, xo]
                np.testing.assert_array_equal(shift(a, (dy, dx), cval=C), want, err_msg=str((name, dy, dx)))


def test_counts_and_weights_restatement():
    words = np.array([[[0b011, 0b100 | 1 << 4], [0b001, 1 << 4]], [[1 << 4] * 2] * 2], dtype=np.int32)          # C = 4
    n = rc.np_counts(words, 4)
    assert n.tolist() == [[2, 1, 1, 0, 2], [0, 0, 0, 0, 4]]
    w = rc.np_weights(n, 1.0, False, False)
    assert w.dtype == np.float32 and w.shape == (2, 4)
    np.testing.assert_array_equal(w, np.array([[1 + (1 - 2 / 6), 1 + (1 - 1 / 6), 1 + (1 - 1 / 6), 1.0], [1.0] * 4]).astype(np.float32))
    # pooled: n = [2, 1, 1, 0] of 10 words' bits in all (the ignore plane's 6 count in the total): 1 + 2 / 0.2, 1 + 2 / 0.1
    assert rc.np_weights(n, 2.0, True, True).tolist() == [11.0, 21.0, 21.0, 1.0]


def test_loss_restatement_equals_the_closed_form():
    """log max(p_c, q) summed over the set with -1/k in front IS -(W/k) log q = (W/k) (lse_all - lse_set): 1e-12 in float64, with
    and without weights, on targets with k from 1 to several, an all-ignored image and 255 runs; and the gradients agree."""
    B, H, W = 3, 12, 14
    y = rc.make_label_maps(B, H, W, C, 5, all_ignored_image=1)
    for border in (0, 1, 2):
        words = rc.np_relax(y.numpy(), C, border)
        k = rc.unpack(words, C)[:, :C].sum(1)
        assert (k[1] == 0).all() and (k.max() == 1 if border == 0 else k.max() >= 3)
        for w in (None, rc.make_weights(C, 7).double(), rc.make_weights(C, 8, rows=B).double()):
            x = rc.make_logits(B, C, H, W, torch.float32, 11 + border).double()
            xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
            la, lb = rc.ref_loss(xa, words, C, w), rc.closed_form(xb, words, C, w)
            assert abs(la.item() - lb.item()) <= 1e-12 * abs(lb.item()), (border, la.item(), lb.item())
            la.backward()
            lb.backward()
            assert (xa.grad - xb.grad).abs().max().item() <= 1e-12 * xb.grad.abs().max().item()
            assert float(xa.grad[1].abs().max()) == 0.0          # the all-ignored image


def test_restatement_on_an_all_ignored_image_and_on_wide_sets():
    """An all-ignored image: loss 0 (0 / (0 + 1)), not NaN.  One pixel with the set {0, 2} of 3 classes and weights w:
    -(w0 + w2) / 2 * log(p0 + p2) / (1 + 1)."""
    x = torch.tensor([1.0, -0.5, 0.25], dtype=torch.float64).view(1, 3, 1, 1)
    none = np.array([[[1 << 3]]], dtype=np.int32)
    assert rc.ref_loss(x, none, 3).item() == 0.0 and rc.closed_form(x, none, 3).item() == 0.0
    w = torch.tensor([0.5, 7.0, 1.25], dtype=torch.float64)
    p = torch.softmax(x.view(3), 0)
    want = -(0.5 + 1.25) / 2 * torch.log(p[0] + p[2]) / 2
    for words in (np.array([[[0b0101]]], dtype=np.int32), np.array([[[0b1101]]], dtype=np.int32)):       # the ignore bit changes nothing
        assert abs(rc.ref_loss(x, words, 3, w).item() - want.item()) < 1e-15
    # k = 1 is the weighted cross entropy of that class over (1 + 1)
    one = np.array([[[0b0010]]], dtype=np.int32)
    assert abs(rc.ref_loss(x, one, 3, w).item() - (-7.0 * torch.log(p[1]) / 2).item()) < 1e-15


def test_symbols_declared_and_exported(cdll):
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos and hasattr(cdll, name), name
    assert ctypes.c_double in protos["mrfp_relax_class_weights"][1]
    nb = cdll.mrfp_relax_nblocks
    assert nb(1, 1, 1) == 1 and nb(2, 67, 130) == 2 * 9 and nb(16, 768, 768) == 16 * 128 and nb(1025, 33, 2) == 1025
    assert cdll.mrfp_soft_nll_nblocks(3, 419 * 419) == 3 * 682 and cdll.mrfp_soft_nll_loss_floats(16) == 17


def test_refusals_through_the_c_abi(cdll):
    """C = 32, border = 9, a wstride that is neither 0 nor C, a null pointer: each entry returns the error with its own text; the
    pointers are into a host buffer, so nothing is launched."""
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255

    def relax(C=19, border=1, t=p, w=p):
        return ("mrfp_relax_labels", (t, 2, 4, 4, C, border, 0, w, p, None))

    def pack(C=19, m=p):
        return ("mrfp_multihot_pack", (m, 2, 16, C, p, p, None))

    def wcounts(C=19, c=p):
        return ("mrfp_relax_word_counts", (p, 2, 16, C, c, None))

    def weights(C=19, c=p):
        return ("mrfp_relax_class_weights", (c, 2, C, 1.0, 0, 0, p, None))

    def dense_f(C=19, ws=0, dtype=0, x=p):
        return ("mrfp_soft_nll_fwd", (x, p, dtype, 2, 16, C, p, ws, p, p, None))

    def dense_b(C=19, ws=0, dtype=0, x=p):
        return ("mrfp_soft_nll_bwd", (x, p, p, p, p, dtype, 2, 16, C, p, ws, None))

    def up_f(C=19, ws=0, dtype=0, ld=32, x=p):
        return ("mrfp_upsample_soft_nll_fwd", (x, ld, p, dtype, 2, 2, 2, 4, 4, C, p, ws, p, p, None))

    def up_b(C=19, ws=0, dtype=0, ld=32, Cd=20, x=p):
        return ("mrfp_upsample_soft_nll_bwd", (x, ld, p, p, p, p, Cd, dtype, 2, 2, 2, 4, 4, C, p, ws, None))

    cases = [(relax(border=9), b"relax_labels: 0 <= border <= 8 (border=9)"), (relax(border=-1), b"relax_labels: 0 <= border <= 8 (border=-1)"),
             (relax(t=None), b"relax_labels: null pointer"), (relax(w=None), b"relax_labels: null pointer"),
             (pack(m=None), b"multihot_pack: null pointer"), (wcounts(c=None), b"relax_word_counts: null pointer"),
             (weights(c=None), b"relax_class_weights: null pointer"),
             (up_f(ld=19), b"upsample_soft_nll_fwd: the score buffer must be channel-padded to 16-byte chunks (ld=19)"),
             (up_b(Cd=32), b"upsample_soft_nll_bwd: ld a 16-byte multiple, Cd = C rounded up to one (ld=32 Cd=32)")]
    for mk, who in ((relax, b"relax_labels"), (pack, b"multihot_pack"), (wcounts, b"relax_word_counts"), (weights, b"relax_class_weights"),
                    (dense_f, b"soft_nll_fwd"), (dense_b, b"soft_nll_bwd"), (up_f, b"upsample_soft_nll_fwd"), (up_b, b"upsample_soft_nll_bwd")):
        cases += [(mk(C=32), who + b": 1 <= C <= 31 (C=32)"), (mk(C=0), who + b": 1 <= C <= 31 (C=0)")]
    for mk, who in ((dense_f, b"soft_nll_fwd"), (dense_b, b"soft_nll_bwd"), (up_f, b"upsample_soft_nll_fwd"), (up_b, b"upsample_soft_nll_bwd")):
        cases += [(mk(ws=7), who + b": wstride must be 0 (one weight row) or C (one per image) (wstride=7 C=19)"),
                  (mk(dtype=99), who + b": unknown dtype 99"), (mk(x=None), who + b": null pointer")]
    for (name, args), text in cases:
        assert len(args) == len(_lib.ARG_NAMES[name]), name
        rc_ = getattr(cdll, name)(*args)
        assert rc_ == -1 and cdll.mrfp_last_error() == text, (name, rc_, cdll.mrfp_last_error())


class _Foreign(nn.Module):
    def forward(self, x, y):
        return x.sum()


def test_criterion_routing(monkeypatch):
    """fused_ce_kwargs / fused_loss send ImgWtLossSoftNLL to ops.soft_nll / ops.upsample_soft_nll with the relaxed words and the
    weights of their counts, by the form of the target; what they return for the criteria that existed before is unchanged."""
    from mrfp_amd import loss
    crit = loss.ImgWtLossSoftNLL(19, upper_bound=2.0, norm=True, border=2, strict_classes=[5, 11])
    kw = loss.fused_ce_kwargs(crit)
    assert kw is not None and kw["soft_nll"].__self__ is crit
    calls = []
    monkeypatch.setattr(loss.ops, "relax_labels", lambda *a, **k: calls.append(("relax", a, k)) or ("WORDS", "COUNTS"))
    monkeypatch.setattr(loss.ops, "pack_multihot", lambda *a, **k: calls.append(("pack", a, k)) or ("PWORDS", "PCOUNTS"))
    monkeypatch.setattr(loss.ops, "relaxed_counts", lambda *a, **k: calls.append(("counts", a, k)) or "WCOUNTS")
    monkeypatch.setattr(loss.ops, "relaxed_class_weights", lambda *a, **k: calls.append(("weights", a, k)) or "W")
    monkeypatch.setattr(loss.ops, "soft_nll", lambda *a, **k: calls.append(("dense", a, k)) or "L")
    monkeypatch.setattr(loss.ops, "upsample_soft_nll", lambda *a, **k: calls.append(("up", a, k)) or "U")
    monkeypatch.setattr(loss.ops, "cross_entropy", lambda *a, **k: calls.append(("ce", a, k)) or "CE")
    monkeypatch.setattr(loss.ops, "upsample_cross_entropy", lambda *a, **k: calls.append(("upce", a, k)) or "UCE")
    labels = torch.zeros(2, 4, 4, dtype=torch.int64)
    words = torch.zeros(2, 4, 4, dtype=torch.int32)
    multihot = torch.zeros(2, 20, 4, 4, dtype=torch.uint8)
    assert loss.fused_loss(crit, "P", labels, (8, 8), 19) == "U"
    assert calls == [("relax", (labels, 19, 2, [5, 11]), dict(want_counts=True)), ("weights", ("COUNTS", 2.0, True, False), {}),
                     ("up", ("P", "WORDS", (8, 8), 19), dict(weight="W"))]
    del calls[:]
    assert loss.fused_loss(crit, "x", words) == "L" and crit("x", multihot) == "L"
    assert calls == [("counts", (words, 19), {}), ("weights", ("WCOUNTS", 2.0, True, False), {}), ("dense", ("x", words, 19), dict(weight="W")),
                     ("pack", (multihot,), dict(want_counts=True)), ("weights", ("PCOUNTS", 2.0, True, False), {}),
                     ("dense", ("x", "PWORDS", 19), dict(weight="W"))]
    with pytest.raises(ValueError):
        crit("x", torch.zeros(2, 19, 4, 4, dtype=torch.uint8))          # C planes, not C + 1
    with pytest.raises(ValueError):
        crit("x", torch.zeros(2, 4, 4, dtype=torch.float32))
    # the criteria that existed before: the same mapping, the same calls
    del calls[:]
    assert loss.fused_ce_kwargs(nn.CrossEntropyLoss(ignore_index=255)) == dict(ignore_index=255, weight=None, label_smoothing=0.0,
                                                                              reduction="mean", per_image=False)
    ib = loss.ImageBasedCrossEntropyLoss2d(19, norm=True, upper_bound=2.0)
    kw = loss.fused_ce_kwargs(ib)
    assert kw["weight"].__self__ is ib and {k: v for k, v in kw.items() if k != "weight"} == dict(
        ignore_index=255, label_smoothing=0.0, reduction="mean", per_image=True)
    assert loss.fused_ce_kwargs(_Foreign()) is None and loss.fused_ce_kwargs(nn.CrossEntropyLoss(reduction="none")) is None
    assert loss.fused_loss(_Foreign(), "x", "y") is None
    monkeypatch.setattr(loss.ops, "label_class_weights", lambda *a: calls.append(("lcw", a)) or ["LW"])
    assert loss.fused_loss(nn.CrossEntropyLoss(ignore_index=7), "x", "labels") == "CE"
    assert loss.fused_loss(ib, "P", "labels", (8, 8), 19) == "UCE"
    assert calls == [("ce", ("x", "labels", 7), dict(weight=None, label_smoothing=0.0, reduction="mean", per_image=False)),
                     ("lcw", ("labels", 19, 2.0, True, False)),
                     ("upce", ("P", "labels", (8, 8), 19, 255), dict(weight=["LW"], label_smoothing=0.0, reduction="mean", per_image=True))]


def test_refusals_that_need_no_device():
    from mrfp_amd import input_pipeline, loss, ops
    from mrfp_amd.config import cfg
    with pytest.raises(ValueError):
        loss.ImgWtLossSoftNLL(19, weights=torch.ones(19))
    with pytest.raises(_lib.MrfpHipError):
        loss.ImgWtLossSoftNLL(32)
    with pytest.raises(_lib.MrfpHipError):
        loss.ImgWtLossSoftNLL(19, border=9)
    with pytest.raises(_lib.MrfpHipError):
        loss.ImgWtLossSoftNLL(19, strict_classes=[19])
    c = loss.ImgWtLossSoftNLL(19)
    assert (c.num_classes, c.ignore_index, c.upper_bound, c.norm, c.batch_weights, c.border, c.strict_classes) == (19, 255, 1.0, False, False, 1, None)
    assert ops.strict_class_mask([5, 11], 19) == (1 << 5) | (1 << 11) and ops.strict_class_mask(None, 19) == 0
    cpu = torch.zeros(1, 4, 4, dtype=torch.int64)
    for f in (lambda: ops.relax_labels(cpu, 19), lambda: ops.relax_labels(cpu, 32), lambda: ops.relax_labels(cpu, 19, border=9),
              lambda: ops.pack_multihot(torch.zeros(1, 20, 4, 4, dtype=torch.uint8)), lambda: ops.relaxed_counts(cpu.int(), 19),
              lambda: ops.relaxed_class_weights(torch.zeros(1, 20, dtype=torch.int64))):
        with pytest.raises(_lib.MrfpHipError):
            f()
    # the reference's settings and their defaults (config.py:56-64); the transform reads them at call time
    assert (cfg.BATCH_WEIGHTING, cfg.BORDER_WINDOW, cfg.STRICTBORDERCLASS) == (False, 1, None)
    from mrfp_amd.dropin import config as dropin_config
    assert dropin_config.cfg is cfg
    with pytest.raises(ValueError):
        input_pipeline.RelaxedBoundaryTarget(19, ignore_id=3)
    t = input_pipeline.RelaxedBoundaryTarget(19)
    words = torch.from_numpy(rc.golden()[rc.golden_key("tiny", 1, "none")])
    np.testing.assert_array_equal(t.to_multihot(words).numpy(), rc.golden()["tiny_multihot"])
