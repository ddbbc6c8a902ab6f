"""No-GPU, no-library checks of the loss operators' layer in mrfp_amd/ops.py: one autograd function over (score source, criterion)
whose C arguments are looked up by the names include/mrfp_hip.h gives them.  The public operators run here on CPU tensors with
the launch, the stream query, the device check and the library's size functions replaced by stubs; what they would hand to each
of the 14 entries is compared, name by name, with the values the call was given.  And the host-side refusals, verbatim."""
import pytest
import torch

from mrfp_amd import _lib, ops

B, C, H, W, HI, WI, LD = 2, 5, 9, 7, 3, 2, 12          # all different, so that a transposed argument shows
IGNORE, EPS, THRESH, KEPT = 11, 0.25, 0.5, 20
ENTRIES = [p + s + d for p in ("mrfp_", "mrfp_upsample_") for s in ("ce", "ce_w", "soft_nll") for d in ("_fwd", "_bwd")] \
    + ["mrfp_ohem_target", "mrfp_upsample_ohem_target"]


class _Sizes:
    """the library's size functions, as far as the operators ask"""
    mrfp_ce_nblocks = staticmethod(lambda npix: 3)
    mrfp_ce_w_nblocks = mrfp_soft_nll_nblocks = staticmethod(lambda b, hw: 4)
    mrfp_ce_w_loss_floats = staticmethod(lambda b, mode: 1 + (b if mode == 2 else 1))
    mrfp_soft_nll_loss_floats = staticmethod(lambda b: 1 + b)
    mrfp_ohem_ws_bytes = staticmethod(lambda b, hw: 64)


@pytest.fixture
def launches(monkeypatch):
    _lib.parse_header()
    seen = []
    monkeypatch.setattr(ops, "call", lambda name, *args: seen.append((name, args)))
    monkeypatch.setattr(ops, "stream", lambda: 77)
    monkeypatch.setattr(ops, "_chk", lambda x, name="x": x)
    monkeypatch.setattr(_lib, "lib", lambda: _Sizes)
    return seen


def _operands():
    x = torch.zeros(B, C, H, W).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    P = torch.zeros(B, LD, HI, WI).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    return x, P, torch.zeros(B, H, W, dtype=torch.int64), torch.zeros(B, H, W, dtype=torch.int32), torch.ones(B, C)


def test_every_entry_gets_its_arguments_by_name(launches):
    """Each of the 14 entries receives exactly the header's argument list, and under every name the value that belongs to it:
    logits / P the scores, target / words the labels, the geometry the entry names, the criterion's own arguments, the outputs."""
    x, P, y, words, w = _operands()
    for s, up in ((x, ()), (P, ((H, W), C))):
        ce, nll = (ops.upsample_cross_entropy, ops.upsample_soft_nll) if up else (ops.cross_entropy, ops.soft_nll)
        ce(s, y, *up, IGNORE).backward()
        ce(s, y, *up, IGNORE, weight=w, label_smoothing=EPS, per_image=True).backward()
        (nll(s, words, *up, weight=w) if up else nll(s, words, C, weight=w)).backward()
        ops.ohem_target(s, y, IGNORE, THRESH, KEPT, **(dict(size=up[0], channels=up[1]) if up else {}))
    assert [n for n, _ in launches if n != "mrfp_bilinear_bwd"] == ENTRIES[:6] + ENTRIES[12:13] + ENTRIES[6:12] + ENTRIES[13:]
    value = dict(dtype=_lib.F32, B=B, HW=H * W, npix=B * H * W, H=H, W=W, Hi=HI, Wi=WI, ld=LD, C=C, Cd=8, ignore_index=IGNORE,
                 wstride=C, smoothing=EPS, mode=2, thresh=THRESH, min_kept=KEPT, stream=77, weight=w.data_ptr(),
                 target=y.data_ptr(), words=words.data_ptr())
    for name, args in launches:
        names = _lib.ARG_NAMES[name]
        assert len(args) == len(names), name
        got = dict(zip(names, args))
        scores = P if "upsample" in name or name == "mrfp_bilinear_bwd" else x
        if name != "mrfp_bilinear_bwd":
            assert got["P" if scores is P else "logits"] == scores.data_ptr(), name
            for n in names:
                assert n not in value or got[n] == value[n], (name, n, got[n])
                assert got[n] is not None, (name, n)
    # the fused backward tail: d(loss)/d(logits) at pitch Cd, then the bilinear backward to pitch ld (12 != 8: dP is zeroed first)
    tails = [args for n, args in launches if n == "mrfp_bilinear_bwd"]
    assert len(tails) == 3 and all(a[2:] == (_lib.F32, B, HI, WI, H, W, 8, LD, 77) for a in tails)
    assert x.grad.shape == x.shape and P.grad.shape == P.shape and P.grad.is_contiguous(memory_format=torch.channels_last)


def test_plain_and_general_criteria(launches):
    """The four keywords at their defaults take the plain entries; `_general=True` alone forces the weighted ones with a null weight
    pointer, wstride 0, smoothing 0 and mode 0."""
    x, P, y, _, _ = _operands()
    ops.upsample_cross_entropy(P, y, (H, W), C).backward()
    ops.cross_entropy(x, y, _general=True).backward()
    names = [n for n, _ in launches]
    assert names == ["mrfp_upsample_ce_fwd", "mrfp_upsample_ce_bwd", "mrfp_bilinear_bwd", "mrfp_ce_w_fwd", "mrfp_ce_w_bwd"]
    for name, args in launches[3:]:
        got = dict(zip(_lib.ARG_NAMES[name], args))
        assert (got["weight"], got["wstride"], got["smoothing"], got["mode"], got["ignore_index"]) == (None, 0, 0.0, 0, 255)


def test_a_missing_name_raises_before_the_launch(launches):
    env = {n: i for i, n in enumerate(_lib.ARG_NAMES["mrfp_ce_w_fwd"])}
    ops._call_named("mrfp_ce_w_fwd", dict(env, extra=1))
    assert launches == [("mrfp_ce_w_fwd", tuple(range(13)) + (77,))]
    del launches[:]
    for lost in ("wstride", "logits", "ws"):
        with pytest.raises(KeyError, match=lost):
            ops._call_named("mrfp_ce_w_fwd", {k: v for k, v in env.items() if k != lost})
    assert not launches
    # the names under which the records offer their values cover every entry, whatever the source and the criterion
    x, P, y, words, w = _operands()
    for src in (ops._Scores(x), ops._Scores(P, (H, W), C)):
        for crit in (ops._PlainCe("t", 255), ops._WeightedCe("t", 255, 0.0, "mean", False), ops._SoftNll("t", C)):
            target, weight = crit.check(src, words if crit.stem == "soft_nll" else y, w)
            for d, more in (("_fwd", {"ws"}), ("_bwd", {"gscale", "dlogits"} | ({"Cd"} if src.fused else set()))):
                have = set(ops._loss_env(src, crit, target, weight, y)) | more | {"stream"}
                assert set(_lib.ARG_NAMES[src.prefix + crit.stem + d]) <= have


def _message(fn, *args, **kw):
    with pytest.raises(_lib.MrfpHipError) as e:
        fn(*args, **kw)
    return str(e.value)


def test_refusals_verbatim():
    """The host-side messages that need no GPU tensor, as they were before the operators were folded."""
    cpu = torch.device("cpu")

    def opt(weight=None, label_smoothing=0.0, reduction="mean", per_image=False):
        return _message(ops._ce_options, "cross_entropy", weight, label_smoothing, reduction, per_image, 2, 19, cpu)

    assert opt(reduction="none") == "cross_entropy: reduction must be 'mean' or 'sum' (got 'none'; 'none' stays the caller's business)"
    assert opt(reduction="sum", per_image=True) == "cross_entropy: per_image sums the per-image weighted means: reduction must be 'mean'"
    assert opt(label_smoothing=1.0) == "cross_entropy: label_smoothing must be in [0, 1) (got 1.0)"
    assert opt(label_smoothing=-0.5) == "cross_entropy: label_smoothing must be in [0, 1) (got -0.5)"
    # where two checks fail, the first one of before still fires first
    assert opt(reduction="none", per_image=True, label_smoothing=2.0).startswith("cross_entropy: reduction must be")
    assert opt(weight=torch.ones(18)) == ("cross_entropy: weight must be a float32 tensor of shape [C] or [B, C] on cpu (C=19, B=2; got "
                                         "(torch.float32, (18,), device(type='cpu')))")
    assert opt(weight=[1.0]) == ("cross_entropy: weight must be a float32 tensor of shape [C] or [B, C] on cpu (C=19, B=2; got "
                                 "<class 'list'>)")
    assert ops._ce_options("w", torch.ones(2, 19), 0.1, "mean", True, 2, 19, cpu)[1:] == (19, 0.1, 2)
    assert ops._ce_options("w", torch.ones(19), 0, "sum", False, 2, 19, cpu)[1:] == (0, 0.0, 1)
    assert ops._ce_options("w", None, 0, "mean", False, 2, 19, cpu) == (None, 0, 0.0, 0)

    words = torch.zeros(2, 4, 3, dtype=torch.int32)
    relaxed = "upsample_soft_nll: the relaxed target must be int32 [B,H,W] words on cpu (ops.relax_labels / ops.pack_multihot)"
    assert _message(ops._soft_nll_options, "upsample_soft_nll", words.long(), None, 2, 4, 3, 19, cpu) == relaxed
    assert _message(ops._soft_nll_options, "upsample_soft_nll", words, None, 2, 3, 4, 19, cpu) == relaxed
    assert _message(ops._soft_nll_options, "soft_nll", words, None, 2, 4, 3, 32, cpu) == \
        "soft_nll: 1 <= num_classes <= 31: the classes and the ignore bit share one 32-bit word (got 32)"
    assert _message(ops._soft_nll_options, "soft_nll", words, torch.ones(3), 2, 4, 3, 19, cpu).startswith(
        "soft_nll: weight must be a float32 tensor of shape [C] or [B, C] on cpu (C=19, B=2; got (torch.float32, (3,)")
    assert _message(ops._relax_args, "relax_labels", 32, 1) == \
        "relax_labels: 1 <= num_classes <= 31: the classes and the ignore bit share one 32-bit word (got 32)"
    assert _message(ops._relax_args, "relax_labels", 0) == \
        "relax_labels: 1 <= num_classes <= 31: the classes and the ignore bit share one 32-bit word (got 0)"
    assert _message(ops._relax_args, "relax_labels", 19, 9) == "relax_labels: 0 <= border <= 8 (got 9)"
    assert ops._relax_args("relax_labels", 31, 8) == (31, 8)

    assert _message(ops._ohem_args, "ohem_target", 1.5, 10) == "ohem_target: thresh must be in [0, 1] (got 1.5)"
    assert _message(ops._ohem_args, "ohem_target", float("nan"), 10) == "ohem_target: thresh must be in [0, 1] (got nan)"
    assert _message(ops._ohem_args, "ohem_target", 0.7, -1) == "ohem_target: min_kept must not be negative (got -1)"
    assert _message(ops._ohem_args, "ohem_target", -0.1, -1) == "ohem_target: thresh must be in [0, 1] (got -0.1)"
    assert ops._ohem_args("ohem_target", 1, 0) == (1.0, 0)


def test_target_checks_verbatim(launches):
    """One helper checks the loss targets and the relaxation operands; each keeps its own text, and the public operators' `who`."""
    x, P, y, words, w = _operands()
    for fn, who in ((lambda t: ops.cross_entropy(x, t), "cross_entropy"), (lambda t: ops.upsample_cross_entropy(P, t, (H, W), C),
                    "upsample_cross_entropy"), (lambda t: ops.ohem_target(x, t), "ohem_target")):
        for bad in (y.int(), y[:, :-1], y[0]):
            assert _message(fn, bad) == "%s: target must be int64 [B,H,W]" % who
    assert _message(ops.soft_nll, x, words, C + 1) == "soft_nll: logits have 5 channels, num_classes is 6"
    assert _message(ops.upsample_soft_nll, P, y, (H, W), C).startswith("upsample_soft_nll: the relaxed target must be int32")
    assert _message(ops.relax_labels, y, 19) == "relax_labels: the target must be a GPU tensor: the HIP path has no CPU fallback"
    assert _message(ops.relaxed_counts, None, 19) == "relaxed_counts: the target must be a GPU tensor: the HIP path has no CPU fallback"
    assert not launches
