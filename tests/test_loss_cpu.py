"""No-GPU checks of the weighted / label-smoothed / per-image cross entropy: exported symbols, host-side refusals (before any
launch), the criterion -> keyword-argument mapping of the models, and the float64 restatement the GPU tests compare against."""
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import loss_common as lc
from mrfp_amd import _lib, build

NEW = ("mrfp_ce_w_nblocks", "mrfp_ce_w_loss_floats", "mrfp_ce_w_fwd", "mrfp_ce_w_bwd", "mrfp_upsample_ce_w_fwd",
       "mrfp_upsample_ce_w_bwd", "mrfp_label_class_weights")


@pytest.fixture(scope="module")
def cdll():
    build.build()
    return _lib.lib()


def test_new_symbols_declared_and_exported(cdll):
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos and hasattr(cdll, name), name
    # the smoothing is a float and the upper bound a double at the boundary
    assert ctypes.c_float in protos["mrfp_ce_w_fwd"][1] and ctypes.c_double in protos["mrfp_label_class_weights"][1]


def test_workspace_and_loss_sizes(cdll):
    """A workgroup stays inside one image: nbx workgroups per image, nbx * B <= 2048 (the project's cap) while B <= 2048."""
    nb, lf = cdll.mrfp_ce_w_nblocks, cdll.mrfp_ce_w_loss_floats
    assert nb(2, 120) == 2 and nb(1, 63) == 1 and nb(3, 257) == 6
    assert nb(3, 419 * 419) == (2048 // 3) * 3 and nb(16, 768 * 768) == 2048 and nb(5, 1 << 30) == 2045
    assert nb(4096, 100) == 4096
    assert lf(16, 0) == 2 and lf(16, 1) == 2 and lf(16, 2) == 17 and lf(1, 2) == 2


def test_host_refusals_before_any_launch(cdll):
    """Every refusal fires on the host with the entry's own text (pointers into a host buffer: nothing is launched)."""
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    E = 0.1

    def dense_f(dtype=0, C=19, ws=0, eps=E, mode=0):
        return ("mrfp_ce_w_fwd", (p, p, dtype, 2, 16, C, 255, p, ws, eps, mode, p, p, None))

    def dense_b(dtype=0, C=19, ws=0, eps=E, mode=0):
        return ("mrfp_ce_w_bwd", (p, p, p, p, p, dtype, 2, 16, C, 255, p, ws, eps, mode, None))

    def up_f(dtype=0, C=19, ws=0, eps=E, mode=0, ld=32, P=p):
        return ("mrfp_upsample_ce_w_fwd", (P, ld, p, dtype, 2, 2, 2, 4, 4, C, 255, p, ws, eps, mode, p, p, None))

    def up_b(dtype=0, C=19, ws=0, eps=E, mode=0, ld=32, Cd=20):
        return ("mrfp_upsample_ce_w_bwd", (p, ld, p, p, p, p, Cd, dtype, 2, 2, 2, 4, 4, C, 255, p, ws, eps, mode, None))

    cases = []
    for mk, who in ((dense_f, b"ce_w_fwd"), (dense_b, b"ce_w_bwd"), (up_f, b"upsample_ce_w_fwd"), (up_b, b"upsample_ce_w_bwd")):
        cases += [
            (mk(dtype=99), who + b": unknown dtype 99"),
            (mk(ws=7), who + b": wstride must be 0 (one weight row) or C (one per image) (wstride=7 C=19)"),
            (mk(eps=1.0), who + b": label smoothing must be in [0, 1) (got 1)"),
            (mk(eps=-0.5), who + b": label smoothing must be in [0, 1) (got -0.5)"),
            (mk(mode=3), who + b": unknown mode 3"),
        ]
    cases += [
        (up_f(C=65, ld=72), b"upsample_ce_w_fwd: 1 <= C <= 64 (C=65)"),
        (up_b(C=65, ld=72, Cd=68), b"upsample_ce_w_bwd: 1 <= C <= 64 (C=65)"),
        (up_f(ld=19), b"upsample_ce_w_fwd: the score buffer must be channel-padded to 16-byte chunks (ld=19)"),
        (up_f(P=p + 4), b"upsample_ce_w_fwd: the score buffer must be channel-padded to 16-byte chunks (ld=32)"),
        (up_f(dtype=1, ld=20), b"upsample_ce_w_fwd: the score buffer must be channel-padded to 16-byte chunks (ld=20)"),
        (up_b(Cd=19), b"upsample_ce_w_bwd: channel pitches must be 16-byte multiples (ld=32 Cd=19)"),
        (up_b(ld=16, Cd=20), b"upsample_ce_w_bwd: channel pitches must be 16-byte multiples (ld=16 Cd=20)"),
    ]
    for (name, args), text in cases:
        assert len(args) == len(_lib.ARG_NAMES[name]), name
        rc = getattr(cdll, name)(*args)
        assert rc == -1 and cdll.mrfp_last_error() == text, (name, rc, cdll.mrfp_last_error())
    # valid wstride == C passes that check (the next refusal is the mode's)
    name, args = dense_f(ws=19, mode=9)
    assert getattr(cdll, name)(*args) == -1 and cdll.mrfp_last_error() == b"ce_w_fwd: unknown mode 9"
    assert cdll.mrfp_label_class_weights(None, 1, 1, 19, 1.0, 0, 0, None, None, None) == -1
    assert cdll.mrfp_last_error().startswith(b"label_class_weights: bad arguments")
    assert cdll.mrfp_label_class_weights(p, 1, 16, 2000, 1.0, 0, 0, p, p, None) == -1


class _Foreign(nn.Module):
    def forward(self, x, y):
        return x.sum()


def test_criterion_mapping(monkeypatch):
    """One helper maps a criterion to the fused call's keyword arguments, or to None for what stays on the stock call."""
    from mrfp_amd import deepv3, loss
    from mrfp_amd.network import deepv3 as ndeepv3
    plain = loss.fused_ce_kwargs(nn.CrossEntropyLoss(ignore_index=255))
    assert plain == dict(ignore_index=255, weight=None, label_smoothing=0.0, reduction="mean", per_image=False)
    w = torch.rand(19)
    c = nn.CrossEntropyLoss(weight=w, ignore_index=7, label_smoothing=0.1, reduction="sum")
    kw = loss.fused_ce_kwargs(c)
    assert kw["weight"] is c.weight and torch.equal(kw["weight"], w)
    assert {k: v for k, v in kw.items() if k != "weight"} == dict(ignore_index=7, label_smoothing=0.1, reduction="sum", per_image=False)
    ib = loss.ImageBasedCrossEntropyLoss2d(19, norm=True, upper_bound=2.0)
    kw = loss.fused_ce_kwargs(ib)
    assert callable(kw["weight"]) and kw["weight"].__self__ is ib
    assert {k: v for k, v in kw.items() if k != "weight"} == dict(ignore_index=255, label_smoothing=0.0, reduction="mean", per_image=True)
    assert (ib.num_classes, ib.norm, ib.upper_bound, ib.batch_weights) == (19, True, 2.0, False)
    assert loss.fused_ce_kwargs(nn.CrossEntropyLoss(reduction="none")) is None
    assert loss.fused_ce_kwargs(_Foreign()) is None and loss.fused_ce_kwargs(None) is None
    # fused_loss: None for what stays on the stock call; a tensor weight passes through, the per-image criterion's is computed
    # from the label map; with `size` the upsample form is called (the operators are replaced: nothing runs on a device here)
    assert loss.fused_loss(_Foreign(), "x", "labels") is None and loss.fused_loss(nn.CrossEntropyLoss(reduction="none"), "x", "y") is None
    calls = []
    monkeypatch.setattr(loss.ops, "cross_entropy", lambda *a, **k: calls.append(("dense", a, k)) or "L")
    monkeypatch.setattr(loss.ops, "upsample_cross_entropy", lambda *a, **k: calls.append(("up", a, k)) or "U")
    monkeypatch.setattr(loss.ops, "label_class_weights", lambda *a: calls.append(("weights", a)) or ["W"])
    assert loss.fused_loss(c, "x", "labels") == "L" and loss.fused_loss(ib, "P", "labels", (8, 8), 19) == "U"
    assert calls[0] == ("dense", ("x", "labels", 7), dict(weight=c.weight, label_smoothing=0.1, reduction="sum", per_image=False))
    assert calls[1] == ("weights", ("labels", 19, 2.0, True, False))
    assert calls[2] == ("up", ("P", "labels", (8, 8), 19, 255), dict(weight=["W"], label_smoothing=0.0, reduction="mean", per_image=True))
    with pytest.raises(ValueError):
        loss.ImageBasedCrossEntropyLoss2d(19, weight=torch.ones(19))
    # both model families go through the one helper; the condition is not written out a second time
    assert ndeepv3.fused_loss is loss.fused_loss and deepv3.fused_loss is loss.fused_loss and not hasattr(deepv3._DeepLabBase, "_plain_ce")


def test_operator_keywords():
    import inspect
    from mrfp_amd import ops
    for f in (ops.cross_entropy, ops.upsample_cross_entropy):
        kw = {k: p.default for k, p in inspect.signature(f).parameters.items() if p.kind is p.KEYWORD_ONLY and not k.startswith("_")}
        assert kw == dict(weight=None, label_smoothing=0.0, reduction="mean", per_image=False)
    assert list(inspect.signature(ops.cross_entropy).parameters)[:3] == ["logits", "target", "ignore_index"]
    assert list(inspect.signature(ops.upsample_cross_entropy).parameters)[:5] == ["P", "target", "size", "channels", "ignore_index"]


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_per_image_reference_is_torchs_weighted_mean_for_one_image(eps):
    """The float64 restatement the GPU tests use (loss_common.ref_loss), forced through its per-image loop, against torch's own
    F.cross_entropy(weight=, label_smoothing=, ignore_index=) at B = 1: `mean` and `image_mean` are torch's weighted mean, `sum` its
    sum; with B = 2 and shared weights `mean` and `sum` still are, and `image_mean` is the sum of the two single-image means."""
    g = torch.Generator().manual_seed(5)
    C = 19
    w = lc.make_weights(C, g).double()
    for B in (1, 2):
        x = (torch.randn(B, C, 7, 9, generator=g) * 3).double()
        y = lc.mask_invalid(lc.make_labels(B, C, 7, 9, g), C)
        rows = w.expand(B, C).contiguous()          # [B,C]: takes the loop
        for mode in ("mean", "sum"):
            want = F.cross_entropy(x, y, weight=w, ignore_index=255, reduction=mode, label_smoothing=eps)
            got = lc.ref_loss(x, y, rows, eps, mode)
            assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item()), (B, mode)
        per = sum(F.cross_entropy(x[b:b + 1], y[b:b + 1], weight=w, ignore_index=255, label_smoothing=eps) for b in range(B))
        for ww in (w, rows):
            got = lc.ref_loss(x, y, ww, eps, "image_mean")
            assert abs(got.item() - per.item()) <= 1e-12 * abs(per.item()), B
    # numpy restatement of the per-image weight rule: absent classes and an all-255 map give weight 1
    t = torch.full((2, 3, 3), 255)
    t[0, 0] = torch.tensor([0, 0, 2])
    wts = lc.np_class_weights(t.numpy(), 4, 1.0, False, False)
    import numpy as np
    assert wts.dtype == np.float32
    np.testing.assert_array_equal(wts, np.array([[1 + (1 - 2 / 3), 1.0, 1 + (1 - 1 / 3), 1.0], [1.0] * 4]).astype(np.float32))
    assert lc.np_class_weights(t.numpy(), 4, 1.0, True, True).tolist() == [[2.5, 1.0, 4.0, 1.0]]
