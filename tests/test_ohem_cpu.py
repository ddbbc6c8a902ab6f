"""No-GPU checks of the online-hard-example-mining cross entropy: exported symbols, host-side refusals (before any launch), the
workspace size, the criterion -> fused call mapping, and the test helper's selection rule against its restatement of the published
module."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
from torch import nn

import ohem_common as oc
from mrfp_amd import _lib, build

NEW = {"mrfp_ohem_ws_bytes": 2, "mrfp_select_kth": 6, "mrfp_ohem_target": 13, "mrfp_upsample_ohem_target": 17}


@pytest.fixture(scope="module")
def cdll():
    build.build()
    return _lib.lib()


def test_new_symbols_declared_and_exported(cdll):
    protos = _lib.parse_header()
    for name, nargs in NEW.items():
        assert name in protos and hasattr(cdll, name) and len(protos[name][1]) == nargs == len(_lib.ARG_NAMES[name]), name
    assert protos["mrfp_ohem_ws_bytes"][0] is ctypes.c_int64
    for name in ("mrfp_ohem_target", "mrfp_upsample_ohem_target"):
        args = dict(zip(_lib.ARG_NAMES[name], protos[name][1]))
        assert args["thresh"] is ctypes.c_float and args["min_kept"] is ctypes.c_int64 and args["ignore_index"] is ctypes.c_int64


def test_workspace_size(cdll):
    """The state and three histograms of at most 2^11 bins: the same few kilobytes at every size the entries take, -1 at one they refuse."""
    ws = cdll.mrfp_ohem_ws_bytes
    small = ws(2, 120)
    assert small == 4 * (16 + 3 * 2048) and ws(3, 419 * 419) == small and ws(16, 768 * 768) == small
    assert ws(1, 1 << 30) == -1 and ws(0, 120) == -1 and ws(2, 0) == -1 and ws(4, 1 << 29) == -1 and ws(65536, 4) == -1


def test_host_refusals_before_any_launch(cdll):
    """Every refusal fires on the host with the entry's own text (pointers into a host buffer: nothing is launched)."""
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255

    def dense(dtype=0, C=19, thresh=0.7, k=10, B=2, HW=16, x=p):
        return ("mrfp_ohem_target", (x, p, dtype, B, HW, C, 255, thresh, k, p, p, p, None))

    def up(dtype=0, C=19, thresh=0.7, k=10, B=2, H=4, W=4, x=p, ld=32):
        return ("mrfp_upsample_ohem_target", (x, ld, p, dtype, B, 2, 2, H, W, C, 255, thresh, k, p, p, p, None))

    cases = []
    for mk, who in ((dense, b"ohem_target"), (up, b"upsample_ohem_target")):
        cases += [
            (mk(x=None), who + b": null pointer"),
            (mk(dtype=99), who + b": unknown dtype 99"),
            (mk(C=0), who + b": 1 <= C <= 64 (C=0)"),
            (mk(C=65, **(dict(ld=72) if mk is up else {})), who + b": 1 <= C <= 64 (C=65)"),
            (mk(k=-1), who + b": min_kept must not be negative (min_kept=-1)"),
            (mk(thresh=float("nan")), who + b": thresh must be in [0, 1] (got nan)"),
            (mk(thresh=1.5), who + b": thresh must be in [0, 1] (got 1.5)"),
            (mk(thresh=-0.25), who + b": thresh must be in [0, 1] (got -0.25)"),
            (mk(B=0), who + b": 1 <= B <= 65535 and B*H*W below 2^31 (B=0)"),
            (mk(B=65536), who + b": 1 <= B <= 65535 and B*H*W below 2^31 (B=65536)"),
        ]
    cases += [
        (dense(HW=1 << 30), b"ohem_target: bad size (H*W=1073741824, below 2^30)"),
        (dense(B=4, HW=1 << 29), b"ohem_target: 1 <= B <= 65535 and B*H*W below 2^31 (B=4)"),
        (up(H=1 << 15, W=1 << 15), b"upsample_ohem_target: bad size (H*W=1073741824, below 2^30)"),
        (up(ld=19), b"upsample_ohem_target: the score buffer must be channel-padded to 16-byte chunks (ld=19)"),
        (up(x=p + 4), b"upsample_ohem_target: the score buffer must be channel-padded to 16-byte chunks (ld=32)"),
        (up(dtype=1, ld=20), b"upsample_ohem_target: the score buffer must be channel-padded to 16-byte chunks (ld=20)"),
        (("mrfp_select_kth", (None, 4, 1, p, p, None)), b"select_kth: null pointer"),
        (("mrfp_select_kth", (p, 0, 1, p, p, None)), b"select_kth: 1 <= n < 2^31 (n=0)"),
        (("mrfp_select_kth", (p, 4, 0, p, p, None)), b"select_kth: 1 <= k <= n (k=0 n=4)"),
        (("mrfp_select_kth", (p, 4, 5, p, p, None)), b"select_kth: 1 <= k <= n (k=5 n=4)"),
    ]
    for (name, args), text in cases:
        assert len(args) == len(_lib.ARG_NAMES[name]), name
        rc = getattr(cdll, name)(*args)
        assert rc == -1 and cdll.mrfp_last_error() == text, (name, rc, cdll.mrfp_last_error())


class _Foreign(nn.Module):
    def forward(self, x, y):
        return x.sum()


def test_criterion_mapping(monkeypatch):
    """OhemCrossEntropy2d enters through its own entry dict(ohem=<bound fused>), which fused_loss calls with (logits, gts, size,
    channels); the dictionaries of the criteria that existed before are what they were."""
    from mrfp_amd import loss, ops
    assert "OhemCrossEntropy2d" in loss.__all__
    w = torch.rand(19)
    crit = loss.OhemCrossEntropy2d(ignore_index=7, thresh=0.6, min_kept=300, weight=w)
    assert (crit.ignore_index, crit.thresh, crit.min_kept) == (7, 0.6, 300) and torch.equal(crit.weight, w)
    assert "weight" not in crit.state_dict()
    kw = loss.fused_ce_kwargs(crit)
    assert list(kw) == ["ohem"] and kw["ohem"].__self__ is crit and kw["ohem"].__func__ is loss.OhemCrossEntropy2d.fused
    d = loss.OhemCrossEntropy2d()
    assert (d.ignore_index, d.thresh, d.min_kept, d.weight) == (255, 0.7, 100000, None)
    calls = []
    monkeypatch.setattr(loss.ops, "ohem_cross_entropy", lambda *a, **k: calls.append(("dense", a, k)) or "L")
    monkeypatch.setattr(loss.ops, "upsample_ohem_cross_entropy", lambda *a, **k: calls.append(("up", a, k)) or "U")
    monkeypatch.setattr(loss.ops, "cross_entropy", lambda *a, **k: calls.append(("ce", a, k)) or "CE")
    monkeypatch.setattr(loss.ops, "upsample_cross_entropy", lambda *a, **k: calls.append(("upce", a, k)) or "UCE")
    assert loss.fused_loss(crit, "x", "labels") == "L" and loss.fused_loss(crit, "P", "labels", (8, 8), 19) == "U"
    assert crit("x", "labels") == "L"
    assert calls[0] == ("dense", ("x", "labels", 7), dict(thresh=0.6, min_kept=300, weight=crit.weight)) and calls[2] == calls[0]
    assert calls[1] == ("up", ("P", "labels", (8, 8), 19, 7), dict(thresh=0.6, min_kept=300, weight=crit.weight))
    # fused_loss hands the entry (logits, gts, size, channels)
    seen = []
    monkeypatch.setattr(loss, "fused_ce_kwargs", lambda c: dict(ohem=lambda *a: seen.append(a) or "O"))
    assert loss.fused_loss(crit, "P", "labels", (8, 8), 19) == "O" and seen == [("P", "labels", (8, 8), 19)]
    monkeypatch.undo()
    # the criteria that existed before
    assert loss.fused_ce_kwargs(nn.CrossEntropyLoss(ignore_index=255)) == dict(ignore_index=255, weight=None, label_smoothing=0.0,
                                                                              reduction="mean", per_image=False)
    assert loss.fused_ce_kwargs(nn.CrossEntropyLoss(reduction="none")) is None
    assert loss.fused_ce_kwargs(_Foreign()) is None and loss.fused_loss(_Foreign(), "x", "y") is None
    assert list(loss.fused_ce_kwargs(loss.ImgWtLossSoftNLL(19))) == ["soft_nll"]
    # no public keyword was added to the two cross-entropy operators; the new operators' signatures
    for f in (ops.cross_entropy, ops.upsample_cross_entropy):
        kws = {k for k, q in inspect.signature(f).parameters.items() if q.kind is q.KEYWORD_ONLY and not k.startswith("_")}
        assert kws == {"weight", "label_smoothing", "reduction", "per_image"}
    sig = inspect.signature(ops.ohem_target).parameters
    assert list(sig) == ["logits", "target", "ignore_index", "thresh", "min_kept", "size", "channels", "want_prob", "want_state"]
    assert [sig[k].default for k in ("ignore_index", "thresh", "min_kept")] == [255, 0.7, 100000]
    assert all(sig[k].kind is sig[k].KEYWORD_ONLY for k in ("size", "channels", "want_prob", "want_state"))
    for f, head in ((ops.ohem_cross_entropy, ["logits", "target", "ignore_index"]),
                    (ops.upsample_ohem_cross_entropy, ["P", "target", "size", "channels", "ignore_index"])):
        q = inspect.signature(f).parameters
        assert list(q)[:len(head)] == head
        assert {k: v.default for k, v in q.items() if v.kind is v.KEYWORD_ONLY} == dict(thresh=0.7, min_kept=100000, weight=None)
    for bad in (dict(thresh=1.5), dict(thresh=float("nan")), dict(min_kept=-1)):
        with pytest.raises(_lib.MrfpHipError):
            loss.OhemCrossEntropy2d(**bad)


@pytest.mark.parametrize("seed", range(5))
def test_rule_equals_the_published_masking(seed):
    """ohem_common.rule on p = softmax(z)[t] gives the masked target ohem_common.published_masked hands its cross entropy, at
    2 x 19 x 33 x 47 and min_kept in {0, 1, 300, N/2, N-1, N, N+1}; an all-ignored map gives an all-ignored target."""
    B, C, H, W = 2, 19, 33, 47
    y = oc.labels(B, H, W, C, 100 + seed, only_ignore=True)
    z = oc.logits(B, C, H, W, torch.float64, 200 + seed, y=y)
    p = oc.true_class_prob(z.permute(0, 2, 3, 1).numpy(), y.numpy(), C)
    # the published form reads its own soft-max: the same values, so that a tie or a threshold falls the same way
    sm = torch.softmax(z, 1).gather(1, torch.where(y == oc.IGNORE, 0, y)[:, None])[:, 0].numpy()
    N = int((y != oc.IGNORE).sum())
    assert 0 < N < B * H * W and np.allclose(sm[y.numpy() != oc.IGNORE], p[y.numpy() != oc.IGNORE], rtol=1e-12)
    modes = set()
    for min_kept in (0, 1, 300, N // 2, N - 1, N, N + 1):
        for thresh in (0.7, 0.05):
            masked, n, kept, theta, mode = oc.rule(sm, y.numpy(), C, thresh, min_kept)
            want = oc.published_masked(z, y, thresh, min_kept).numpy()
            assert n == N and np.array_equal(masked, want), (min_kept, thresh)
            assert kept == int((masked != oc.IGNORE).sum()) and (min_kept > N or kept >= min_kept)
            modes.add(mode)
    assert modes == {oc.KEEP_ALL, oc.THRESH, oc.KTH}
    dead = torch.full_like(y, oc.IGNORE)
    masked, n, kept, theta, mode = oc.rule(sm, dead.numpy(), C, 0.7, 10)
    assert (n, kept, mode) == (0, 0, oc.KEEP_ALL) and (masked == oc.IGNORE).all()
    assert (oc.published_masked(z, dead, 0.7, 10) == oc.IGNORE).all()


def test_rule_ties_and_nan():
    """Every tie at theta is kept (the kept count exceeds min_kept); a NaN p sorts last and is never kept below keep-all."""
    t = np.zeros(8, dtype=np.int64)
    p = np.array([0.9, 0.5, 0.5, 0.5, 0.5, 0.95, np.nan, 0.1], dtype=np.float32)
    masked, N, kept, theta, mode = oc.rule(p, t, 2, 0.2, 3)
    assert (N, kept, mode) == (8, 5, oc.KTH) and theta == np.float32(0.5) and oc.theta_bits(theta) == 0x3f000000
    assert masked.tolist() == [255, 0, 0, 0, 0, 255, 255, 0]
    masked, N, kept, theta, mode = oc.rule(p, t, 2, 0.2, 8)          # q is the NaN: the threshold stays
    assert (kept, mode) == (1, oc.THRESH) and theta == np.float32(0.2)
    masked, N, kept, theta, mode = oc.rule(p, t, 2, 0.2, 9)          # min_kept > N: every valid pixel, the NaN one included
    assert (kept, mode) == (8, oc.KEEP_ALL) and oc.theta_bits(theta) == 0x7f800000
