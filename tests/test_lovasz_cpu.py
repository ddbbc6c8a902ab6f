"""The Lovasz-Softmax loss, what needs no GPU: the float64 restatement the GPU tests hold the kernels to (lovasz_common) against the
set-function form and Berman's published form, its invariance under a permutation of tied pixels, the C header's new entries, the
argument refusals (raised before anything touches the library) and the routing of the module through loss.fused_ce_kwargs."""
import itertools

import numpy as np
import pytest
import torch
from torch import nn

import lovasz_common as lv
from mrfp_amd import _lib, loss, ops


def _errors(rng, labels, C):
    """Random soft-max rows for the pixels `labels`, and per class (e, fg)."""
    n = len(labels)
    p = lv.softmax64(rng.normal(size=(n, C, 1, 1)) * 2.0).reshape(n, C)
    lab = np.asarray(labels)
    return [(np.abs((lab == c).astype(np.float64) - p[:, c]), (lab == c).astype(np.float64)) for c in range(C)]


def test_restatement_equals_the_set_function_form_for_every_binary_label_pattern():
    """N <= 7, C = 2: every label pattern; the definition against sum_k e_(k) [J(S_k) - J(S_{k-1})] and against Berman's form."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for n in range(1, 8):
        for labels in itertools.product((0, 1), repeat=n):
            for e, fg in _errors(rng, labels, 2):
                got, g = lv.class_terms(e, fg)
                want = lv.set_function_class(e, fg)
                pub = lv.berman_class(e, fg)
                worst = max(worst, abs(got - want), abs(got - pub))
                assert abs(got - want) <= 1e-14 and abs(got - pub) <= 1e-14, (labels, got, want, pub)
                assert g.min() >= -1e-15                       # g_i >= 0
    print("largest difference between the three forms: %.3g" % worst)


@pytest.mark.parametrize("labels", [(0, 1, 2, 0, 1, 2, 0), (2, 2, 2, 2), (0, 0, 1, 1, 1), (1,), (0, 2, 0, 2, 2, 0)])
def test_restatement_equals_the_set_function_form_for_three_classes(labels):
    rng = np.random.default_rng(len(labels))
    for e, fg in _errors(rng, labels, 3):            # a class that does not occur (G = 0) included: its loss is the largest error
        got, g = lv.class_terms(e, fg)
        assert abs(got - lv.set_function_class(e, fg)) <= 1e-14 and abs(got - lv.berman_class(e, fg)) <= 1e-14
        if fg.sum() == 0:
            assert abs(got - e.max()) <= 1e-15 and g.sum() == 1.0


def test_loss_is_invariant_under_a_permutation_of_tied_pixels():
    """Errors drawn from three values, so most pixels are tied: any order of the tied pixels gives the same loss_c (the tie rule
    fixes the gradient, not the value)."""
    rng = np.random.default_rng(5)
    for trial in range(20):
        n = 12
        e = rng.choice([0.0, 0.25, 1.0], size=n)
        fg = (rng.random(n) < 0.4).astype(np.float64)
        base, _ = lv.class_terms(e, fg)
        for _ in range(10):
            # a random order that is still descending in e: shuffle, then a stable sort by e
            perm = rng.permutation(n)
            order = perm[np.argsort(-e[perm], kind="stable")]
            assert np.all(np.diff(e[order]) <= 0)
            got, _ = lv.class_terms(e, fg, order)
            assert abs(got - base) <= 1e-14, (trial, got, base)


def test_ref_lovasz_scopes_classes_and_empty_cases():
    x, y = lv.make_case(3, 4, 5, 6, torch.float32, 11)
    x, y = x.numpy(), y.numpy()
    # the batch scope is the mean over the present classes of the per-class terms
    p = lv.softmax64(x).transpose(0, 2, 3, 1).reshape(-1, 4)
    yf = y.reshape(-1)
    valid = (yf >= 0) & (yf < 4) & (yf != 255)
    terms = [lv.berman_class(np.abs((yf[valid] == c) - p[valid, c]), yf[valid] == c) for c in range(4)]
    present = [c for c in range(4) if (yf[valid] == c).any()]
    assert present == [0, 1, 2]                                                      # make_labels leaves class C - 1 out
    assert abs(lv.ref_lovasz(x, y) - np.mean([terms[c] for c in present])) <= 1e-14
    assert abs(lv.ref_lovasz(x, y, classes="all") - np.mean(terms)) <= 1e-14
    assert abs(terms[3] - p[valid, 3].max()) <= 1e-15                                # an absent class adds the largest p_c
    # per image: the mean over the images that have a counted class; an all-ignored image is left out, not averaged in as 0
    per = [lv.ref_lovasz(x[b:b + 1], y[b:b + 1]) for b in range(3)]
    assert abs(lv.ref_lovasz(x, y, per_image=True) - np.mean(per)) <= 1e-14
    half = y.copy()
    half[1] = 255
    assert abs(lv.ref_lovasz(x, half, per_image=True) - np.mean([per[0], per[2]])) <= 1e-14
    assert abs(lv.ref_lovasz(x, half, "all", per_image=True) - np.mean([lv.ref_lovasz(x[b:b + 1], y[b:b + 1], "all") for b in (0, 2)])) <= 1e-14
    # nothing valid
    blank = np.full_like(y, 255)
    for cl in ("present", "all"):
        l, g = lv.ref_lovasz(x, blank, cl, want_grad=True)
        assert l == 0.0 and np.abs(g).max() == 0.0


def test_ref_gradient_is_the_derivative_with_g_held_constant():
    """Central differences of sum_c sum_i e_i(z) g_i / K with g and the order frozen at z."""
    x, y = lv.make_case(2, 3, 3, 4, torch.float32, 12)
    x, y = x.numpy().astype(np.float64), y.numpy()
    l0, grad = lv.ref_lovasz(x, y, want_grad=True)
    p0 = lv.softmax64(x)
    yf = y.reshape(-1)
    valid = (yf >= 0) & (yf < 3) & (yf != 255)
    present = [c for c in range(3) if (yf[valid] == c).any()]
    gs = {}
    for c in present:
        fg = (yf[valid] == c).astype(np.float64)
        e = np.abs(fg - p0.transpose(0, 2, 3, 1).reshape(-1, 3)[valid, c])
        gs[c] = (fg, lv.class_terms(e, fg)[1])

    def frozen(z):
        p = lv.softmax64(z).transpose(0, 2, 3, 1).reshape(-1, 3)[valid]
        return sum((np.abs(fg - p[:, c]) * g).sum() for c, (fg, g) in gs.items()) / len(gs)
    assert abs(frozen(x) - l0) <= 1e-14
    rng = np.random.default_rng(1)
    for _ in range(12):
        i = tuple(rng.integers(0, s) for s in x.shape)
        d = np.zeros_like(x)
        d[i] = 1e-6
        num = (frozen(x + d) - frozen(x - d)) / 2e-6
        assert abs(num - grad[i]) <= 1e-8, (i, num, grad[i])


NEW_ENTRIES = ["mrfp_sort_tile_items", "mrfp_sort_scan_sweep", "mrfp_sort_pairs_ws_bytes", "mrfp_sort_pairs", "mrfp_lovasz_group_classes",
               "mrfp_lovasz_ws_bytes", "mrfp_lovasz_out_floats", "mrfp_lovasz_fwd", "mrfp_lovasz_bwd", "mrfp_upsample_lovasz_fwd",
               "mrfp_upsample_lovasz_bwd", "mrfp_lovasz_errors"]


def test_header_declares_the_new_entries():
    protos = _lib.parse_header()
    for n in NEW_ENTRIES:
        assert n in protos and len(protos[n][1]) == len(_lib.ARG_NAMES[n]), n
    names = _lib.ARG_NAMES
    # the argument lists of the region entries with the Lovasz options where those have theirs: one autograd function serves both
    swap = {"weight": None, "kind": None, "smooth": None, "present_only": "all_classes"}
    for pre in ("mrfp_", "mrfp_upsample_"):
        want = [swap.get(a, a) for a in names[pre + "region_fwd"] if swap.get(a, a) is not None]
        assert names[pre + "lovasz_fwd"] == want, (names[pre + "lovasz_fwd"], want)
        assert names[pre + "lovasz_bwd"] == names[pre + "region_bwd"]
    assert names["mrfp_sort_pairs"] == ["keys_in", "payload_in", "keys_out", "payload_out", "n", "offsets", "S", "bits", "ws", "stream"]
    assert ops.LOVASZ_CLASSES == {"present": 0, "all": 1} and ops.LOVASZ_SENTINEL == 2.0


def test_host_only_queries():
    from mrfp_amd import build
    build.build()
    L = _lib.lib()
    T = int(L.mrfp_sort_tile_items())
    assert T >= 256 and T % 64 == 0 and int(L.mrfp_sort_scan_sweep()) >= 64
    grp = int(L.mrfp_lovasz_group_classes())
    assert 1 <= grp <= 8
    # the sort workspace: the two alternate buffers plus the histograms; refused sizes are negative
    assert int(L.mrfp_sort_pairs_ws_bytes(1000, 1)) >= 8 * 1000 and int(L.mrfp_sort_pairs_ws_bytes(2 ** 31, 1)) < 0
    assert int(L.mrfp_sort_pairs_ws_bytes(10, 0)) < 0
    # the loss workspace is bounded by the group size, not by C: the same for 19 and 64 classes up to the per-class partials
    HW = 768 * 768
    w19, w64 = int(L.mrfp_lovasz_ws_bytes(16, HW, 19, 0)), int(L.mrfp_lovasz_ws_bytes(16, HW, 64, 0))
    per_pixel = w19 / (16 * HW)
    print("workspace at 16 x 768 x 768: %d bytes for 19 classes (%.2f per pixel), %d for 64" % (w19, per_pixel, w64))
    assert 16 * grp <= per_pixel < 16 * grp + 2 and w64 - w19 < 0.01 * w19
    assert int(L.mrfp_lovasz_ws_bytes(1, 2 ** 31, 19, 0)) < 0 and int(L.mrfp_lovasz_ws_bytes(2, 2 ** 30, 19, 0)) < 0
    assert int(L.mrfp_lovasz_ws_bytes(1, 100, 65, 0)) < 0
    assert int(L.mrfp_lovasz_out_floats(2, 100, 19, 1)) == 2 + 2 * 24 + 19 * 200
    # argument validation happens on the host before any launch
    assert L.mrfp_sort_pairs(None, None, None, None, 5, None, 1, 32, None, None) != 0 and b"sort_pairs: null pointer" in L.mrfp_last_error()
    assert L.mrfp_sort_pairs(None, None, None, None, 5, None, 1, 33, None, None) != 0 and b"bits" in L.mrfp_last_error()
    assert L.mrfp_sort_pairs(None, None, None, None, 5, None, 2, 32, None, None) != 0 and b"offsets" in L.mrfp_last_error()
    assert L.mrfp_lovasz_fwd(None, None, 0, 1, 4, 3, 255, 0, 0, None, None, None) != 0 and b"lovasz_fwd" in L.mrfp_last_error()


class _Foreign(nn.Module):
    def forward(self, x, y):
        return x.sum()


def test_routing_of_the_module(monkeypatch):
    assert "LovaszSoftmax2d" in loss.__all__
    lov = loss.LovaszSoftmax2d(classes="all", per_image=True, ignore_index=7)
    ce = nn.CrossEntropyLoss(ignore_index=7)
    both = loss.SumLoss((1.0, ce), (0.5, lov))
    assert list(loss.fused_ce_kwargs(lov)) == ["lovasz"] and loss.fused_ce_kwargs(lov)["lovasz"] == lov.fused
    assert list(loss.fused_ce_kwargs(both)) == ["sum"]
    assert not lov.state_dict() and not list(lov.parameters())
    # a sum that holds a foreign module still has no fused form
    s = loss.SumLoss((1.0, lov), (0.5, _Foreign()))
    assert loss.fused_ce_kwargs(s) is None and loss.fused_loss(s, "x", "y") is None and s.fused("x", "y") is None
    d = loss.LovaszSoftmax2d()
    assert (d.classes, d.per_image, d.ignore_index) == ("present", False, 255)

    seen = []

    def op(name, value):
        def f(*a, **k):
            seen.append((name, a, k))
            return value
        return f
    for name, value in (("lovasz_softmax", 5.0), ("upsample_lovasz_softmax", 7.0), ("cross_entropy", 11.0), ("upsample_cross_entropy", 13.0)):
        monkeypatch.setattr(ops, name, op(name, value))
    assert loss.fused_loss(lov, "x", "y") == 5.0 and loss.fused_loss(lov, "P", "y", (8, 8), 19) == 7.0 and lov("x", "y") == 5.0
    assert seen[0][:2] == ("lovasz_softmax", ("x", "y", 7)) and seen[1][:2] == ("upsample_lovasz_softmax", ("P", "y", (8, 8), 19, 7))
    assert seen[0][2] == seen[1][2] == dict(classes="all", per_image=True)
    del seen[:]
    assert loss.fused_loss(both, "x", "y") == 1.0 * 11.0 + 0.5 * 5.0 and both("x", "y") == 13.5
    assert loss.fused_loss(both, "P", "y", (8, 8), 19) == 1.0 * 13.0 + 0.5 * 7.0


def test_refusals_come_before_the_library(monkeypatch):
    def no_lib():
        raise AssertionError("an argument refusal touched the library")
    monkeypatch.setattr(_lib, "lib", no_lib)
    E = _lib.MrfpHipError
    x = torch.zeros(2, 5, 3, 4)
    y = torch.zeros(2, 3, 4, dtype=torch.int64)
    for bad in ("some", None, ["present"], 3):
        with pytest.raises(E, match="lovasz_softmax: classes must be 'present' or 'all'"):
            ops.lovasz_softmax(x, y, classes=bad)
        with pytest.raises(E, match="upsample_lovasz_softmax: classes must be 'present' or 'all'"):
            ops.upsample_lovasz_softmax(x, y, (6, 8), 5, classes=bad)
        with pytest.raises(E, match="LovaszSoftmax2d: classes must be 'present' or 'all'"):
            loss.LovaszSoftmax2d(classes=bad)
    # the region loss keeps refusing the name: the Lovasz loss is an operator of its own
    with pytest.raises(E, match="region_loss: kind"):
        ops.region_loss(x, y, kind="lovasz")
    # the operators' door: CPU tensors
    with pytest.raises(E, match="must live on the GPU"):
        ops.lovasz_softmax(x, y)
    with pytest.raises(E, match="must live on the GPU"):
        ops.upsample_lovasz_softmax(x, y, (6, 8), 5)
    with pytest.raises(E, match="must live on the GPU"):
        ops.lovasz_errors(x, y)
    # what depends on the tensors: the criterion record's check, on CPU tensors here
    crit = ops._Lovasz("lovasz_softmax", 255)
    src = ops._Scores(x)
    with pytest.raises(E, match="lovasz_softmax: target must be int64"):
        crit.check(src, y.int(), None)
    with pytest.raises(E, match="lovasz_softmax: target must be int64"):
        crit.check(src, y[:, :2], None)
    t, w = crit.check(src, y, None)
    assert t.dtype == torch.int64 and w is None
    with pytest.raises(E, match="lovasz_softmax: 1 <= C <= 64"):
        crit.check(ops._Scores(torch.zeros(1, 65, 2, 2)), torch.zeros(1, 2, 2, dtype=torch.int64), None)
    with pytest.raises(E, match="upsample_lovasz_softmax: 1 <= C <= 64"):
        ops._Lovasz("upsample_lovasz_softmax", 255).check(ops._Scores(torch.zeros(1, 72, 2, 2), (4, 4), 65),
                                                        torch.zeros(1, 4, 4, dtype=torch.int64), None)
    # the size limit, on tensors that own no memory
    big = ops._Scores(torch.zeros(2, 8, 2, 2, device="meta"), (32768, 32768), 5)
    with pytest.raises(E, match=r"upsample_lovasz_softmax: .* B \* H \* W < 2\^31"):
        ops._Lovasz("upsample_lovasz_softmax", 255).check(big, torch.zeros(1, device="meta"), None)
    ok = ops._Scores(torch.zeros(1, 8, 2, 2, device="meta"), (32768, 32768), 5)
    ops._lovasz_limits("lovasz_errors", ok)                            # 2^30 pixels: inside
    # sort_pairs
    k = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(E, match="sort_pairs: 1 <= bits <= 32"):
        ops.sort_pairs(k, k, bits=0)
    with pytest.raises(E, match="sort_pairs: 1 <= bits <= 32"):
        ops.sort_pairs(k, k, bits=33)
    with pytest.raises(E, match="sort_pairs: keys must be a GPU tensor"):
        ops.sort_pairs(k, k)
    km = torch.zeros(4, dtype=torch.int32, device="meta")

    class _OnGpu(torch.Tensor):          # a meta tensor that says it lives on the GPU: the checks behind the door, without a device
        is_cuda = True
    kg = km.as_subclass(_OnGpu)
    with pytest.raises(E, match="sort_pairs: keys must be a 1-dimensional int32 tensor"):
        ops.sort_pairs(torch.zeros(4, device="meta").as_subclass(_OnGpu), kg)
    with pytest.raises(E, match="sort_pairs: payload must be a 1-dimensional int32 tensor of 4 elements"):
        ops.sort_pairs(kg, torch.zeros(5, dtype=torch.int32, device="meta").as_subclass(_OnGpu))
    with pytest.raises(E, match="sort_pairs: offsets must be a 1-dimensional int64 GPU tensor"):
        ops.sort_pairs(kg, kg, offsets=torch.zeros(3, dtype=torch.int64))
