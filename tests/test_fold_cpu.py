"""Folded inference (mrfp_amd/inference.py), the parts that need no GPU: the C boundary of the new entry points, the set of
`conv -> BatchNorm` pairs each model folds, and the fold arithmetic itself restated in fp64."""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

from mrfp_amd import _lib


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


# ---- the header ----------------------------------------------------------------------------------------------------------
def test_header_declares_fold_entries():
    protos = _lib.parse_header()
    # mrfp_conv_fwd has 23 arguments: without colstats, plus act -> 23; mrfp_dwconv_fwd has 16: without ws, plus act -> 16
    assert len(protos["mrfp_conv_fwd"][1]) == 23
    assert len(protos["mrfp_conv_fwd_act"][1]) == 23
    assert len(protos["mrfp_dwconv_fwd"][1]) == 16
    assert len(protos["mrfp_dwconv_fwd_act"][1]) == 16
    assert len(protos["mrfp_pack_weight_folded"][1]) == 17
    assert len(protos["mrfp_pack_weights_folded_batched"][1]) == 6
    names = _lib.ARG_NAMES
    assert "colstats" not in names["mrfp_conv_fwd_act"] and names["mrfp_conv_fwd_act"][-2:] == ["act", "stream"]
    assert [a for a in names["mrfp_conv_fwd"] if a != "colstats"] == [a for a in names["mrfp_conv_fwd_act"] if a != "act"]
    assert "ws" not in names["mrfp_dwconv_fwd_act"] and names["mrfp_dwconv_fwd_act"][-2:] == ["act", "stream"]
    assert [a for a in names["mrfp_dwconv_fwd"] if a != "ws"] == [a for a in names["mrfp_dwconv_fwd_act"] if a != "act"]
    # the argument counts the header states in its comments are the ones it declares
    text = open(_lib.HEADER).read()
    for entry, n in (("mrfp_conv_fwd_act", 23), ("mrfp_dwconv_fwd_act", 16), ("mrfp_pack_weight_folded", 17),
                     ("mrfp_pack_weights_folded_batched", 6)):
        head = text[:text.index("int %s(" % entry)]
        comment = head[head.rindex("/*"):]
        assert "(%d arguments)" % n in comment, entry


def test_library_exports_fold_entries():
    L = _lib.lib()
    for entry in ("mrfp_conv_fwd_act", "mrfp_dwconv_fwd_act", "mrfp_pack_weight_folded", "mrfp_pack_weights_folded_batched"):
        assert hasattr(L, entry)


# ---- foldable_pairs ------------------------------------------------------------------------------------------------------
def _build(name):
    from mrfp_amd import deepv3
    from mrfp_amd.network import deepv3 as ndv3
    if name == "mrfp-r50":
        return _quiet(deepv3.MRFPPlus, 19, trunk="resnet-50")
    if name == "mrfp-r101":
        return _quiet(deepv3.MRFPPlus, 19, trunk="resnet-101")
    if name == "simple":
        return _quiet(deepv3.simpleDeepV3Plus, 19)
    if name == "mobilenet":
        return _quiet(ndv3.DeepMobileNetV3PlusD, None, 19, None, None)
    if name == "r50-d":
        return _quiet(ndv3.DeepR50V3PlusD, None, 19, None, None)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["mrfp-r50", "mrfp-r101", "simple", "mobilenet", "r50-d"])
def test_foldable_pairs_are_the_batchnorms_of_the_tree(name):
    from mrfp_amd import inference
    from mrfp_amd.network import Mobilenet, Resnet, mynn
    from mrfp_amd.network.instance_whitening import InstanceWhitening
    from mrfp_amd.network.sync_switchwhiten import SyncSwitchWhiten2d
    model = _build(name)
    names = {id(m): n for n, m in model.named_modules()}
    # expected: every HipBatchNorm2d / HipLocalBatchNorm2d of the tree, minus the eight HRFP norms, minus dsn.1
    hrfp = {id(bn) for _, bn in model.hrfp_layers()} if hasattr(model, "hrfp_layers") else set()
    assert len(hrfp) in (0, 8)
    expected = {n for n, m in model.named_modules()
                if isinstance(m, mynn.HipBatchNorm2d) and id(m) not in hrfp and n != "dsn.1"}
    pairs = inference.foldable_pairs(model)
    got = [names[id(nrm)] for _, nrm, _, _ in pairs]
    assert len(got) == len(set(got)), "a norm is listed twice"
    assert set(got) == expected
    parent = {}
    for n, m in model.named_modules():
        for cn, c in m.named_children():
            parent[id(c)] = m
    for conv, nrm, act, has_res in pairs:
        assert isinstance(conv, mynn.HipConv2d) and isinstance(nrm, mynn.HipBatchNorm2d)
        assert not isinstance(nrm, (mynn.HipInstanceNorm2d, InstanceWhitening, SyncSwitchWhiten2d))
        assert conv.out_channels == nrm.num_features
        assert act in (None, "relu", "relu6")
        owner = parent[id(nrm)]
        nname = names[id(nrm)]
        if isinstance(owner, Mobilenet.ConvBNReLU):
            assert (act, has_res) == ("relu6", False), nname
        elif isinstance(owner, torch.nn.Sequential) and isinstance(parent.get(id(owner)), Mobilenet.InvertedResidual):
            assert act is None and has_res == parent[id(owner)].use_res_connect, nname
        elif isinstance(owner, Resnet.Bottleneck):
            if nrm is owner.bn3:
                assert has_res and act == ("relu" if owner.iw < 1 else None), nname
            else:
                assert (act, has_res) == ("relu", False), nname
        elif isinstance(owner, torch.nn.Sequential) and isinstance(parent.get(id(owner)), Resnet._Block):
            assert (act, has_res) == (None, False), nname              # the downsample pair
        else:
            assert (act, has_res) == ("relu", False), nname              # stem, ASPP, bot_*, final1
    if name == "mrfp-r50":
        assert len(pairs) == 61          # the BatchNorms outside HRFP
        # layer1..layer3 end in an iw tap (wt_layer 4): their last block is folded without activation
        last = model.layer1[-1]
        assert [a for c, n, a, r in pairs if n is last.bn3] == [None]
    if name == "mobilenet":
        assert sum(1 for c, n, a, r in pairs if c.groups != 1) == 17      # one depthwise 3x3 per inverted residual


def test_wider_resnet_folds_its_head_only():
    from mrfp_amd import deepv3, inference
    model = _quiet(deepv3.MRFPPlus, 19, trunk="wider_resnet38_a2")
    names = {id(m): n for n, m in model.named_modules()}
    got = sorted(names[id(nrm)] for _, nrm, _, _ in inference.foldable_pairs(model))
    assert got, "the head folds"
    assert all(n.startswith(("aspp.", "bot_fine.", "bot_aspp.", "final1.")) for n in got), got
    assert len(got) == 9                 # 5 ASPP branches, bot_fine, bot_aspp, 2 x final1
    assert not any(n.startswith(("mod", "bn_out")) for n in got)


def test_fold_state_needs_eval_and_no_grad():
    from mrfp_amd import inference
    from mrfp_amd.network import mynn
    model = _build("simple")
    conv, nrm, _, _ = inference.foldable_pairs(model)[0]
    model.eval()
    with torch.no_grad():
        assert not mynn.fold_state(conv, nrm)                 # not enabled
    with inference.fold_norms(model) as h:
        assert h.enabled
        assert not mynn.fold_state(conv, nrm)                 # gradients enabled
        with torch.no_grad():
            assert mynn.fold_state(conv, nrm)
            model.train()
            assert not mynn.fold_state(conv, nrm)             # training mode
            model.eval()
    with torch.no_grad():
        assert not mynn.fold_state(conv, nrm)                 # the context switched it off again
    h = inference.fold_norms(model).enable()
    with torch.no_grad():
        assert mynn.fold_state(conv, nrm)
    h.disable()
    with torch.no_grad():
        assert not mynn.fold_state(conv, nrm)
    # a BatchNorm without running statistics is never folded
    nrm2 = mynn.HipBatchNorm2d(conv.out_channels, track_running_stats=False)
    assert not inference._foldable(conv, nrm2)


# ---- the arithmetic ------------------------------------------------------------------------------------------------------
def _fold64(w, cb, gamma, beta, mean, var, eps):
    A = gamma / torch.sqrt(var + eps)
    S = beta - mean * A
    if cb is not None:
        S = S + A * cb
    return w * A.view(-1, 1, 1, 1), S


@pytest.mark.parametrize("case", ["dense", "depthwise", "conv_bias", "tiny_var"])
def test_fold_arithmetic_fp64(case):
    g = torch.Generator().manual_seed({"dense": 1, "depthwise": 2, "conv_bias": 3, "tiny_var": 4}[case])
    dt = torch.float64
    C, N, groups = (12, 12, 12) if case == "depthwise" else (10, 14, 1)
    x = torch.randn(2, C, 9, 11, generator=g, dtype=dt)
    w = torch.randn(N, C // groups, 3, 3, generator=g, dtype=dt)
    cb = torch.randn(N, generator=g, dtype=dt) if case == "conv_bias" else None
    gamma, beta = torch.randn(N, generator=g, dtype=dt), torch.randn(N, generator=g, dtype=dt)
    mean = torch.randn(N, generator=g, dtype=dt)
    var = torch.rand(N, generator=g, dtype=dt) + 0.1
    if case == "tiny_var":
        var[::2] = torch.tensor([0.0, 1e-12, 1e-9, 1e-7, 1e-6, 0.0, 1e-10], dtype=dt)
    eps = 1e-5
    ref = F.batch_norm(F.conv2d(x, w, cb, padding=1, groups=groups), mean, var, gamma, beta, training=False, eps=eps)
    wf, S = _fold64(w, cb, gamma, beta, mean, var, eps)
    got = F.conv2d(x, wf, S, padding=1, groups=groups)
    rel = ((got - ref).abs().max() / ref.abs().max()).item()
    assert rel <= 1e-12, rel
