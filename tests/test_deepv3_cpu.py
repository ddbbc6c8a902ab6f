"""DeepLabV3+ baseline (mrfp_amd/network/deepv3.py, Mobilenet.py) and the depthwise / ReLU6 entry points: CPU checks.

The module trees against the reference's key / shape spec (tests/golden/deepv3_spec.json, written by
tests/golden/make_golden_deepv3.py from the reference itself), the CPU restatement against the reference's recorded numbers,
the C ABI declarations, and the refusal of grouped convolutions the kernels do not implement.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

import deepv3_common as dc

GOLD = np.load(dc.GOLDEN)


def _build(name):
    from mrfp_amd.network import deepv3
    with contextlib.redirect_stdout(io.StringIO()):
        return getattr(deepv3, name)(None, dc.NC, torch.nn.CrossEntropyLoss(ignore_index=255),
                                     torch.nn.CrossEntropyLoss(ignore_index=255))


@pytest.mark.parametrize("name", ["DeepMobileNetV3PlusD", "DeepMobileNetV3PlusD_OS8", "DeepR50V3PlusD"])
def test_state_dict_matches_reference_spec(name):
    m = _build(name)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == dc.spec(name)


def test_factories_and_trunk_guard():
    from mrfp_amd.network import deepv3
    for name in ("DeepR50V3PlusD_OS8", "DeepR101V3PlusD", "DeepR101V3PlusD_OS8"):
        m = _build(name)
        assert "layer4.0.conv2.weight" in m.state_dict()
    m = _build("DeepR101V3PlusD")
    assert "layer0.3.weight" in m.state_dict() and m.layer4[0].conv2.dilation == (2, 2)
    assert _build("DeepR50V3PlusD_OS8").layer3[0].conv2.dilation == (2, 2)
    os8 = _build("DeepMobileNetV3PlusD_OS8")
    assert os8.layer2[0].conv[1][0].dilation == (2, 2) and os8.layer3[3].conv[1][0].dilation == (4, 4)
    assert os8.layer2[0].conv[1][0].stride == (1, 1) and os8.layer1[0].conv[1][0].stride == (2, 2)
    with pytest.raises(ValueError, match="shufflenetv2"):
        with contextlib.redirect_stdout(io.StringIO()):
            deepv3.DeepV3Plus(19, trunk="shufflenetv2")


def test_dropin_import_path():
    from mrfp_amd.dropin.network import Mobilenet, deepv3
    assert deepv3.DeepMobileNetV3PlusD.__module__ == "mrfp_amd.network.deepv3"
    assert Mobilenet.mobilenet_v2.__module__ == "mrfp_amd.network.Mobilenet"


@pytest.mark.parametrize("name", list(dc.CASES))
def test_restatement_matches_reference_golden(name):
    trunk, variant = dc.CASES[name]
    sd, x, y, keep = dc.case_inputs(name)
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    work = {k: v.clone() for k, v in sd.items()}
    work.update(leaf)
    ns, taps = {}, {}
    l1, l2 = dc.deepv3_forward(work, x, trunk, variant, True, gts=y, drop_mask=keep, new_stats=ns, taps=taps)
    (l1 + l2).backward()
    p = name + "/"
    assert l1.item() == float(GOLD[p + "loss1"]) and l2.item() == float(GOLD[p + "loss2"])
    np.testing.assert_array_equal(taps["logits"][:, :4, 60:64, 60:64].detach().numpy(), GOLD[p + "train_logits_crop"])
    for f in GOLD.files:
        if f.startswith(p + "grad_l2/"):
            k = f[len(p + "grad_l2/"):]
            assert leaf[k].grad.double().pow(2).sum().sqrt().item() == float(GOLD[f]), k
        elif f.startswith(p + "running/"):
            np.testing.assert_array_equal(ns[f[len(p + "running/"):]][:8].numpy(), GOLD[f])


def test_header_declares_depthwise_entry_points():
    from mrfp_amd import _lib
    protos = _lib.parse_header()
    for name in ("mrfp_dwconv_nslab", "mrfp_dwconv_wgrad_ws_bytes", "mrfp_dwconv_fwd", "mrfp_dwconv_dgrad", "mrfp_dwconv_wgrad",
                 "mrfp_affine_fwd_relu6_mask", "mrfp_mask_gate"):
        assert name in protos, name
    assert len(protos["mrfp_dwconv_fwd"][1]) == 16 and len(protos["mrfp_dwconv_wgrad"][1]) == 15


def test_grouped_non_depthwise_conv_raises():
    from mrfp_amd import _lib, conv
    from mrfp_amd.network.mynn import HipConv2d
    m = HipConv2d(32, 64, 3, padding=1, groups=4, bias=False)
    with pytest.raises(_lib.MrfpHipError, match="groups=4"):
        m(torch.zeros(1, 32, 8, 8))
    m = HipConv2d(32, 32, 1, groups=32, bias=False)          # depthwise, but 1x1: not implemented either
    with pytest.raises(_lib.MrfpHipError, match="grouped"):
        m(torch.zeros(1, 32, 8, 8))
    w = torch.zeros(32, 1, 3, 3)                               # a depthwise weight handed to the dense path
    with pytest.raises(_lib.MrfpHipError, match="grouped"):
        conv.conv2d(torch.zeros(1, 32, 8, 8).contiguous(memory_format=torch.channels_last), w, None, 1, 1, 1)
