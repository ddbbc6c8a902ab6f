"""MobileNetV2 behind the reference's `network.Mobilenet` surface (reference network/Mobilenet.py: ConvBNReLU,
InvertedResidual, MobileNetV2, mobilenet_v2), executing on the HIP kernels of mrfp_amd/csrc.

Same module tree and state_dict keys as the reference (`features.N.conv.M.{0,1}`, `features.0.{0,1}`, `classifier.1`), so
reference checkpoints load unchanged.  The modules keep the reference's `[x, w_arr]` calling convention (DeepV3Plus passes
that list through its layer0..layer4 splits).  Depthwise 3x3 convolutions run on csrc/conv_dw.hip, the pointwise ones on the
MFMA implicit GEMM; every norm is a plain BatchNorm over this process's batch (the reference builds them as nn.BatchNorm2d,
never Norm2d: they are never synchronised across ranks), with ReLU6 folded into its apply pass.
"""
from __future__ import annotations

from typing import Any, Callable, List, Optional

import torch
from torch import nn

from .. import ops
from . import mynn
from .instance_whitening import InstanceWhitening

__all__ = ["MobileNetV2", "mobilenet_v2", "ConvBNReLU", "InvertedResidual"]

_CKPT_NAME = "mobilenet_v2-b0353104.pth"


def _make_divisible(v: float, divisor: int, min_value: Optional[int] = None) -> int:
    """Round a channel count to a multiple of `divisor`, never more than 10 % below v (the TF MobileNet rule)."""
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def _iw_layer(iw: int, channels: int):
    """The tap an `iw` code selects (reference Mobilenet.py ConvBNReLU / InvertedResidual __init__); an empty Sequential otherwise."""
    if iw in (1, 2):
        return InstanceWhitening(channels)
    if iw == 3:
        return mynn.HipInstanceNorm2d(channels, affine=False)
    if iw == 4:
        return mynn.HipInstanceNorm2d(channels, affine=True)
    return nn.Sequential()


def _apply_iw(layer, iw, x, w_arr):
    if iw in (1, 2):
        x, w = layer(x)
        w_arr.append(w)
    elif iw >= 1:
        x = layer(x)
    return x


def _unpack(x_tuple, what):
    if len(x_tuple) != 2:
        print("error in %s forward path" % what)          # reference Mobilenet.py prints and returns None
        return None, None
    return x_tuple[0], x_tuple[1]


class ConvBNReLU(nn.Sequential):
    """Sequential(conv, BatchNorm2d, ReLU6, iw tap) -- children 0..3 as the reference; the conv is depthwise when
    groups == in_planes == out_planes."""

    def __init__(self, in_planes: int, out_planes: int, kernel_size: int = 3, stride: int = 1, groups: int = 1,
                 norm_layer: Optional[Callable[..., nn.Module]] = None, iw: int = 0) -> None:
        padding = (kernel_size - 1) // 2
        if norm_layer is None:
            norm_layer = mynn.HipLocalBatchNorm2d
        self.iw = iw
        super().__init__(mynn.HipConv2d(in_planes, out_planes, kernel_size, stride, padding, groups=groups, bias=False),
                         norm_layer(out_planes), nn.ReLU6(inplace=True), _iw_layer(iw, out_planes))

    def forward(self, x_tuple):
        x, w_arr = _unpack(x_tuple, "BN")
        if x is None:
            return None
        x = mynn.conv_norm(self[0], self[1], x, act="relu6")
        return [_apply_iw(self[3], self.iw, x, w_arr), w_arr]


class InvertedResidual(nn.Module):
    """[1x1 expand ConvBNReLU] -> 3x3 depthwise ConvBNReLU -> 1x1 linear conv -> BatchNorm (+ skip when stride 1 and inp == oup)."""

    def __init__(self, inp: int, oup: int, stride: int, expand_ratio: int,
                 norm_layer: Optional[Callable[..., nn.Module]] = None, iw: int = 0) -> None:
        super().__init__()
        self.stride = stride
        assert stride in [1, 2]
        if norm_layer is None:
            norm_layer = mynn.HipLocalBatchNorm2d
        self.expand_ratio = expand_ratio
        self.iw = iw
        self.instance_norm_layer = _iw_layer(iw, oup)
        hidden_dim = int(round(inp * expand_ratio))
        self.use_res_connect = self.stride == 1 and inp == oup
        layers: List[nn.Module] = []
        if expand_ratio != 1:
            layers.append(ConvBNReLU(inp, hidden_dim, kernel_size=1, norm_layer=norm_layer))
        layers.extend([
            ConvBNReLU(hidden_dim, hidden_dim, stride=stride, groups=hidden_dim, norm_layer=norm_layer),
            mynn.HipConv2d(hidden_dim, oup, 1, 1, 0, bias=False),
            norm_layer(oup),
        ])
        self.conv = nn.Sequential(*layers)

    def forward(self, x_tuple):
        x, w_arr = _unpack(x_tuple, "invert residual")
        if x is None:
            return None
        t = [x, w_arr]
        n = len(self.conv)
        for i in range(n - 2):
            t = self.conv[i](t)
        conv_x, w_arr = t
        x = mynn.conv_norm(self.conv[n - 2], self.conv[n - 1], conv_x, post_add=x if self.use_res_connect else None)
        return [_apply_iw(self.instance_norm_layer, self.iw, x, w_arr), w_arr]


class MobileNetV2(nn.Module):
    """reference Mobilenet.py MobileNetV2: features[0] stem ConvBNReLU (stride 2), features[1..17] inverted residuals,
    features[18] 1x1 ConvBNReLU to last_channel; classifier Dropout(0.2) -> Linear."""

    def __init__(self, num_classes: int = 1000, width_mult: float = 1.0,
                 inverted_residual_setting: Optional[List[List[int]]] = None, round_nearest: int = 8,
                 block: Optional[Callable[..., nn.Module]] = None, norm_layer: Optional[Callable[..., nn.Module]] = None,
                 iw: list = [0, 0, 0, 0, 0, 0, 0]) -> None:
        super().__init__()
        if block is None:
            block = InvertedResidual
        if norm_layer is None:
            norm_layer = mynn.HipLocalBatchNorm2d
        input_channel = 32
        last_channel = 1280
        if inverted_residual_setting is None:
            inverted_residual_setting = [
                # t, c, n, s
                [1, 16, 1, 1],
                [6, 24, 2, 2],
                [6, 32, 3, 2],
                [6, 64, 4, 2],
                [6, 96, 3, 1],
                [6, 160, 3, 2],
                [6, 320, 1, 1],
            ]
        if len(inverted_residual_setting) == 0 or len(inverted_residual_setting[0]) != 4:
            raise ValueError("inverted_residual_setting should be non-empty "
                             "or a 4-element list, got {}".format(inverted_residual_setting))
        input_channel = _make_divisible(input_channel * width_mult, round_nearest)
        self.last_channel = _make_divisible(last_channel * max(1.0, width_mult), round_nearest)
        features: List[nn.Module] = [ConvBNReLU(3, input_channel, stride=2, norm_layer=norm_layer)]
        feature_count = 0
        iw_layer = [1, 6, 10, 17, 18]          # the features that carry an iw tap: iw[2..6] (reference Mobilenet.py)
        for t, c, n, s in inverted_residual_setting:
            output_channel = _make_divisible(c * width_mult, round_nearest)
            for i in range(n):
                feature_count += 1
                stride = s if i == 0 else 1
                code = iw[iw_layer.index(feature_count) + 2] if feature_count in iw_layer else 0
                features.append(block(input_channel, output_channel, stride, expand_ratio=t, norm_layer=norm_layer, iw=code))
                input_channel = output_channel
        features.append(ConvBNReLU(input_channel, self.last_channel, kernel_size=1, norm_layer=norm_layer))
        self.features = nn.Sequential(*features)
        self.classifier = nn.Sequential(nn.Dropout(0.2), nn.Linear(self.last_channel, num_classes))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.zeros_(m.bias)

    def _forward_impl(self, x):
        """Image classification: features -> global average pool -> Dropout -> Linear (the Linear as a 1x1 convolution of the
        pooled [B, last_channel, 1, 1] map)."""
        t = self.features([ops.as_activation(x), []])[0]
        t = ops.global_avg_pool(t)
        drop, fc = self.classifier[0], self.classifier[1]
        if self.training and drop.p > 0:
            B, C = t.shape[0], t.shape[1]
            keep = torch.bernoulli(torch.full((B, C), 1.0 - drop.p, device=t.device)) / (1.0 - drop.p)
            t = ops.channel_scale(t, keep)
        y = ops.conv2d(t, fc.weight.view(fc.out_features, fc.in_features, 1, 1), fc.bias, 1, 0, 1)
        return y.float().reshape(y.shape[0], -1)

    def forward(self, x):
        return self._forward_impl(x)


def mobilenet_v2(pretrained: bool = False, progress: bool = True, **kwargs: Any) -> MobileNetV2:
    """The reference downloads the ImageNet weights here.  There is no network in this build: a local checkpoint
    (cfg.MODEL.PRETRAINED_DIR or MRFP_PRETRAINED_DIR / mobilenet_v2-b0353104.pth) is restored when present, otherwise the
    initialiser's weights stay and a warning is printed."""
    import os
    from ..config import cfg
    model = MobileNetV2(**kwargs)
    if pretrained:
        d = cfg.MODEL.PRETRAINED_DIR or os.environ.get("MRFP_PRETRAINED_DIR")
        path = os.path.join(d, _CKPT_NAME) if d else None
        if path and os.path.exists(path):
            mynn.forgiving_state_restore(model, torch.load(path, map_location="cpu"))
        else:
            print("[mrfp_amd] no local %s checkpoint (set cfg.MODEL.PRETRAINED_DIR); keeping initialiser weights" % _CKPT_NAME)
    return model
