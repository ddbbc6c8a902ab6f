"""Folded inference: in `eval()` every BatchNorm with running statistics is a fixed per-channel affine, so
`conv -> BatchNorm (-> ReLU | ReLU6) (-> + residual)` runs as ONE convolution launch -- the forward pack is the fp32 master scaled
by A[n] = gamma / sqrt(var + eps) and rounded once, S[n] = beta - mean * A (+ A * conv bias) is the launch's bias, the activation
and the residual add are the kernel's epilogue (mrfp_conv_fwd_act, mrfp_dwconv_fwd_act; packs: mrfp_pack_weight_folded).  The
`mrfp_bn_eval_coef` launch and the affine apply pass over the activation disappear.

    with fold_norms(model):
        logits = model(x, training=False)          # under torch.no_grad(), model in eval()

    handle = fold_norms(model).enable()            # ... or switched on and off by hand
    handle.disable()

The mode is opt-in and per model.  A pair runs folded only while the mode is enabled, its modules are in `eval()` and
`torch.is_grad_enabled()` is false (network.mynn.fold_state); in every other state the ordinary two calls run, bit for bit -- a
model left with the fold enabled trains exactly like one that never had it.  With the fold enabled `MRFPPlus` also skips its HRFP
branch at `training=False`: nothing reads its outputs there, and in `eval()` its BatchNorms update no running statistics.

Folded (foldable_pairs): `deepv3._ConvBnRelu` (ASPP, bot_fine, bot_aspp), `final1`, the Bottleneck / BasicBlock pairs of the ResNet
trunks (bn3 / bn2 with the residual as the epilogue's addend; with an `iw` tap behind the block the pair is folded without
activation and the tap runs as it does unfolded), the downsample pair, the stem pairs whose norm is a BatchNorm,
`Mobilenet.ConvBNReLU` (ReLU6, dense and depthwise) and the linear tail of `Mobilenet.InvertedResidual` (block input as addend).

NOT folded, by construction -- each keeps its current path:
  * InstanceNorm (`HipInstanceNorm2d`): per-image statistics, nothing fixed to fold;
  * `InstanceWhitening` / `SyncSwitchWhiten2d`;
  * WiderResNet's pre-activation blocks: their norm precedes a ReLU that precedes the convolution (and `bn_out` follows a
    residual add): there is no convolution in front of the norm to fold into;
  * a BatchNorm with `track_running_stats=False` (it normalises with batch statistics in eval() too);
  * the eight HRFP BatchNorms (they sit behind a nearest resize and always use batch statistics in the reference's forward);
  * the train-only `dsn` head of `network.deepv3.DeepV3Plus`.

Folded packs hang on the pack cache of mrfp_amd/conv.py and are rebuilt -- one batched launch for the whole model -- whenever a
weight or one of the four BatchNorm tensors changed (optimizer step, load_state_dict, conv.invalidate_packs(), any training-mode
BatchNorm forward); see conv.get_folded_pack.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

from torch import nn

from . import conv as conv_mod
from .network import mynn

__all__ = ["fold_norms", "foldable_pairs"]


def _foldable(conv, norm) -> bool:
    return (isinstance(conv, mynn.HipConv2d) and isinstance(norm, mynn.HipBatchNorm2d) and norm.track_running_stats
            and norm.running_mean is not None and norm.running_var is not None)


def _resnet_stem(trunk, layer0) -> List[Tuple[nn.Module, nn.Module, Optional[str], bool]]:
    """(conv, norm) of a ResNet stem as `layer0` holds them: conv, norm, relu (x3 for the deep stem), max pool."""
    from .network import Resnet
    n = 3 if isinstance(trunk, Resnet.ResNet3X3) else 1
    return [(layer0[3 * i], layer0[3 * i + 1], "relu", False) for i in range(n)]


def foldable_pairs(model: nn.Module):
    """[(conv, norm, act, has_residual)] of the `conv -> BatchNorm` call sites fold_norms(model) folds, in module order.
    act: None, 'relu' or 'relu6' -- the activation that moves into the convolution's epilogue; has_residual: whether the epilogue
    also adds the block's skip connection."""
    from . import deepv3
    from .network import Mobilenet, Resnet
    out = []
    for m in model.modules():
        cand = []
        if isinstance(m, deepv3._ConvBnRelu):
            cand.append((m[0], m[1], "relu", False))
        if isinstance(m, deepv3._DeepLabBase):
            f1 = getattr(m, "final1", None)
            if f1 is not None:
                cand += [(f1[0], f1[1], "relu", False), (f1[3], f1[4], "relu", False)]
            trunk = m._trunk[0] if getattr(m, "_trunk", None) else None
            if isinstance(trunk, (Resnet.ResNet, Resnet.ResNet3X3)) and isinstance(getattr(m, "layer0", None), nn.Sequential):
                cand += _resnet_stem(trunk, m.layer0)
        if isinstance(m, Resnet.ResNet3X3):
            cand += [(m.conv1, m.bn1, "relu", False), (m.conv2, m.bn2, "relu", False), (m.conv3, m.bn3, "relu", False)]
        elif isinstance(m, Resnet.ResNet):
            cand.append((m.conv1, m.bn1, "relu", False))
        if isinstance(m, Resnet._Block):
            tail_act = "relu" if m.iw < 1 else None          # an iw tap behind the block runs its own norm + ReLU
            if isinstance(m, Resnet.Bottleneck):
                cand += [(m.conv1, m.bn1, "relu", False), (m.conv2, m.bn2, "relu", False), (m.conv3, m.bn3, tail_act, True)]
            else:
                cand += [(m.conv1, m.bn1, "relu", False), (m.conv2, m.bn2, tail_act, True)]
            if m.downsample is not None:
                cand.append((m.downsample[0], m.downsample[1], None, False))
        if isinstance(m, Mobilenet.ConvBNReLU):
            cand.append((m[0], m[1], "relu6", False))
        if isinstance(m, Mobilenet.InvertedResidual):
            n = len(m.conv)
            cand.append((m.conv[n - 2], m.conv[n - 1], None, bool(m.use_res_connect)))
        for c, nrm, act, res in cand:
            if _foldable(c, nrm) and not any(nrm is p[1] for p in out):
                out.append((c, nrm, act, res))
    return out


class _FoldSet(list):
    """[(conv, norm)] of one model (a list that can be weakly referenced: conv.register_fold_set)"""


class fold_norms:
    """Context manager / handle that switches the folded inference mode of `model` on and off (module docstring)."""

    def __init__(self, model: nn.Module):
        self.model = model
        self._mine = False

    def enable(self):
        if getattr(self.model, "_mrfp_fold_set", None) is not None:
            return self                              # already on (an outer context owns it)
        pairs = foldable_pairs(self.model)
        from . import deepv3
        for _, nrm, _, _ in pairs:
            nrm._mrfp_fold = True
        for m in self.model.modules():
            if isinstance(m, deepv3.MRFPPlus):
                m._mrfp_fold = True                  # HRFP is not run at training=False
        fs = _FoldSet((c, n) for c, n, _, _ in pairs)
        object.__setattr__(self.model, "_mrfp_fold_set", fs)
        conv_mod.register_fold_set(fs)
        self._mine = True
        return self

    def disable(self):
        fs = getattr(self.model, "_mrfp_fold_set", None)
        if fs is None:
            return self
        for _, nrm in fs:
            if hasattr(nrm, "_mrfp_fold"):
                del nrm._mrfp_fold
        for m in self.model.modules():
            if "_mrfp_fold" in m.__dict__:
                del m.__dict__["_mrfp_fold"]
        object.__delattr__(self.model, "_mrfp_fold_set")
        self._mine = False
        return self

    @property
    def enabled(self) -> bool:
        return getattr(self.model, "_mrfp_fold_set", None) is not None

    def __enter__(self):
        was_on = self.enabled
        self.enable()
        self._mine = not was_on
        return self

    def __exit__(self, *exc):
        if self._mine:
            self.disable()
        return False
