"""Criteria beyond the plain nn.CrossEntropyLoss(ignore_index=255) of main.py:822, for the `criterion` / `criterion_aux` arguments
the reference's DeepV3Plus takes from its caller (network/deepv3.py:111), and the one mapping from a criterion to the keyword
arguments of the fused loss operators (ops.cross_entropy / ops.upsample_cross_entropy; kernels in csrc/loss.hip).

ImageBasedCrossEntropyLoss2d is the per-image class-weighted loss the DeepLabV3+ baseline that network/deepv3.py derives from was
trained with.  Its source is not in the reference tree: the rule stated in ops.label_class_weights is the definition here
(build-defined).  The published form copies the label map to the host every step for np.histogram; here the
histogram, the weights and the loss stay on the device, with no synchronisation.
"""
from __future__ import annotations

from torch import nn

from . import ops

__all__ = ["ImageBasedCrossEntropyLoss2d", "fused_ce_kwargs", "fused_loss"]


class ImageBasedCrossEntropyLoss2d(nn.Module):
    """sum over the images of the batch of NLLLoss(weight = w(image))(log_softmax(inputs[i]), targets[i]), w from the image's own label
    histogram (batch_weights: from the whole batch's, one row for all images)."""

    def __init__(self, classes, weight=None, ignore_index=255, norm=False, upper_bound=1.0, batch_weights=False):
        super().__init__()
        if weight is not None:
            raise ValueError("ImageBasedCrossEntropyLoss2d computes its class weights from the labels on every call (the original "
                             "overwrites a fixed weight): weight must be None")
        self.num_classes = int(classes)
        self.ignore_index = int(ignore_index)
        self.norm = bool(norm)
        self.upper_bound = float(upper_bound)
        self.batch_weights = bool(batch_weights)

    def class_weights(self, targets):
        """float32 [B, C] on the device, or [C] with batch_weights."""
        w = ops.label_class_weights(targets, self.num_classes, self.upper_bound, self.norm, self.batch_weights)
        return w[0] if self.batch_weights else w

    def forward(self, inputs, targets):
        return ops.cross_entropy(inputs, targets, self.ignore_index, weight=self.class_weights(targets), per_image=True)


def fused_ce_kwargs(criterion):
    """The keyword arguments with which ops.cross_entropy / ops.upsample_cross_entropy compute `criterion`, or None for a criterion
    they cannot (reduction='none', a foreign module): that one keeps the stock call on the full-resolution fp32 logits.  `weight` is
    a tensor, None, or -- for the per-image criterion -- a callable of the label map (fused_loss calls it)."""
    c = criterion
    if isinstance(c, ImageBasedCrossEntropyLoss2d):
        return dict(ignore_index=c.ignore_index, weight=c.class_weights, label_smoothing=0.0, reduction="mean", per_image=True)
    if isinstance(c, nn.CrossEntropyLoss) and c.reduction in ("mean", "sum"):
        return dict(ignore_index=c.ignore_index, weight=c.weight, label_smoothing=float(c.label_smoothing), reduction=c.reduction,
                    per_image=False)
    return None


def fused_loss(criterion, logits, gts, size=None, channels=None):
    """`criterion` on the fused loss kernels, or None for a criterion they do not compute (fused_ce_kwargs).  With `size`, `logits`
    are the channel-padded low-resolution class scores and the bilinear upsample to `size` is part of the loss kernel."""
    kw = fused_ce_kwargs(criterion)
    if kw is None:
        return None
    ignore = kw.pop("ignore_index")
    if callable(kw["weight"]):
        kw["weight"] = kw["weight"](gts)
    if size is not None:
        return ops.upsample_cross_entropy(logits, gts, size, channels, ignore, **kw)
    return ops.cross_entropy(logits, gts, ignore, **kw)
