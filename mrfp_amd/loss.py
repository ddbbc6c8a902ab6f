"""Criteria beyond the plain nn.CrossEntropyLoss(ignore_index=255) of main.py:822, for the `criterion` / `criterion_aux` arguments
the reference's DeepV3Plus takes from its caller (network/deepv3.py:111), and the one mapping from a criterion to the keyword
arguments of the fused loss operators (ops.cross_entropy / ops.upsample_cross_entropy; kernels in csrc/loss.hip).

ImageBasedCrossEntropyLoss2d is the per-image class-weighted loss the DeepLabV3+ baseline that network/deepv3.py derives from was
trained with.  Its source is not in the reference tree: the rule stated in ops.label_class_weights is the definition here
(build-defined).  The published form copies the label map to the host every step for np.histogram; here the
histogram, the weights and the loss stay on the device, with no synchronisation.

ImgWtLossSoftNLL is the joint-weighted soft-NLL loss of that baseline, the criterion that consumes the relaxed boundary targets of
the reference's transforms/transforms.py:75-124 (`jointwtborder`, utils/misc.py:51).  Its source is not in the reference tree
either: include/mrfp_hip.h and DESIGN.md section 8 hold the definition.  The published form builds a [B, C+1, H, W] uint8 multi-hot on
the host and copies it back every step for the class histogram; here a relaxed target is one int32 word per pixel (ops.relax_labels),
and relaxation, histogram, weights and loss are device kernels (csrc/relax.hip).

OhemCrossEntropy2d is the online-hard-example-mining cross entropy of the same lineage (the published OhemCrossEntropy2dTensor; its
source is not in the reference tree: include/mrfp_hip.h and DESIGN.md section 8 hold the definition).  The published form soft-maxes
the full-resolution logits, sorts every probability and branches on a host value; here the kept set is chosen by device kernels
with no host wait (csrc/ohem.hip: probability plane, exact radix select, masked target) and the loss is the fused cross entropy on
the masked target.

FocalLoss2d and RegionLoss2d are the two families a caller reaches for when mIoU, not pixel accuracy, is the metric: a focal term
that down-weights easy pixels, and the soft Dice / Jaccard overlap term, a direct surrogate of the IoU harness.evaluate reports,
almost always used as CE + lambda * Dice -- SumLoss.  Neither is in the reference tree: include/mrfp_hip.h and DESIGN.md section 8
hold the definitions; the kernels are csrc/loss.hip (Focal) and csrc/region.hip.

LovaszSoftmax2d is the third: the Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018), the convex surrogate of the Jaccard
index, usually trained as CE + lambda * Lovasz -- SumLoss again.  Not in the reference tree either; the published form soft-maxes the
full-resolution logits and runs one torch.sort and one cumulative sum per class on them; here the ranking is a stable segmented
radix sort on the device (csrc/sort.hip, csrc/lovasz.hip) and the fused form never writes the full-resolution logits.

ConsistencyLoss2d compares the class scores of TWO forward passes instead of scores with a label map: KL against a teacher at a
temperature, the Jensen-Shannon divergence of two views, or the pseudo-label cross entropy with a confidence threshold -- the
regulariser of MRFP's perturbed against its unperturbed view, self-training against the averaged weights, distillation into a smaller
model.  Not in the reference tree: include/mrfp_hip.h and DESIGN.md section 8 hold the definitions; the kernels are csrc/consist.hip.
It is NOT an (inputs, targets) criterion: a model refuses it as `criterion`, harness.ConsistencyStep is the callable that runs it.
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops

__all__ = ["ImageBasedCrossEntropyLoss2d", "ImgWtLossSoftNLL", "OhemCrossEntropy2d", "FocalLoss2d", "RegionLoss2d",
           "LovaszSoftmax2d", "SumLoss", "ScoreMap", "ConsistencyLoss2d", "fused_ce_kwargs", "fused_loss"]


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


class ImgWtLossSoftNLL(nn.Module):
    """sum over the images of sum_valid (W_i / k_i) (-log sum_{c in set_i} softmax_c) / (valid_b + 1), the class weights w from the
    relaxed target's own per-image bit counts (batch_weights: from the whole batch's).  The target is an int64 [B,H,W] label map
    (relaxed here with `border` / `strict_classes`), int32 [B,H,W] words (ops.relax_labels, input_pipeline.RelaxedBoundaryTarget) or
    the reference's uint8 [B, C+1, H, W] multi-hot."""

    def __init__(self, classes, ignore_index=255, weights=None, upper_bound=1.0, norm=False, batch_weights=False, border=1,
                 strict_classes=None):
        super().__init__()
        if weights is not None:
            raise ValueError("ImgWtLossSoftNLL computes its class weights from the relaxed target on every call (the original "
                             "overwrites a fixed weight): weights must be None")
        self.num_classes, self.border = ops._relax_args("ImgWtLossSoftNLL", classes, border)
        self.strict_classes = None if strict_classes is None else [int(c) for c in strict_classes]
        ops.strict_class_mask(self.strict_classes, self.num_classes)
        self.ignore_index = int(ignore_index)        # documentation only: every label outside 0..classes-1 is ignore
        self.upper_bound = float(upper_bound)
        self.norm = bool(norm)
        self.batch_weights = bool(batch_weights)

    def relaxed(self, target):
        """(int32 [B,H,W] words, int64 [B, C+1] counts) of a target in any of the three forms."""
        if target.dtype == torch.int32 and target.dim() == 3:
            return target, ops.relaxed_counts(target, self.num_classes)
        if target.dtype == torch.uint8 and target.dim() == 4:
            if target.shape[1] != self.num_classes + 1:
                raise ValueError("ImgWtLossSoftNLL: a multi-hot target has classes + 1 = %d planes (got %d)" % (
                    self.num_classes + 1, target.shape[1]))
            return ops.pack_multihot(target, want_counts=True)
        if target.dtype == torch.int64 and target.dim() == 3:
            return ops.relax_labels(target, self.num_classes, self.border, self.strict_classes, want_counts=True)
        raise ValueError("ImgWtLossSoftNLL: the target is an int64 [B,H,W] label map, int32 [B,H,W] words or a uint8 [B,C+1,H,W] "
                         "multi-hot (got %s %s)" % (target.dtype, tuple(target.shape)))

    def fused(self, logits, target, size=None, channels=None):
        """The loss on the kernels: of dense logits, or with `size` of the channel-padded low-resolution scores."""
        words, counts = self.relaxed(target)
        w = ops.relaxed_class_weights(counts, self.upper_bound, self.norm, self.batch_weights)
        if size is not None:
            return ops.upsample_soft_nll(logits, words, size, channels, weight=w)
        return ops.soft_nll(logits, words, self.num_classes, weight=w)

    def forward(self, inputs, target):
        return self.fused(inputs, target)


class OhemCrossEntropy2d(nn.Module):
    """nn.CrossEntropyLoss(weight, ignore_index) over the pixels the OHEM rule keeps: the valid pixels whose probability of the true
    class is at most max(thresh, the min_kept-th smallest such probability of the batch); every valid pixel when the batch has fewer
    than min_kept.  The selection is per rank and a constant for the backward."""

    def __init__(self, ignore_index=255, thresh=0.7, min_kept=100000, weight=None):
        super().__init__()
        self.thresh, self.min_kept = ops._ohem_args("OhemCrossEntropy2d", thresh, min_kept)
        self.ignore_index = int(ignore_index)
        # moves with the model, stays out of its state_dict
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight, dtype=torch.float32).detach().clone(),
                             persistent=False)

    def fused(self, logits, gts, size=None, channels=None):
        """The loss on the kernels: of dense logits, or with `size` of the channel-padded low-resolution scores."""
        if size is not None:
            return ops.upsample_ohem_cross_entropy(logits, gts, size, channels, self.ignore_index, thresh=self.thresh,
                                                   min_kept=self.min_kept, weight=self.weight)
        return ops.ohem_cross_entropy(logits, gts, self.ignore_index, thresh=self.thresh, min_kept=self.min_kept, weight=self.weight)

    def forward(self, inputs, targets):
        return self.fused(inputs, targets)


class FocalLoss2d(nn.Module):
    """-w[t] (1 - p_t)^gamma log p_t over the valid pixels, reduced as nn.CrossEntropyLoss(weight, ignore_index, reduction) reduces:
    'mean' divides by the sum of the target weights.  gamma = 0 is that cross entropy.  At most 64 classes."""

    def __init__(self, gamma=2.0, weight=None, ignore_index=255, reduction="mean"):
        super().__init__()
        self.gamma = ops._focal_options("FocalLoss2d", gamma)
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("FocalLoss2d: reduction must be 'mean', 'sum' or 'none' (got %r)" % (reduction,))
        self.ignore_index, self.reduction = int(ignore_index), reduction
        # moves with the model, stays out of its state_dict
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight, dtype=torch.float32).detach().clone(),
                             persistent=False)

    def fused(self, logits, gts, size=None, channels=None):
        """The loss on the kernels: of dense logits, or with `size` of the channel-padded low-resolution scores.  reduction='none'
        has no kernel: the operator refuses it."""
        kw = dict(gamma=self.gamma, weight=self.weight, reduction=self.reduction)
        if size is not None:
            return ops.upsample_focal_loss(logits, gts, size, channels, self.ignore_index, **kw)
        return ops.focal_loss(logits, gts, self.ignore_index, **kw)

    def forward(self, inputs, targets):
        return self.fused(inputs, targets)


class RegionLoss2d(nn.Module):
    """The soft Dice (kind='dice') or Jaccard ('jaccard') loss of softmax(inputs) against the one-hot targets over the valid pixels:
    the weighted mean over the classes of 1 - S_c, S_c = (2 I_c + s) / (P_c + T_c + s) or (I_c + s) / (P_c + T_c - I_c + s), over the
    classes present in the scope (present_only) or all of them (needs smooth > 0).  The scope is the whole batch of this rank -- under
    data parallelism the sums are per rank, like the OHEM selection -- or each image (per_image), averaged over the images that have
    a class.  Nothing valid: 0.  At most 64 classes."""

    def __init__(self, kind="dice", smooth=1.0, present_only=True, weight=None, ignore_index=255, per_image=False):
        super().__init__()
        _, self.smooth, self.present_only, _ = ops._region_options("RegionLoss2d", kind, smooth, present_only, None, None, None)
        self.kind, self.ignore_index, self.per_image = kind, int(ignore_index), bool(per_image)
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight, dtype=torch.float32).detach().clone(),
                             persistent=False)

    def fused(self, logits, gts, size=None, channels=None):
        """The loss on the kernels: of dense logits, or with `size` of the channel-padded low-resolution scores."""
        kw = dict(kind=self.kind, smooth=self.smooth, present_only=self.present_only, weight=self.weight, per_image=self.per_image)
        if size is not None:
            return ops.upsample_region_loss(logits, gts, size, channels, self.ignore_index, **kw)
        return ops.region_loss(logits, gts, self.ignore_index, **kw)

    def forward(self, inputs, targets):
        return self.fused(inputs, targets)


class LovaszSoftmax2d(nn.Module):
    """The Lovasz-Softmax loss of softmax(inputs) against the targets over the valid pixels: per class the errors |[t == c] - p_c| of the
    scope's pixels, sorted descending (ties by ascending pixel index: the order, and so the gradient, is reproducible), weighted by the
    Lovasz gradient of the Jaccard loss; the mean over the classes present in the scope (classes='present') or over all ('all').  The
    scope is the whole batch of this rank -- under data parallelism the order is per rank, like the OHEM selection -- or each image
    (per_image), averaged over the images that have a counted class (the published helper also averages all-ignored images in, as 0).
    Nothing valid: 0.  At most 64 classes, B * H * W < 2^31."""

    def __init__(self, classes="present", per_image=False, ignore_index=255):
        super().__init__()
        ops._lovasz_options("LovaszSoftmax2d", classes)
        self.classes, self.per_image, self.ignore_index = classes, bool(per_image), int(ignore_index)

    def fused(self, logits, gts, size=None, channels=None):
        """The loss on the kernels: of dense logits, or with `size` of the channel-padded low-resolution scores."""
        kw = dict(classes=self.classes, per_image=self.per_image)
        if size is not None:
            return ops.upsample_lovasz_softmax(logits, gts, size, channels, self.ignore_index, **kw)
        return ops.lovasz_softmax(logits, gts, self.ignore_index, **kw)

    def forward(self, inputs, targets):
        return self.fused(inputs, targets)


class SumLoss(nn.Module):
    """sum_k w_k * crit_k(inputs, targets): SumLoss((1.0, nn.CrossEntropyLoss(ignore_index=255)), (0.5, RegionLoss2d())).  Its fused
    form is the same sum of the parts' fused forms over the same scores; it has one only if every part has."""

    def __init__(self, *parts):
        super().__init__()
        if not parts:
            raise ValueError("SumLoss: at least one (weight, criterion) pair")
        for part in parts:
            if not (isinstance(part, (tuple, list)) and len(part) == 2 and isinstance(part[1], nn.Module)):
                raise ValueError("SumLoss: every part is a (weight, criterion module) pair (got %r)" % (part,))
        self.weights = [float(w) for w, _ in parts]
        self.criteria = nn.ModuleList([c for _, c in parts])

    def parts(self):
        return list(zip(self.weights, self.criteria))

    def fused(self, logits, gts, size=None, channels=None):
        """sum_k w_k * fused_loss(crit_k, ...), or None if a part has no fused form."""
        if any(fused_ce_kwargs(c) is None for c in self.criteria):
            return None
        total = None
        for w, c in self.parts():
            term = w * fused_loss(c, logits, gts, size, channels)
            total = term if total is None else total + term
        return total

    def forward(self, inputs, targets):
        total = self.fused(inputs, targets)
        if total is None:          # a part the kernels do not compute: every part as its module computes it
            for w, c in self.parts():
                term = w * c(inputs, targets)
                total = term if total is None else total + term
        return total


class ScoreMap:
    """Fused class scores: P, the channel-padded low-resolution buffer [B,ld,Hi,Wi] of a model's head (autograd-attached where the
    model trains), to be upsampled to `size` = (H, W) inside the loss kernel, its first `channels` planes the classes."""
    __slots__ = ("P", "size", "channels")

    def __init__(self, P, size, channels):
        self.P, self.size, self.channels = P, (int(size[0]), int(size[1])), int(channels)

    def detach(self):
        return ScoreMap(self.P.detach(), self.size, self.channels)


class ConsistencyLoss2d(nn.Module):
    """forward(student, teacher, valid=None): ops.consistency_loss of two dense logit tensors, or ops.upsample_consistency_loss of two
    ScoreMaps of one size and class count (their pitch and low resolution may differ).  kind 'kl' (T^2 KL(teacher || student), the
    teacher a constant), 'js' (T^2 times the Jensen-Shannon divergence, a gradient to every view that requires one) or 'hard' (cross
    entropy against the teacher's arg-max where its confidence reaches `threshold`, over the kept pixels or, normalize='valid', over
    the counted ones).  valid: an int64 [B,H,W] label map, a pixel counts iff 0 <= valid < C; None: every pixel.  Nothing counted or
    kept: 0.  At most 64 classes.  Not an (inputs, targets) criterion: fused_ce_kwargs has no entry for it and a model refuses it."""

    def __init__(self, kind="kl", temperature=1.0, threshold=0.0, normalize="kept"):
        super().__init__()
        ops._consist_options("ConsistencyLoss2d", kind, temperature, threshold, normalize)
        self.kind, self.temperature, self.threshold, self.normalize = kind, float(temperature), float(threshold), normalize

    def forward(self, student, teacher, valid=None, want_counts=False):
        if isinstance(teacher, torch.Tensor) and not teacher.is_floating_point():
            raise TypeError("ConsistencyLoss2d compares the class scores of two forward passes: forward(student, teacher, valid=None); "
                            "it is not an (inputs, targets) criterion (got an integer tensor as the teacher's scores)")
        kw = dict(kind=self.kind, temperature=self.temperature, threshold=self.threshold, normalize=self.normalize,
                  want_counts=want_counts)
        fused = (isinstance(student, ScoreMap), isinstance(teacher, ScoreMap))
        if fused[0] != fused[1]:
            raise ops._lib.MrfpHipError("ConsistencyLoss2d: both views are dense logits or both are ScoreMaps (mixed forms are not built)")
        if not fused[0]:
            return ops.consistency_loss(student, teacher, valid, **kw)
        if student.size != teacher.size or student.channels != teacher.channels:
            raise ops._lib.MrfpHipError("ConsistencyLoss2d: the two ScoreMaps have one output size and one class count (got %s x %d and "
                                        "%s x %d)" % (student.size, student.channels, teacher.size, teacher.channels))
        return ops.upsample_consistency_loss(student.P, teacher.P, student.size, student.channels, valid, **kw)


def refuse_two_view_criterion(name, criterion):
    """A model's `criterion` / `criterion_aux` is called as criterion(inputs, targets): ConsistencyLoss2d is not such a module."""
    if isinstance(criterion, ConsistencyLoss2d):
        raise TypeError("%s: ConsistencyLoss2d compares two forward passes, forward(student, teacher, valid=None), and is not an "
                        "(inputs, targets) criterion: keep the model's supervised criterion and hand the Trainer a "
                        "harness.ConsistencyStep as loss_fn" % name)


def fused_ce_kwargs(criterion):
    """The keyword arguments with which ops.cross_entropy / ops.upsample_cross_entropy compute `criterion`, or None for a criterion
    they cannot (reduction='none', a foreign module): that one keeps the stock call on the full-resolution fp32 logits.  `weight` is
    a tensor, None, or -- for the per-image criterion -- a callable of the label map (fused_loss calls it).  ImgWtLossSoftNLL is not a
    cross entropy: its entry is dict(soft_nll=<its own fused call>), which fused_loss calls with (logits, gts, size, channels);
    OhemCrossEntropy2d chooses its pixels first: dict(ohem=<its own fused call>), called the same way; so are FocalLoss2d (dict(focal=),
    None with reduction='none'), RegionLoss2d (dict(region=)), LovaszSoftmax2d (dict(lovasz=)) and SumLoss (dict(sum=), None if a part has none)."""
    c = criterion
    if isinstance(c, ConsistencyLoss2d):          # two forward passes, no label map: not an (inputs, targets) criterion at all
        return None
    if isinstance(c, FocalLoss2d):
        return dict(focal=c.fused) if c.reduction in ("mean", "sum") else None
    if isinstance(c, RegionLoss2d):
        return dict(region=c.fused)
    if isinstance(c, LovaszSoftmax2d):
        return dict(lovasz=c.fused)
    if isinstance(c, SumLoss):
        return None if any(fused_ce_kwargs(p) is None for p in c.criteria) else dict(sum=c.fused)
    if isinstance(c, OhemCrossEntropy2d):
        return dict(ohem=c.fused)
    if isinstance(c, ImgWtLossSoftNLL):          # not a cross entropy: fused_loss hands the call to the criterion's own kernels
        return dict(soft_nll=c.fused)
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
    for own in ("soft_nll", "ohem", "focal", "region", "lovasz", "sum"):
        if own in kw:
            return kw[own](logits, gts, size, channels)
    ignore = kw.pop("ignore_index")
    if callable(kw["weight"]):
        kw["weight"] = kw["weight"](gts)
    if size is not None:
        return ops.upsample_cross_entropy(logits, gts, size, channels, ignore, **kw)
    return ops.cross_entropy(logits, gts, ignore, **kw)
