"""Shared by test_ohem_cpu.py and test_ohem_gpu.py: the OHEM selection rule of include/mrfp_hip.h / DESIGN.md section 8 restated in
numpy on a given probability plane, the published module's masking restated in torch, and the seeded inputs of the GPU cases."""
import numpy as np
import torch
import torch.nn.functional as F

IGNORE = 255
SENTINEL = np.float32(2.0)
KEEP_ALL, THRESH, KTH = 0, 1, 2


def valid_mask(t, C, ignore=IGNORE):
    t = np.asarray(t)
    return (t != ignore) & (t >= 0) & (t < C)


def rule(p, t, C, thresh, min_kept, ignore=IGNORE):
    """The rule on the probability plane p (float32 or float64 numpy, any value where the pixel is invalid) and the int64 labels t
    -> (masked target, N, kept count, theta in p's type, mode).  np.sort puts NaN last, as torch.sort; `<=` is false for a NaN."""
    p, t = np.asarray(p), np.asarray(t)
    valid = valid_mask(t, C, ignore)
    N = int(valid.sum())
    th = p.dtype.type(thresh)
    if N == 0 or min_kept > N:
        kept, theta, mode = valid, p.dtype.type(np.inf), KEEP_ALL
    else:
        theta, mode = th, THRESH
        if min_kept > 0:
            q = np.sort(p[valid])[min_kept - 1]
            if q > th:
                theta, mode = q, KTH
        with np.errstate(invalid="ignore"):
            kept = valid & (p <= theta)
    return np.where(kept, t, ignore), N, int(kept.sum()), theta, mode


def theta_bits(theta):
    return int(np.float32(theta).view(np.uint32))


def published_masked(pred, target, thresh, min_kept, ignore=IGNORE):
    """The masking of the published OhemCrossEntropy2dTensor.forward, statement for statement (its labels are classes or `ignore`; it
    prints where this returns early).  pred [B,C,H,W], target int64 [B,H,W] -> the masked target it hands nn.CrossEntropyLoss."""
    b, c, h, w = pred.shape
    target = target.clone().view(-1)
    valid = target.ne(ignore)
    target = target * valid.long()
    num_valid = int(valid.sum())
    prob = F.softmax(pred, dim=1).transpose(0, 1).reshape(c, -1)
    if min_kept > num_valid:
        pass
    elif num_valid > 0:
        prob = prob.masked_fill(~valid, 1)
        mask_prob = prob[target, torch.arange(len(target))]
        threshold = thresh
        if min_kept > 0:
            index = mask_prob.argsort()
            threshold_index = index[min(len(index), min_kept) - 1]
            if mask_prob[threshold_index] > thresh:
                threshold = mask_prob[threshold_index]
        kept = mask_prob.le(threshold)
        target = target * kept.long()
        valid = valid & kept
    return target.masked_fill(~valid, ignore).view(b, h, w)


def true_class_prob(z, t, C, ignore=IGNORE):
    """exp(z_t - lse) in float64 of class vectors z [..., C] (any float type) at the valid pixels of t [...]; NaN elsewhere."""
    z = np.asarray(z, dtype=np.float64)
    valid = valid_mask(t, C, ignore)
    m = z.max(-1, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(z - m).sum(-1))
    zt = np.take_along_axis(z, np.where(valid, t, 0)[..., None], -1)[..., 0]
    return np.where(valid, np.exp(zt - lse), np.nan)


def labels(B, H, W, C, seed, only_ignore=False):
    """int64 [B,H,W]: uniform classes, ~10 % 255, and (unless only_ignore) some -1, C and 200, all invalid."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (B, H, W), generator=g)
    r = torch.rand(B, H, W, generator=g)
    y[r < 0.10] = IGNORE
    if not only_ignore:
        y[(r >= 0.10) & (r < 0.13)] = -1
        y[(r >= 0.13) & (r < 0.16)] = C
        y[(r >= 0.16) & (r < 0.19)] = 200
    return y


def logits(B, C, H, W, dtype, seed, scale=2.5, boost=3.0, y=None):
    """host [B,C,H,W] of `dtype`: scale * randn, plus `boost` on the true class where y gives one; rounded to the dtype."""
    g = torch.Generator().manual_seed(seed)
    x = scale * torch.randn(B, C, H, W, generator=g)
    if y is not None:
        ok = torch.from_numpy(valid_mask(y.numpy(), C))
        x += boost * F.one_hot(torch.where(ok, y, torch.zeros_like(y)), C).permute(0, 3, 1, 2) * ok[:, None]
    return x.to(dtype)


def widest_gap(sorted_vals, lo, hi):
    """(index i, relative gap) of the widest relative gap v[i+1] / v[i] - 1 between consecutive sorted values with lo <= i < hi (hi
    clipped to the last pair)"""
    v = np.asarray(sorted_vals, dtype=np.float64)
    hi = min(hi, len(v) - 1)
    rel = v[lo + 1:hi + 1] / v[lo:hi] - 1.0
    i = int(np.argmax(rel))
    return lo + i, float(rel[i])
