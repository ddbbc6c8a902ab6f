"""Shared by test_consistency_cpu.py and test_consistency_gpu.py: the float64 torch restatements of the three two-view consistency
kinds (include/mrfp_hip.h: mrfp_consist_*), written with torch ops so that autograd supplies the reference gradients, an independent
numpy loop, and the seeded inputs of the tests.  test_consistency_cpu.py pins the restatements (against F.kl_div, F.cross_entropy and
the numpy loop); the GPU tests compare the kernels with them.

The input rule (a condition on the inputs, not a measurement): the kept set of kind 'hard' has to be the same in fp32 on the device
and in float64 here.  make_views rounds the inputs to the activation dtype first; for FUSED views it takes a pixel out (valid = 255)
where the teacher's float64 top-2 logit margin is < 1e-3 (an interpolated near-tie may resolve either way in fp32) or its confidence
is within 1e-4 of the threshold, and asserts that at most 2 % of the pixels go; for DENSE views only the threshold band applies: the
arg-max is taken on the exact inputs, so exact ties (the 16-bit 33 x 65 cases have them) test the first-maximum rule."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import loss_common as lc

IGNORE = lc.IGNORE
KINDS = ("kl", "js", "hard")
MARGIN, BAND, MAX_EXCLUDED = 1e-3, 1e-4, 0.02


def counted_mask(valid, C, shape):
    if valid is None:
        return torch.ones(shape, dtype=torch.bool)
    return (valid >= 0) & (valid < C)


def first_argmax(zt):
    """np.argmax over the class axis: the first maximum."""
    return torch.from_numpy(np.argmax(zt.detach().numpy(), axis=1))


def ref_consistency(zs, zt, valid=None, kind="kl", T=1.0, threshold=0.0, normalize="kept", want_counts=False):
    """zs, zt [B,C,H,W] float64 (either may require a gradient), valid int64 [B,H,W] or None (counted iff 0 <= valid < C).
    kl: T^2 sum_c q_c (log q_c - log p_c), q a constant; js: T^2 (KL(p||m) + KL(q||m)) / 2; both the mean over the counted pixels.
    hard: -log softmax(zs)_k, k the teacher's first arg-max, over the counted pixels with softmax(zt)_k >= threshold (T = 1), divided by
    their number ('kept') or by the counted pixels ('valid').  An empty denominator: 0."""
    B, C, H, W = zs.shape
    counted = counted_mask(valid, C, (B, H, W))
    n = int(counted.sum())
    if kind == "hard":
        ztd = zt.detach()
        k = first_argmax(ztd)
        conf = F.softmax(ztd, 1).gather(1, k[:, None])[:, 0]
        kept = counted & (conf >= threshold)
        l = -F.log_softmax(zs, 1).gather(1, k[:, None])[:, 0]
        nk = int(kept.sum())
        D = nk if normalize == "kept" else n
        loss = (l * kept).sum() / D if D > 0 else zs.sum() * 0.0
    else:
        lp = F.log_softmax(zs / T, 1)
        lq = F.log_softmax(zt / T, 1)
        if kind == "kl":
            lq = lq.detach()
            l = (lq.exp() * (lq - lp)).sum(1)
        else:
            lm = torch.logaddexp(lp, lq) - math.log(2.0)
            l = 0.5 * ((lp.exp() * (lp - lm)).sum(1) + (lq.exp() * (lq - lm)).sum(1))
        nk = n
        loss = T * T * (l * counted).sum() / n if n > 0 else (zs.sum() + zt.sum()) * 0.0
    return (loss, (n, nk)) if want_counts else loss


def np_consistency(zs, zt, valid, kind, T, threshold, normalize):
    """The same in plain numpy loops over pixels and classes (the independent restatement of the CPU test)."""
    zs, zt = np.asarray(zs, dtype=np.float64), np.asarray(zt, dtype=np.float64)
    B, C, H, W = zs.shape
    total, n, nk = 0.0, 0, 0

    def softmax(v):
        e = np.exp(v - v.max())
        return e / e.sum()
    for b in range(B):
        for i in range(H):
            for j in range(W):
                if valid is not None and not 0 <= int(valid[b, i, j]) < C:
                    continue
                n += 1
                s, t = zs[b, :, i, j], zt[b, :, i, j]
                if kind == "hard":
                    k = int(np.argmax(t))
                    if softmax(t)[k] >= threshold:
                        nk += 1
                        total += -math.log(softmax(s)[k])
                    continue
                nk += 1
                p, q = softmax(s / T), softmax(t / T)
                if kind == "kl":
                    total += T * T * sum(q[c] * (math.log(q[c]) - math.log(p[c])) for c in range(C))
                else:
                    m = 0.5 * (p + q)
                    total += T * T * 0.5 * sum(p[c] * math.log(p[c] / m[c]) + q[c] * math.log(q[c] / m[c]) for c in range(C))
    D = nk if (kind == "hard" and normalize == "kept") else n
    return (total / D if D > 0 else 0.0), (n, nk)


def upsampled(x, size):
    return F.interpolate(x, size, mode="bilinear", align_corners=True)


def threshold_for(C, threshold):
    """N(0, 2^2) logits over two classes are confident nearly everywhere: only 0.9 leaves some pixels out there."""
    return 0.9 if C == 2 else threshold


def make_views(B, C, H, W, dtype, seed, low_s=None, low_t=None, threshold=None, blank_image=None, scale=2.0):
    """-> (xs, xt, valid): the two views as float32 holding values of `dtype` -- [B,C,H,W], or with low_s / low_t = (h, w) the
    low-resolution scores of each -- independent N(0, scale^2) draws, and an int64 [B,H,W] label map (loss_common.make_labels: ~10 %
    255, a few -1 and C) from which the input rule of the module docstring has taken the ambiguous pixels for `threshold`
    (None: kinds that keep every counted pixel)."""
    g = torch.Generator().manual_seed(seed)
    hs, ws = low_s if low_s is not None else (H, W)
    ht, wt = low_t if low_t is not None else (H, W)
    xs = (torch.randn(B, C, hs, ws, generator=g) * scale).to(dtype).float()
    xt = (torch.randn(B, C, ht, wt, generator=g) * scale).to(dtype).float()
    valid = lc.make_labels(B, C, H, W, g)
    if blank_image is not None:
        valid[blank_image] = IGNORE
    if threshold is not None:
        fused = low_t is not None
        z = upsampled(xt.double(), (H, W)) if fused else xt.double()
        top = z.topk(2, dim=1).values
        conf = F.softmax(z, 1).max(1).values
        out = (conf - threshold).abs() < BAND
        if fused:
            out |= (top[:, 0] - top[:, 1]) < MARGIN
        share = float(out.double().mean())
        assert share <= MAX_EXCLUDED, "the input rule takes %.3f of the pixels out (C=%d, threshold=%g)" % (share, C, threshold)
        valid[out] = IGNORE
    return xs, xt, valid
