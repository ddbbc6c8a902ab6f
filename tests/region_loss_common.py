"""Shared by test_region_loss_cpu.py and test_region_loss_gpu.py: the float64 torch restatements of the focal loss and of the soft
Dice / Jaccard region loss (include/mrfp_hip.h: mrfp_focal_*, mrfp_region_*), written with torch ops so that autograd supplies the
reference gradient, and the seeded inputs of their tests.  test_region_loss_cpu.py pins the restatements (against F.cross_entropy
and an independent numpy loop); the GPU tests compare the kernels with them."""
import numpy as np
import torch
import torch.nn.functional as F

import loss_common as lc

IGNORE = lc.IGNORE
MODES = lc.MODES
GAMMAS = (0.0, 0.5, 2.0, 5.0)
KINDS = ("dice", "jaccard")


def _onehot(y, C):
    """(valid [B,1,H,W], one-hot [B,C,H,W] zero at invalid pixels) in float64; y's invalid labels are 255 only."""
    valid = (y != IGNORE)
    oh = F.one_hot(torch.where(valid, y, torch.zeros_like(y)), C).permute(0, 3, 1, 2).double() * valid[:, None]
    return valid[:, None].double(), oh


def ref_focal(logits, y, w, gamma, mode):
    """logits [B,C,H,W] float64, y int64 [B,H,W] (ignored = 255 only), w float64 [C] / [B,C] / None.
    l_i = -w_b[t_i] (1 - p_t)^gamma log p_t, 1 - p_t as the sum of the other probabilities; num_b = sum_i l_i, den_b = sum_i w_b[t_i]
    over the valid pixels of image b; mean = sum_b num_b / sum_b den_b, sum = sum_b num_b, image_mean = sum_b num_b / den_b."""
    B, C = logits.shape[:2]
    if w is None:
        w = torch.ones(C, dtype=torch.float64)
    wb = (w if w.dim() == 2 else w[None].expand(B, C)).double()
    valid, oh = _onehot(y, C)
    lp = F.log_softmax(logits, 1)
    lpt = (lp * oh).sum(1)
    q = (lp.exp() * (valid - oh)).sum(1)
    mod = torch.ones_like(q) if gamma == 0 else q.clamp_min(1e-300) ** gamma
    wt = (wb[:, :, None, None] * oh).sum(1)
    nums = (-wt * mod * lpt).sum((1, 2))
    dens = wt.sum((1, 2))
    if mode == "mean":
        return nums.sum() / dens.sum()
    if mode == "sum":
        return nums.sum()
    return (nums / dens).sum()


def ref_region(logits, y, w=None, kind="dice", smooth=1.0, present_only=True, per_image=False, want_sums=False):
    """logits [B,C,H,W] float64, y int64 [B,H,W] (ignored = 255 only), w float64 [C] / None.  Per scope group (the batch, or each
    image): I_c = sum p_c [t = c], P_c = sum p_c, T_c = #{t = c} over the valid pixels; S_c = (2 I_c + s) / (P_c + T_c + s) (dice),
    (I_c + s) / (P_c + T_c - I_c + s) (jaccard); L = sum_K w_c (1 - S_c) / sum_K w_c, K = {T_c > 0} or all; the mean of L over the
    groups whose sum_K w_c > 0, 0 if there is none."""
    B, C = logits.shape[:2]
    if w is None:
        w = torch.ones(C, dtype=torch.float64)
    valid, oh = _onehot(y, C)
    p = F.softmax(logits, 1) * valid
    dims = (2, 3) if per_image else (0, 2, 3)
    I, P, T = (p * oh).sum(dims).reshape(-1, C), p.sum(dims).reshape(-1, C), oh.sum(dims).reshape(-1, C)
    if want_sums:
        return torch.stack([I, P, T], 1)
    K = (T > 0).double() if present_only else torch.ones_like(T)
    if kind == "dice":
        N, D = 2.0 * I + smooth, P + T + smooth
    else:
        N, D = I + smooth, P + T - I + smooth
    S = N / torch.where(K > 0, D, torch.ones_like(D))
    wK = w.double()[None] * K
    WK = wK.sum(1)
    counts = WK > 0
    if not bool(counts.any()):
        return logits.sum() * 0.0
    L = (wK * (1.0 - S)).sum(1)[counts] / WK[counts]
    return L.mean()


def np_region(logits, y, w, kind, smooth, present_only, per_image):
    """The same in plain numpy loops over pixels and classes (the independent restatement of the CPU test)."""
    x = np.asarray(logits, dtype=np.float64)
    y = np.asarray(y)
    B, C, H, W = x.shape
    w = np.ones(C) if w is None else np.asarray(w, dtype=np.float64)
    groups = [[b] for b in range(B)] if per_image else [list(range(B))]
    losses = []
    for imgs in groups:
        I, P, T = np.zeros(C), np.zeros(C), np.zeros(C)
        for b in imgs:
            for i in range(H):
                for j in range(W):
                    t = int(y[b, i, j])
                    if t == IGNORE or t < 0 or t >= C:
                        continue
                    z = x[b, :, i, j]
                    e = np.exp(z - z.max())
                    pr = e / e.sum()
                    P += pr
                    I[t] += pr[t]
                    T[t] += 1
        num = den = 0.0
        for c in range(C):
            if present_only and T[c] == 0:
                continue
            S = (2 * I[c] + smooth) / (P[c] + T[c] + smooth) if kind == "dice" else (I[c] + smooth) / (P[c] + T[c] - I[c] + smooth)
            num += w[c] * (1.0 - S)
            den += w[c]
        if den > 0:
            losses.append(num / den)
    return float(np.mean(losses)) if losses else 0.0


def make_case(B, C, H, W, dtype, seed, scale=3.0, low=None, blank_image=None):
    """(logits rounded to dtype as float32 [B,C,h,w], labels [B,H,W], labels with every invalid one 255, class weights [C], per-image
    weights [B,C]).  low = (h, w): the scores are low-resolution and the labels have the output size (H, W).  blank_image: that image
    is ignored entirely.  loss_common.make_labels: ~10 % 255, a few -1 and C, class C-1 absent."""
    g = torch.Generator().manual_seed(seed)
    h, w_ = low if low is not None else (H, W)
    x = (torch.randn(B, C, h, w_, generator=g) * scale).to(dtype).float()
    y = lc.make_labels(B, C, H, W, g)
    if blank_image is not None:
        y[blank_image] = IGNORE
    return x, y, lc.mask_invalid(y, C), lc.make_weights(C, g), lc.make_weights(C, g, rows=B)
