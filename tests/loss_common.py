"""Shared by test_loss_cpu.py and test_loss_gpu.py: the float64 torch restatement of the weighted / label-smoothed / per-image
cross entropy (include/mrfp_hip.h, mrfp_ce_w_*) and the seeded inputs of its tests.  test_loss_cpu.py pins the restatement against
torch's own F.cross_entropy; the GPU tests compare the kernels with it."""
import numpy as np
import torch
import torch.nn.functional as F

IGNORE = 255
MODES = ("mean", "sum", "image_mean")


def mask_invalid(y, C):
    """The kernels treat every label outside 0..C-1 as ignored; torch raises for them (as test_launch_geometry_gpu._mask_invalid)."""
    return torch.where((y >= 0) & (y < C), y, torch.full_like(y, IGNORE))


def ref_loss(logits, y, w, eps, mode):
    """logits [B,C,H,W] float64, y int64 [B,H,W] (ignored = 255 only), w float64 [C] / [B,C] / None.
    mean / sum with one weight row: F.cross_entropy itself.  Otherwise the per-image loop over F.nll_loss(weight=w_b):
    num_b = (1-eps) * sum_i w_b[t_i] (-lp_i[t_i]) + (eps/C) * sum_i sum_c w_b[c] (-lp_i[c]),  den_b = sum_i w_b[t_i]  (valid i);
    mean = sum_b num_b / sum_b den_b, sum = sum_b num_b, image_mean = sum_b num_b / den_b."""
    B, C = logits.shape[:2]
    if w is None:
        w = torch.ones(C, dtype=torch.float64)
    if mode in ("mean", "sum") and w.dim() == 1:
        return F.cross_entropy(logits, y, weight=w, ignore_index=IGNORE, reduction=mode, label_smoothing=eps)
    lp = F.log_softmax(logits, 1)
    nums, dens = [], []
    for b in range(B):
        wb = w[b] if w.dim() == 2 else w
        valid = y[b] != IGNORE
        num = (1.0 - eps) * F.nll_loss(lp[b:b + 1], y[b:b + 1], weight=wb, ignore_index=IGNORE, reduction="sum")
        if eps:
            num = num + (eps / C) * ((-lp[b] * wb.view(C, 1, 1)).sum(0) * valid).sum()
        nums.append(num)
        dens.append(wb[y[b][valid]].sum())
    if mode == "mean":
        return sum(nums) / sum(dens)
    if mode == "sum":
        return sum(nums)
    return sum(n / d for n, d in zip(nums, dens))


def make_labels(B, C, H, W, g):
    """~10 % of the labels 255, a few -1 and C (ignored by the kernels), and class C-1 absent (C > 2)."""
    y = torch.randint(0, C - 1 if C > 2 else C, (B, H, W), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.1] = IGNORE
    flat = y.view(-1)
    n = flat.numel()
    if n >= 8:
        flat[int(torch.randint(0, n, (1,), generator=g))] = -1
        flat[int(torch.randint(0, n, (1,), generator=g))] = C
        if n >= 64:
            flat[3] = -1
            flat[n - 5] = C
    return y


def make_weights(C, g, rows=None):
    """uniform in [0.5, 1.5], class 0 exactly 0 (row r of a per-image table: class r % C)."""
    w = torch.rand((C,) if rows is None else (rows, C), generator=g) + 0.5
    if rows is None:
        w[0] = 0.0
    else:
        for r in range(rows):
            w[r, r % C] = 0.0
    return w


def np_class_weights(t, C, upper_bound, norm, batch):
    """The per-image rule in numpy: np.histogram(t, range(C+1)), the two formulas in float64, one rounding to float32."""
    t = np.asarray(t)
    rows = [t.reshape(-1)] if batch else [t[b].reshape(-1) for b in range(t.shape[0])]
    out = []
    for r in rows:
        n = np.histogram(r, range(C + 1))[0].astype(np.float64)
        total = n.sum()
        w = np.ones(C, dtype=np.float64)
        nz = n > 0
        f = n[nz] / total
        w[nz] = 1.0 + upper_bound / f if norm else 1.0 + upper_bound * (1.0 - f)
        out.append(w)
    return np.stack(out).astype(np.float32)
