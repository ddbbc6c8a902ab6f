"""Shared by test_lovasz_cpu.py and test_lovasz_gpu.py: the float64 numpy restatement of the Lovasz-Softmax loss as include/mrfp_hip.h
defines it (mrfp_lovasz_*), its gradient with g held constant, the two other forms the CPU test pins it against (Berman's
dot(errors_sorted, lovasz_grad(fg_sorted)) and the set-function form), and the seeded inputs of the tests.

The order of a scope's pixels is a stable sort by e descending, ties by ascending flat index.  ref_lovasz takes it from its own
float64 errors, or -- `order_errors` -- from error planes computed elsewhere (ops.lovasz_errors: the device's own fp32 errors), so
that near-ties between fp32 and fp64 errors cannot swap ranks when a gradient is compared element by element."""
import numpy as np
import torch

import loss_common as lc

IGNORE = lc.IGNORE


def softmax64(logits):
    z = np.asarray(logits, dtype=np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def stable_desc(e):
    """Positions in the order: e descending, ties by ascending position."""
    return np.argsort(-np.asarray(e, dtype=np.float64), kind="stable")


def class_terms(e, fg, order=None):
    """One class of one scope.  e [n] float64 errors and fg [n] 0/1 of the scope's VALID pixels in flat-index order -> (loss_c, g [n] in
    the same pixel order), by the definition: J_i = 1 - (G - F_i - f_i) / (G + B_i + 1 - f_i), J_i^- = 1 - (G - F_i) / (G + B_i) (0 for the
    first pixel), g_i = J_i - J_i^-, loss_c = sum e_i g_i.  order: a permutation to use instead of stable_desc(e)."""
    e = np.asarray(e, dtype=np.float64)
    f = np.asarray(fg, dtype=np.float64)
    n = e.shape[0]
    if n == 0:
        return 0.0, np.zeros(0)
    if order is None:
        order = stable_desc(e)
    fs = f[order]
    G = f.sum()
    F = np.cumsum(fs) - fs                 # foreground before
    Bk = np.arange(n) - F                  # background before
    J = 1.0 - (G - F - fs) / (G + Bk + 1.0 - fs)
    with np.errstate(divide="ignore", invalid="ignore"):
        Jm = 1.0 - (G - F) / (G + Bk)
    Jm[0] = 0.0
    gs = J - Jm
    g = np.empty(n)
    g[order] = gs
    return float((e[order] * gs).sum()), g


def berman_class(e, fg):
    """dot(errors_sorted, lovasz_grad(fg_sorted)) as published."""
    e = np.asarray(e, dtype=np.float64)
    f = np.asarray(fg, dtype=np.float64)
    if e.shape[0] == 0:
        return 0.0
    order = stable_desc(e)
    es, fs = e[order], f[order]
    gts = fs.sum()
    inter = gts - np.cumsum(fs)
    union = gts + np.cumsum(1.0 - fs)
    jac = 1.0 - inter / union
    jac[1:] = jac[1:] - jac[:-1]
    return float((es * jac).sum())


def set_function_class(e, fg):
    """sum_k e_(k) [J(S_k) - J(S_{k-1})], J(S) = the Jaccard loss when exactly the pixels of S are mispredicted: a mispredicted
    foreground pixel leaves the intersection, a mispredicted background pixel joins the union; J(empty) = 0."""
    e = np.asarray(e, dtype=np.float64)
    f = np.asarray(fg).astype(bool)
    order = stable_desc(e)
    G = int(f.sum())

    def J(S):
        if not S:
            return 0.0
        miss_fg = sum(1 for i in S if f[i])
        miss_bg = len(S) - miss_fg
        return 1.0 - (G - miss_fg) / (G + miss_bg)
    total, S = 0.0, []
    for i in order:
        before = J(S)
        S.append(int(i))
        total += e[i] * (J(S) - before)
    return total


def ref_lovasz(logits, y, classes="present", per_image=False, order_errors=None, want_grad=False):
    """logits [B,C,H,W] (any float array; computed in float64), y int64 [B,H,W] (a label outside 0..C-1 is ignored).  -> the loss, or
    (loss, d loss / d logits float64 [B,C,H,W]) with g held constant.  order_errors: [C,B,H,W] error planes whose stable descending
    order is used in place of the float64 errors' own (their values at invalid pixels are not looked at)."""
    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(y)
    B, C, H, W = z.shape
    p = softmax64(z)
    pf = p.transpose(0, 2, 3, 1).reshape(B * H * W, C)              # [N, C] in flat pixel order
    yf = y.reshape(-1)
    valid = (yf >= 0) & (yf < C) & (yf != IGNORE)
    oe = None if order_errors is None else np.asarray(order_errors, dtype=np.float64).reshape(C, B * H * W)
    scopes = [np.arange(b * H * W, (b + 1) * H * W) for b in range(B)] if per_image else [np.arange(B * H * W)]
    A = np.zeros((B * H * W, C))                                     # a_i[c] before the division by the scopes that count
    losses = []
    for idx in scopes:
        idx = idx[valid[idx]]
        if idx.size == 0:
            continue
        terms, rows = [], []
        for c in range(C):
            fg = (yf[idx] == c).astype(np.float64)
            if classes == "present" and fg.sum() == 0:
                continue
            e = np.abs(fg - pf[idx, c])
            order = None if oe is None else stable_desc(oe[c, idx])
            l, g = class_terms(e, fg, order)
            terms.append(l)
            rows.append((c, (1.0 - 2.0 * fg) * g))
        if not terms:
            continue
        losses.append(sum(terms) / len(terms))
        for c, a in rows:
            A[idx, c] = a / len(terms)
    loss = float(np.mean(losses)) if losses else 0.0
    if not want_grad:
        return loss
    if losses:
        A /= len(losses)
    grad = pf * (A - (A * pf).sum(1, keepdims=True))
    grad[~valid] = 0.0
    return loss, grad.reshape(B, H, W, C).transpose(0, 3, 1, 2)


def make_case(B, C, H, W, dtype, seed, scale=3.0, low=None, blank_image=None):
    """(logits rounded to dtype as float32 [B,C,h,w], labels [B,H,W]).  low = (h, w): the scores are low-resolution and the labels have
    the output size.  loss_common.make_labels: ~10 % 255, a few -1 and C, class C-1 absent (C > 2)."""
    g = torch.Generator().manual_seed(seed)
    h, w_ = low if low is not None else (H, W)
    x = (torch.randn(B, C, h, w_, generator=g) * scale).to(dtype).float()
    y = lc.make_labels(B, C, H, W, g)
    if blank_image is not None:
        y[blank_image] = IGNORE
    return x, y
