"""Shared by test_relaxed_cpu.py and test_relaxed_gpu.py: restatements of boundary label relaxation and of the joint-weighted
soft-NLL loss, written from the definitions in include/mrfp_hip.h, and the seeded inputs of their tests.

  np_relax        translation-and-OR in numpy: the relaxed word of a pixel is the OR of 1 << t over its window, t = the label if it
                  is a class, else C; outside the image 1 << C; a strict class keeps its own bit
  np_counts / np_weights   per-image bit counts and the class-weight rule in float64, rounded once to float32
  ref_loss        the loss in float64 torch in the PUBLISHED shape -- log(max(softmax, multihot * sum(softmax * multihot))) summed
                  over the multi-hot with the class weights, -1/k in front, divided by valid + 1, looped per image -- so that the
                  closed form the kernels compute (closed_form below) is a checked claim; gradients come from autograd
"""
import os

import numpy as np
import torch

IGNORE = 255
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relaxed.npz")
GOLDEN_C = 19
GOLDEN_MAPS = ("blocky", "lines", "edges", "all255")
GOLDEN_BORDERS = (0, 1, 2)
GOLDEN_STRICT = {"none": None, "s5_11": [5, 11]}


def class_words(t, C):
    """1 << label for a class, 1 << C for everything else, uint32."""
    t = np.asarray(t).astype(np.int64)
    return np.left_shift(np.uint32(1), np.where((t >= 0) & (t < C), t, C).astype(np.uint32)).astype(np.uint32)


def np_relax(t, C, border, strict=None):
    """t: integer label maps [..., H, W] -> int32 words of the same shape."""
    own = class_words(t, C)
    H, W = own.shape[-2:]
    r = int(border)
    pad = np.full(own.shape[:-2] + (H + 2 * r, W + 2 * r), np.uint32(1) << np.uint32(C), dtype=np.uint32)
    pad[..., r:r + H, r:r + W] = own
    out = np.zeros_like(own)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= pad[..., dy:dy + H, dx:dx + W]          # the map translated by (dy - r, dx - r), constant fill
    mask = np.uint32(sum(1 << int(c) for c in (strict or ())))
    out = np.where((own & mask) != 0, own, out)
    return out.astype(np.uint32).view(np.int32)


def unpack(words, C, set_value=1):
    """int32 words [..., H, W] -> uint8 multi-hot [..., C+1, H, W] (the reference's layout), set bytes = set_value."""
    w = np.asarray(words).view(np.uint32)
    bits = np.arange(C + 1, dtype=np.uint32).reshape((-1, 1, 1))
    return (((w[..., None, :, :] >> bits) & 1) * set_value).astype(np.uint8)


def np_counts(words, C):
    """int32 words [B,H,W] -> int64 [B, C+1]: pixels of each image with each bit set."""
    return unpack(words, C).astype(np.int64).sum((-2, -1))


def np_weights(counts, upper_bound, norm, batch):
    """f_c = n_c / sum_{c=0..C} n_c in float64; 1 + ub (1 - f_c), or 1 + ub / f_c (norm); 1 where n_c == 0; one rounding to float32.
    -> [B, C], or [C] from the pooled counts (batch)."""
    n = np.asarray(counts, dtype=np.int64)
    rows = n.sum(0, keepdims=True) if batch else n
    out = []
    for r in rows:
        total = np.float64(r.sum())
        nc = r[:-1].astype(np.float64)
        w = np.ones(len(nc), dtype=np.float64)
        nz = nc > 0
        f = nc[nz] / total
        w[nz] = 1.0 + upper_bound / f if norm else 1.0 + upper_bound * (1.0 - f)
        out.append(w)
    out = np.stack(out).astype(np.float32)
    return out[0] if batch else out


def _rows(w, B, C):
    if w is None:
        w = torch.ones(C, dtype=torch.float64)
    w = w.double()
    return w.expand(B, C) if w.dim() == 1 else w


def ref_loss(logits, words, C, w=None):
    """logits float64 [B,C,H,W] (may require grad; on any device), words int32 [B,H,W] (numpy), w float64 [C] / [B,C] / None."""
    words = np.asarray(words)
    B = logits.shape[0]
    w = _rows(w, B, C).to(logits.device)
    total = 0.0
    for b in range(B):
        mh = torch.from_numpy(unpack(words[b], C)[:C].astype(np.float64)).to(logits.device)      # [C,H,W], the ignore plane dropped
        p = torch.softmax(logits[b], 0)
        q = (p * mh).sum(0, keepdim=True)
        term = torch.log(torch.max(p, mh * q))                                      # the published customsoftmax
        k = mh.sum(0)
        valid = k > 0
        per_pixel = -(mh * w[b].view(C, 1, 1) * term).sum(0) / torch.where(valid, k, torch.ones_like(k))
        total = total + (per_pixel * valid).sum() / (valid.sum() + 1)
    return total


def closed_form(logits, words, C, w=None):
    """What the kernels compute: l_i = (W_i / k_i) (lse_all(z_i) - lse_{S_i}(z_i)), L = sum_b sum_valid l_i / (valid_b + 1)."""
    words = np.asarray(words)
    B = logits.shape[0]
    w = _rows(w, B, C)
    total = 0.0
    for b in range(B):
        mh = torch.from_numpy(unpack(words[b], C)[:C].astype(bool))
        k = mh.sum(0)
        valid = k > 0
        z = logits[b]
        lse_all = torch.logsumexp(z, 0)
        lse_set = torch.logsumexp(torch.where(mh, z, torch.full_like(z, -float("inf"))), 0)
        W = (mh * w[b].view(C, 1, 1)).sum(0)
        li = torch.where(valid, W / k.clamp_min(1) * (lse_all - torch.where(valid, lse_set, torch.zeros_like(lse_set))),
                         torch.zeros_like(lse_all))
        total = total + li.sum() / (valid.sum() + 1)
    return total


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------
def make_label_maps(B, H, W, C, seed, all_ignored_image=None, cell=(5, 7)):
    """Blocky int64 label maps [B,H,W]: random classes in cells of `cell` pixels; ~6 % of the pixels 255 and, in an image of at least
    6 x 6, the 4 x 4 corner block (its core stays ignored after relaxation by 1 or 2); a few -1 and C (ignored by the kernels); a full
    row / column of 255 on row 32 / column 64 (the tile seams of mrfp_relax_labels) where the image has one; class C-1 absent (C > 2)."""
    g = torch.Generator().manual_seed(seed)
    ch, cw = (H + cell[0] - 1) // cell[0], (W + cell[1] - 1) // cell[1]
    coarse = torch.randint(0, C - 1 if C > 2 else C, (B, ch, cw), generator=g)
    y = coarse.repeat_interleave(cell[0], 1).repeat_interleave(cell[1], 2)[:, :H, :W].contiguous()
    y[torch.rand(B, H, W, generator=g) < 0.06] = IGNORE
    if H >= 6 and W >= 6:
        y[:, :4, :4] = IGNORE
    flat = y.view(-1)
    if flat.numel() >= 8:
        flat[int(torch.randint(0, flat.numel(), (1,), generator=g))] = -1
        flat[int(torch.randint(0, flat.numel(), (1,), generator=g))] = C
    if H > 32:
        y[:, 32, :] = IGNORE
    if W > 64:
        y[:, :, 64] = IGNORE
    if all_ignored_image is not None:
        y[all_ignored_image] = IGNORE
    return y


def make_logits(B, C, H, W, dtype, seed, scale=3.0):
    """float32 logits rounded to `dtype` first."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, C, H, W, generator=g) * scale).to(dtype).float()


def make_weights(C, seed, rows=None):
    """uniform in [0.5, 1.5], one class exactly 0 (row r of a per-image table: class r % C)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand((C,) if rows is None else (rows, C), generator=g) + 0.5
    if rows is None:
        w[0] = 0.0
    else:
        for r in range(rows):
            w[r, r % C] = 0.0
    return w


def golden():
    return np.load(GOLDEN)


def golden_key(name, border, strict):
    return "%s_b%d_%s" % (name, border, strict)
