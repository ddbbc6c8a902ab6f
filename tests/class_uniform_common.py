"""Class-uniform sampling restated in numpy and plain Python: what tests/test_class_uniform_cpu.py and tests/test_class_uniform_gpu.py
compare mrfp_tile_class_sums, ClassUniformSampler, TrainTransform.draw(centroid=) and harness.train_batches with.

  tile_sums_np       the rule of include/mrfp_hip.h: per tile and class n, sum(x - x0), sum(y - y0) and the integer division
  scipy_centroid     int(scipy.ndimage.center_of_mass(patch == c)) + offset, the published form, for the CPU cross-check
  epoch_np / pick_np the sampler
  parent_draw        TrainTransform.draw as it was before it took a centroid, statement for statement (recorded before the class
                     was touched): what centroid=None must keep giving
  centroid_draw      the same with the centroid branch of dataloaders.py:424-425, 313-322 and this build's mirror rule
  golden_templates   the cases tests/golden/make_golden_class_uniform.py records (sizes, crop, scale range, centroid)
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "class_uniform.npz")
JITTER = dict(brightness=0.5, hue=0.3, contrast=0.2, saturation=0.2)          # main.py:413


# ---- the tile rule -----------------------------------------------------------------------------------------------------------
def tile_count(size, tile, partial):
    return -(-size // tile) if partial else size // tile


def tile_sums_np(lab, C, tile, table=None, partial=False):
    """lab uint8 [B,H,W] -> (sums int64 [B,nty,ntx,C,3], cent int32 [B,nty,ntx,C,2]); Python integers, so nothing can wrap."""
    lab = np.asarray(lab)
    if lab.ndim == 2:
        lab = lab[None]
    v = np.asarray(table, dtype=np.uint8)[lab] if table is not None else lab
    B, H, W = v.shape
    nty, ntx = tile_count(H, tile, partial), tile_count(W, tile, partial)
    sums = np.zeros((B, nty, ntx, C, 3), dtype=np.int64)
    cent = np.full((B, nty, ntx, C, 2), -1, dtype=np.int32)
    for b in range(B):
        for ty in range(nty):
            for tx in range(ntx):
                y0, x0 = ty * tile, tx * tile
                patch = v[b, y0:y0 + tile, x0:x0 + tile]
                for c in np.unique(patch).tolist():
                    if c >= C:
                        continue
                    ys, xs = np.nonzero(patch == c)
                    n, sx, sy = int(len(xs)), int(xs.astype(np.int64).sum()), int(ys.astype(np.int64).sum())
                    sums[b, ty, tx, c] = (n, sx, sy)
                    cent[b, ty, tx, c] = (x0 + sx // n, y0 + sy // n)
    return sums, cent


def tile_sums_big_np(lab, C, tile, table=None, partial=False):
    """tile_sums_np for maps with very many tiles (the capped-grid case): vectorised with bincount over (tile, class)."""
    lab = np.asarray(lab)
    v = (np.asarray(table, dtype=np.uint8)[lab] if table is not None else lab).astype(np.int64)
    B, H, W = v.shape
    nty, ntx = tile_count(H, tile, partial), tile_count(W, tile, partial)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ty, tx = yy // tile, xx // tile
    keep = (ty < nty) & (tx < ntx)
    sums = np.zeros((B, nty, ntx, C, 3), dtype=np.int64)
    for b in range(B):
        m = keep & (v[b] < C)
        key = ((ty[m] * ntx + tx[m]) * C + v[b][m])
        for k, wgt in enumerate((None, (xx - tx * tile)[m], (yy - ty * tile)[m])):
            sums[b, ..., k] = np.bincount(key, weights=wgt, minlength=nty * ntx * C).astype(np.int64).reshape(nty, ntx, C)
    n = sums[..., 0]
    x0 = (np.arange(ntx) * tile)[None, None, :, None]
    y0 = (np.arange(nty) * tile)[None, :, None, None]
    safe = np.maximum(n, 1)
    cent = np.stack([np.where(n > 0, x0 + sums[..., 1] // safe, -1), np.where(n > 0, y0 + sums[..., 2] // safe, -1)], -1).astype(np.int32)
    return sums, cent


def scipy_centroid(patch, c, x0=0, y0=0):
    """The published form: center_of_mass of the class mask (float64), int() of each coordinate, plus the tile offset -> (cx, cy)."""
    from scipy import ndimage
    cy, cx = ndimage.center_of_mass(patch == c)
    return int(cx) + x0, int(cy) + y0


# ---- the sampler ---------------------------------------------------------------------------------------------------------------
def pick_np(alist, k, np_rng):
    idx = np.arange(len(alist))
    np_rng.shuffle(idx)
    return [alist[int(idx[i % len(alist)])] for i in range(k)]


def epoch_np(n_images, by_class, pct, np_rng, shuffle=True):
    C = len(by_class)
    per_class = int(n_images * pct / C)
    n_rand = n_images - per_class * C
    items = [(i, None, None) for i in pick_np(range(n_images), n_rand, np_rng)]
    for c in range(C):
        if by_class[c]:
            items += [(i, cen, c) for i, cen in pick_np(by_class[c], per_class, np_rng)]
    if shuffle:
        np_rng.shuffle(items)
    return items, per_class, n_rand


# ---- the draw ------------------------------------------------------------------------------------------------------------------
def _jitter_draw(rng, np_rng):
    if rng.random() < 0.5:
        j = JITTER
        ops = [("brightness", float(np_rng.uniform(max(0, 1 - j["brightness"]), 1 + j["brightness"]))),
               ("contrast", float(np_rng.uniform(max(0, 1 - j["contrast"]), 1 + j["contrast"]))),
               ("saturation", float(np_rng.uniform(max(0, 1 - j["saturation"]), 1 + j["saturation"]))),
               ("hue", float(np_rng.uniform(-j["hue"], j["hue"])))]
        np_rng.shuffle(ops)
        return ops
    return None


def parent_draw(t, smin, smax, w, h, rng, np_rng):
    """-> (flip, jitter, (sw, sh), (pad_w, pad_h), (x1, y1), blur): TrainTransform.draw of the parent commit."""
    flip = rng.random() < 0.5
    jitter = _jitter_draw(rng, np_rng)
    scale_amt = 1.0 * rng.uniform(smin, smax)
    sw, sh = int(w * scale_amt), int(h * scale_amt)
    pad_w = pad_h = 0
    x1 = y1 = 0
    if not (sw == t and sh == t):
        pad_h = (t - sh) // 2 + 1 if t > sh else 0
        pad_w = (t - sw) // 2 + 1 if t > sw else 0
        W2, H2 = sw + 2 * pad_w, sh + 2 * pad_h
        x1 = 0 if W2 == t else rng.randint(0, W2 - t)
        y1 = 0 if H2 == t else rng.randint(0, H2 - t)
    blur = rng.random() if rng.random() < 0.5 else None
    return flip, jitter, (sw, sh), (pad_w, pad_h), (x1, y1), blur


def centroid_draw(t, smin, smax, w, h, rng, np_rng, centroid):
    """-> parent_draw's tuple + (the scaled, mirrored centroid,): dataloaders.py:424-425 (the centroid scaled with the size), :313-322
    (randint(c - t, c), clipped; two draws, always, past the early return), the centroid not moved by the padding; mirrored
    (w - 1 - c_x) when the flip fired."""
    flip = rng.random() < 0.5
    jitter = _jitter_draw(rng, np_rng)
    scale_amt = 1.0 * rng.uniform(smin, smax)
    sw, sh = int(w * scale_amt), int(h * scale_amt)
    c_x, c_y = centroid
    if flip:
        c_x = w - 1 - c_x
    c_x, c_y = [int(c * scale_amt) for c in (c_x, c_y)]
    pad_w = pad_h = 0
    x1 = y1 = 0
    if not (sw == t and sh == t):
        pad_h = (t - sh) // 2 + 1 if t > sh else 0
        pad_w = (t - sw) // 2 + 1 if t > sw else 0
        W2, H2 = sw + 2 * pad_w, sh + 2 * pad_h
        x1 = rng.randint(c_x - t, c_x)
        x1 = min(W2 - t, max(0, x1))
        y1 = rng.randint(c_y - t, c_y)
        y1 = min(H2 - t, max(0, y1))
    blur = rng.random() if rng.random() < 0.5 else None
    return flip, jitter, (sw, sh), (pad_w, pad_h), (x1, y1), blur, (c_x, c_y)


def draw_tuple(d):
    """A mrfp_amd.input_pipeline.Draw as parent_draw's tuple."""
    return d.flip, d.jitter, tuple(d.scaled), tuple(d.pad), tuple(d.crop), d.blur


# ---- the golden cases ----------------------------------------------------------------------------------------------------------
GOLDEN_CROP = 16
GOLDEN_SIZES = ((40, 24), (24, 20), (24, 40), (16, 16))      # (w, h); the last one with scale 1: the early return


def golden_templates():
    """[(size index, smin, smax, (c_x, c_y))]: 40 cases over four source sizes and five centroid positions each, corners included."""
    out = []
    for k in range(40):
        si = k % 4
        w, h = GOLDEN_SIZES[si]
        cen = ((0, 0), (w - 1, h - 1), (w - 1, 0), (w // 2, h // 2), (3, h - 2))[(k // 4) % 5]
        smin, smax = (1.0, 1.0) if si == 3 and k % 8 == 3 else (0.5, 2.0)
        out.append((si, smin, smax, cen))
    return out


def golden_source(si):
    """The seeded source pair of size GOLDEN_SIZES[si]: uint8 [h,w,3] and a blocky uint8 label map [h,w] (classes 0..18, some 255)."""
    w, h = GOLDEN_SIZES[si]
    g = np.random.default_rng(7000 + si)
    img = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    lab = np.repeat(np.repeat(g.integers(0, 19, ((h + 3) // 4, (w + 3) // 4), dtype=np.uint8), 4, 0), 4, 1)[:h, :w].copy()
    lab[g.random((h, w)) < 0.04] = 255
    return img, lab


def load_golden():
    return np.load(GOLDEN)


# ---- the GPU cases of the operator (tests/test_class_uniform_gpu.py) ---------------------------------------------------------------
def ragged_map():
    """B=2, 13 x 21, labels from {0..4, 7, 255}; row 12 and column 20 -- outside every whole 4 x 4 tile -- carry class 4, which occurs
    nowhere else."""
    g = np.random.default_rng(11)
    lab = g.choice(np.array([0, 1, 2, 3, 7, 255], dtype=np.uint8), size=(2, 13, 21))
    lab[:, 12, :] = 4
    lab[:, :, 20] = 4
    return lab
