"""Plain-torch fp64 restatement of the test-time-augmentation accumulator (ops.prob_accum / harness.evaluate_tta) and the shared
inputs of its tests.  The reference scores single-scale only, so the yardstick is this restatement: F.interpolate(mode="bilinear",
align_corners=True) in float64, torch.flip, softmax(dim=1), weighted sums into an fp64 accumulator.  The window grid and the
destination rectangles are host arithmetic and come from harness (tests/test_eval_tta_cpu.py pins them on hand-written cases)."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -23          # fp32 unit in the last place at 1.0: the unit of the accumulator tolerance


def accum_restated(logits, nc, acc, cnt, rect=None, flip=False, weight=1.0, dtype=torch.float64):
    """acc[B,H,W,nc] / cnt[B,H,W] (tensors of `dtype` on the host, updated in place) += one variant.  logits: [B,ld,hs,ws]
    (any storage), only channels 0..nc-1 are read; they are taken as they are (already rounded to the device's input format)."""
    B, H, W, _ = acc.shape
    y0, x0, hd, wd = (0, 0, H, W) if rect is None else rect
    z = logits.detach().cpu()[:, :nc].to(dtype)
    if flip:
        z = torch.flip(z, dims=(3,))
    z = F.interpolate(z, size=(hd, wd), mode="bilinear", align_corners=True)
    p = torch.softmax(z, dim=1).permute(0, 2, 3, 1)
    acc[:, y0:y0 + hd, x0:x0 + wd, :] += weight * p
    cnt[:, y0:y0 + hd, x0:x0 + wd] += weight
    return acc, cnt


def nhwc_logits(B, ld, hs, ws, dtype, seed, scale=3.0):
    """3 * randn class scores [B,ld,hs,ws] in NHWC storage, rounded to `dtype` (host tensor)."""
    g = torch.Generator().manual_seed(seed)
    z = (scale * torch.randn(B, hs, ws, ld, generator=g)).to(dtype)
    return z.permute(0, 3, 1, 2)          # logical NCHW over NHWC storage = channels_last


def hist_from_acc(acc, label, nc):
    """np.argmax (first maximum) + metrics.fast_hist of an accumulator on the host -> (hist, pred)."""
    from mrfp_amd import metrics
    a = acc.detach().cpu().numpy()
    pred = np.argmax(a, axis=-1)
    lab = label.detach().cpu().numpy()
    return metrics.fast_hist(pred.reshape(-1), lab.reshape(-1), nc), pred


def top2_gap(acc, cnt):
    """(best - second best averaged probability) per pixel of an fp64 restatement accumulator: acc / cnt."""
    top = torch.topk(acc, 2, dim=-1).values
    return (top[..., 0] - top[..., 1]) / cnt


# kernel-vs-restatement cases of the GPU test: (B, NC, ld, hs, ws, H, W, list of (rect, flip, weight)) -- ws = 1, odd sizes, hd not a
# multiple of anything, rectangles touching every border, overlapping rectangles (accumulation), B = 1 and 3
ACCUM_CASES = [
    ("nc19_ld19_borders", 1, 19, 19, 7, 9, 37, 53, [((0, 0, 29, 41), False, 1.0), ((8, 12, 29, 41), True, 0.5),
                                                       ((0, 12, 37, 41), True, 1.0), ((8, 0, 29, 53), False, 2.0)]),
    ("nc19_ld24_b3", 3, 19, 24, 11, 13, 45, 50, [(None, False, 1.0), ((3, 5, 41, 43), True, 1.0), ((44, 0, 1, 50), False, 0.25)]),
    ("nc19_ld32_wide", 1, 19, 32, 24, 80, 96, 320, [(None, False, 1.0), (None, True, 1.0), ((0, 63, 96, 257), True, 1.0)]),
    ("nc19_ws1", 1, 19, 32, 5, 1, 23, 17, [(None, False, 1.0), ((1, 16, 21, 1), True, 1.0)]),
    ("nc19_hs1_same", 3, 19, 19, 1, 31, 1, 31, [(None, True, 1.0), (None, False, 1.5)]),
    ("nc2", 3, 2, 8, 6, 7, 19, 301, [(None, False, 1.0), ((2, 1, 17, 299), True, 0.75)]),
    ("nc32", 1, 32, 32, 9, 10, 33, 47, [(None, True, 1.0), ((0, 0, 33, 47), False, 1.0), ((5, 7, 20, 40), True, 3.0)]),
]
