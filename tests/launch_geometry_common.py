"""The shapes of tests/test_launch_geometry_gpu.py and the launch path each was chosen for.

One table for both files: test_launch_geometry_cpu.py asks the library's host-only queries (mrfp_stats_nslab, mrfp_dwconv_nslab,
mrfp_dwconv_wgrad_ws_bytes, mrfp_ce_nblocks) whether every shape still takes that path, test_launch_geometry_gpu.py runs the kernels
at it.  A later change of a cap (csrc/common.hpp lines_per_image, csrc/conv_dw.hip dw_strips, csrc/loss.hip ce_blocks) then fails
the CPU file instead of quietly turning the GPU file back into single-line tests.

Row kernels (csrc/common.hpp): one workgroup per line while B * lines <= 2048, else workgroup j of an image walks lines j, j + ly,
...; 256 threads = colthreads x rowthreads over (channel vector, pixel), a row thread of the statistics / apply kernels takes four
pixels per trip, so one trip covers 4 * rowthreads pixels of a line.  The finalize kernels (csrc/stats.hip) sum the partial rows on
kFL = 128 lanes (BatchNorm: B * ly rows; InstanceNorm forward: ly rows per image) or kIL = 8 lanes per image (InstanceNorm
backward), four rows per lane per trip of the unrolled body, which runs only above 3 * lanes rows.
"""
import os

import torch

KFL, KIL = 128, 8                # csrc/stats.hip: partial lanes of reduce_partials / of in_bwd_finalize_kernel per image
ROW_CAP = 2048                   # csrc/common.hpp lines_per_image
CE_CAP, CE_THREADS = 2048, 256   # csrc/loss.hip ce_blocks, csrc/eval.hip

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

ROW_BLOCKS_ENV = "MRFP_ROW_BLOCKS"


def row_blocks_overridden():
    """MRFP_ROW_BLOCKS changes lines_per_image: none of the premises below would hold."""
    return os.environ.get(ROW_BLOCKS_ENV) is not None


SKIP_REASON = ROW_BLOCKS_ENV + " is set: it changes lines_per_image, the shapes of this file would take other launch paths"


def ceil_div(a, b):
    return -(-a // b)


def lanes(C, dtype):
    """(VEC, lpr, colthreads, rowthreads) of a row kernel: csrc/common.hpp pick_vec / make_lanes."""
    full = 16 // torch.empty((), dtype=dtype).element_size()
    vec = full if C % full == 0 else 1
    lpr = C // vec
    col = min(lpr, 256)
    return vec, lpr, col, 256 // col


# ---- 1. row kernels with many lines per workgroup -----------------------------------------------------------------------------
# name -> (shape, dtypes, expected workgroups per image, what the shape is for)
#   lines:   "multi" -- some workgroup walks >= 2 lines;  "single" -- every workgroup one line
#   uneven:  the workgroups of an image do not all walk the same number of lines
#   bn_body: B * ly > 3 * KFL  (reduce_partials of bn_finalize / bn_bwd_finalize runs its unrolled body)
#   in_body: ly > 3 * KFL      (in_finalize / plane_sum per image; then also ly > 3 * KIL for in_bwd_finalize)
ROW_SHAPES = {
    "two_lines_uneven": dict(shape=(16, 8, 161, 5), dtypes=(F32, BF16, F16), ly=81, lines="multi", uneven=True, bn_body=True,
                             in_body=False, lpr_over_256=False),
    "two_lines_c64": dict(shape=(24, 64, 130, 3), dtypes=(F32, BF16), ly=65, lines="multi", uneven=False, bn_body=True,
                          in_body=False, lpr_over_256=False),
    "scalar_c19": dict(shape=(2, 19, 1100, 3), dtypes=(F32, BF16), ly=550, lines="multi", uneven=False, bn_body=True,
                       in_body=True, lpr_over_256=False),
    "single_line_many_partials": dict(shape=(4, 16, 500, 4), dtypes=(F32, BF16), ly=500, lines="single", uneven=False,
                                      bn_body=True, in_body=True, lpr_over_256=False),
    "wide_c2048": dict(shape=(16, 2048, 140, 1), dtypes=(F32,), ly=70, lines="multi", uneven=False, bn_body=True,
                       in_body=False, lpr_over_256=True),
}

# HRFP stage: nearest resize -> BatchNorm -> ReLU; the row kernels walk the OUTPUT lines (statistics, apply) and the INPUT lines
# (backward apply).  (input shape, resize, output lines, workgroups per image over the output, ... over the input)
RESIZE_CASES = {
    "up_1.2": dict(shape=(16, 8, 135, 5), rs=dict(scale=1.2), Ho=162, ly_out=81, ly_in=68),
    "down_0.838": dict(shape=(16, 8, 193, 6), rs=dict(scale=0.838), Ho=161, ly_out=81, ly_in=97),
}

# bilinear: forward walks output lines, backward input lines
BILINEAR_CASES = {
    "up": dict(shape=(16, 8, 70, 5), size=(161, 9), ly_fwd=81, ly_bwd=70),
    "down": dict(shape=(16, 8, 161, 9), size=(70, 5), ly_fwd=70, ly_bwd=81),
}

# max pool 3x3 / stride 2: forward walks the Ho = (H - 1) // 2 + 1 output lines, backward (and both passes of the fused
# InstanceNorm + ReLU + pool backward) the H input lines
POOL_SHAPES = {
    "c8": dict(shape=(16, 8, 321, 5), ly_fwd=81, ly_bwd=107),              # 2 lines (uneven) forward, 3 lines backward
    "c64": dict(shape=(24, 64, 261, 3), ly_fwd=66, ly_bwd=66),             # Ho = 131: 2 lines (uneven); H = 261: 4 lines (uneven)
    "c19_scalar": dict(shape=(2, 19, 2201, 3), ly_fwd=551, ly_bwd=734),    # Ho = 1101: 2 lines; H = 2201: 3 lines
}

# ---- 2. lines longer than one trip of the row threads ---------------------------------------------------------------------------
# (shape, dtype, pixels per trip = 4 * rowthreads, rest of the line behind the full trips, some row threads idle in the last trip)
TRIP_CASES = {
    "c64_bf16": dict(shape=(2, 64, 3, 150), dtype=BF16, trip=128, full=1, rest=22, idle_threads=True),
    "c8_bf16": dict(shape=(1, 8, 2, 1100), dtype=BF16, trip=1024, full=1, rest=76, idle_threads=True),
    "c8_f32": dict(shape=(1, 8, 2, 700), dtype=F32, trip=512, full=1, rest=188, idle_threads=False),
}

# ---- 3. depthwise 3x3 with multi-row strips -------------------------------------------------------------------------------------
# per (stride): strips of the forward / weight-gradient launch over the Ho output rows and of the dgrad launch over the H input rows
#   fwd / wg / dg = (strips per image, rows per strip, rows of the last strip)
DW_CASES = {
    "c960_f32": dict(B=8, C=960, H=41, W=3, dtypes=(F32,), nchunk=8,
                     s1=dict(fwd=(21, 2, 1), wg=(14, 3, 2), dg=(21, 2, 1)),
                     s2=dict(fwd=(21, 1, 1), wg=(11, 2, 1), dg=(21, 2, 1))),      # (Ho = 21 <= 32: the forward is single-row at stride 2)
    "c960_f32_tall": dict(B=8, C=960, H=83, W=3, dtypes=(F32,), nchunk=8,         # ... so a taller one for the strided forward
                          s1=dict(fwd=(28, 3, 2), wg=(14, 6, 5), dg=(28, 3, 2)),
                          s2=dict(fwd=(21, 2, 2), wg=(14, 3, 3), dg=(28, 3, 2))),
    "c96_16bit": dict(B=16, C=96, H=300, W=2, dtypes=(BF16, F16), nchunk=1,
                      s1=dict(fwd=(100, 3, 3), wg=(60, 5, 5), dg=(100, 3, 3)),
                      s2=dict(fwd=(75, 2, 2), wg=(50, 3, 3), dg=(100, 3, 3))),
    "c12_padded": dict(B=16, C=12, H=301, W=2, dtypes=(BF16,), nchunk=1,           # Cp = 16 > C: pad-channel zeroing in a multi-row strip
                       s1=dict(fwd=(101, 3, 1), wg=(61, 5, 1), dg=(101, 3, 1)),
                       s2=dict(fwd=(76, 2, 1), wg=(51, 3, 1), dg=(101, 3, 1))),
}
DW_STATS_CASE = ("c96_16bit", 2)       # the fused-statistics repeat: 75 strips of 2 rows over Ho = 150, B * nslab = 1200 rows


def dw_pitch(C, dtype):
    epc = 16 // torch.empty((), dtype=dtype).element_size()
    return ceil_div(C, epc) * epc


# ---- 4. loss / evaluation kernels above the grid cap ------------------------------------------------------------------------------
CE_CASE = dict(B=1, C=19, H=725, W=725)                        # 525 625 pixels > 2048 * 256 = 524 288; 525 625 % 256 = 57
UPCE_CASE = dict(B=1, C=19, ld=32, Hi=182, Wi=182, H=725, W=725)
