"""Exact-arithmetic data for the convolution kernels: ternary operands, float64 references, the conditions under which equality is owed.

Host only (torch on the CPU; nothing here touches the HIP library).  tests/test_conv_exact_cpu.py proves the design on the host,
tests/test_conv_exact_gpu.py holds the kernels of csrc/conv_*.hip to it.

The idea.  x, w, bias, gy, the addend are drawn from {-1, 0, +1} (the gate from {0, 1}).  Every operand is then exact in bf16, f16 and
fp32, every product is exact, and every partial sum -- in any order, on any MFMA path, in any split-K slab -- is an integer whose
magnitude is at most the sum of the magnitudes of the terms.  While that sum stays below 2^24 every partial sum is exact in fp32, so
the fp32 accumulators hold the true value whatever the order; the one rounding at the store is exact too when the value itself is an
integer of at most 256 (bf16: 8 significand bits), 2048 (f16: 11) or 2^24 (fp32).  The device result must then EQUAL the float64
reference: torch.equal, no tolerance, no dependence on a rounding mode.  The fused statistics sum y and y^2 in fp32 (and combine in
float64): exact while the per-channel sum of y^2 (which bounds the sum of |y|: integers) stays below 2^24.

The conditions are asserted on the REFERENCE, never on a device result (check_output / check_stats).  One data set serves the three
types, so it is drawn for the strictest one (bf16).  The nonzero density is 2/3; a case whose expected spread would break a condition
gets a lower one from pick_nz() -- a rule over the case's dimensions alone (sigma^2 = K * d_a * d_b for a sum of K products of operands
of densities d_a, d_b; 6.5 sigma against the bf16 limit, since the largest cases have 3e7 outputs; expected sum of y^2 = M * sigma^2
with a factor 1.5 of room).  The rule only has to be good enough: what decides is the assertion on the reference.

The sum of the magnitudes of the terms is the same convolution of |x| with |w|.  It is evaluated in fp32: partial sums of non-negative
integers grow monotonically, so an fp32 evaluation is either exact or has reached 2^24 -- in which case the assertion fails as it should.

The case lists are imported, not copied: tests/golden/conv_plan.json is keyed to them, and the suite has run every one of these shapes
on the GPU.
"""
import math

import torch
import torch.nn.functional as F

from test_conv_gpu import CASES, GROUP_CASES, C64_CASES, C128_CASES, PWK_CASES          # noqa: F401
from test_depthwise_gpu import CASES as _DW_TYPED_CASES
from test_lowrank_skip_gpu import KERNEL_CASES as LOWRANK_CASES                          # noqa: F401
import test_ops_gpu as _ops_gpu

# (B, C, N, H, W, dil, resize): the convolution -> nearest resize -> BatchNorm cases, read off the test that owns them
WSTAT_CASES = next(m.args[1] for m in _ops_gpu.test_batch_norm_behind_a_resize_takes_its_statistics_from_the_convolution_epilogue.pytestmark
                   if m.name == "parametrize" and m.args[0] == "case")

# the depthwise shape list without its dtype column (every geometry runs in all three types here), in first-seen order
DW_CASES = list(dict.fromkeys(c[:6] for c in _DW_TYPED_CASES))

LIMIT = {torch.bfloat16: 256, torch.float16: 2048, torch.float32: 1 << 24}
TWO24 = 1 << 24
DENOM = 48               # densities are nz / 48 with nz even: 32 (2/3), 16, 8, 4, 2
# rows of the [M][N] output one tile / strip / row block of the kernels covers (csrc/conv_igemm.hip, conv_pw.hip, conv_pwk.hip,
# conv_c64.hip), and the channel widths of their column blocks: the mismatch reporter prints positions modulo these
TILE_ROWS = (48, 64, 96, 128, 192, 256, 384)
TILE_COLS = (16, 32, 64, 128)


def sid(case):
    return "x".join(str(int(v)) if not isinstance(v, torch.dtype) else str(v)[6:] for v in case)


def dname(T):
    return {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}[T]


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def ternary(shape, nz, seed):
    """fp32 tensor of `shape` over {-1, 0, +1}: P(+1) = P(-1) = nz / 96.  Fixed seed -> fixed data."""
    assert nz % 2 == 0 and 2 <= nz <= DENOM
    g = torch.Generator().manual_seed(int(seed))
    r = torch.randint(0, DENOM, tuple(shape), generator=g, dtype=torch.int8)
    return (r < nz // 2).float() - ((r >= nz // 2) & (r < nz)).float()


def binary(shape, seed):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(0, 2, tuple(shape), generator=g, dtype=torch.uint8)


def pick_nz(K, M=0, nz_other=None, limit=256):
    """Largest density step nz (of 32, 16, 8, 4, 2) at which a sum of K products stays inside `limit` at 6.5 sigma and -- with M > 0,
    for an output whose statistics are taken -- M such outputs keep sum y^2 below 2^24 / 1.5.  nz_other: the density of the other
    operand when it is already fixed (None: both operands get this one)."""
    nz = 32
    while nz > 2:
        d, do = nz / DENOM, (nz_other if nz_other is not None else nz) / DENOM
        var = K * d * do
        if 6.5 * math.sqrt(var) <= limit and (M == 0 or 1.5 * M * var < TWO24):
            break
        nz //= 2
    return nz


def out_size(H, k, stride, pad, dil):
    return (H + 2 * pad - dil * (k - 1) - 1) // stride + 1


def conv_data(B, C, H, W, N, k, stride, pad, dil, has_bias, seed, stats=None):
    """-> dict(x, w, b, gy, nz=(x/w step, gy step)) for one dense convolution.  stats: whether the forward output's statistics are
    checked (default: the bias-free cases, as the library fuses them)."""
    Ho, Wo = out_size(H, k, stride, pad, dil), out_size(W, k, stride, pad, dil)
    if stats is None:
        stats = not has_bias
    M = stats if type(stats) is int else (B * Ho * Wo if stats else 0)        # (an int: the weighted element count behind a resize)
    nz = pick_nz(C * k * k, M)
    # the input gradient sums N * k * k / stride^2 products of gy and w (a dilation above the image leaves fewer: the bound holds)
    nzg = pick_nz(max(1, N * k * k // (stride * stride)), 0, nz_other=nz)
    x = ternary((B, C, H, W), nz, seed)
    w = ternary((N, C, k, k), nz, seed + 1)
    b = ternary((N,), 32, seed + 2) if has_bias else None
    gy = ternary((B, N, Ho, Wo), nzg, seed + 3)
    return dict(x=x, w=w, b=b, gy=gy, nz=(nz, nzg), geom=(stride, pad, dil))


def seed_of(case, salt=0):
    import zlib
    return (zlib.crc32(repr(tuple(str(v) for v in case)).encode()) + 7919 * salt) & 0x3FFFFFFF


def dense_data(case, salt=0):
    """conv_data for a (B, Cin, H, W, Cout, k, stride, pad, dil, bias) tuple of CASES"""
    B, C, H, W, N, k, st, pad, dil, hb = case
    return conv_data(B, C, H, W, N, k, st, pad, dil, hb, seed_of(case, salt))


def group_data(case, i):
    """problem i of a (B, Cin, H, W, Cout, k, stride, pad, dil, problems) tuple of GROUP_CASES: x and gy (weight gradients only)"""
    B, C, H, W, N, k, st, pad, dil, _n = case
    Ho, Wo = out_size(H, k, st, pad, dil), out_size(W, k, st, pad, dil)
    return ternary((B, C, H, W), 32, seed_of(case, 2 * i)), ternary((B, N, Ho, Wo), 32, seed_of(case, 2 * i + 1))


def c64_as_dense(case):
    B, C, H, W, N, dil, hb = case
    return (B, C, H, W, N, 3, 1, dil, dil, hb)


def pwk_as_dense(case):
    B, C, H, W, N = case
    return (B, C, H, W, N, 1, 1, 0, 1, False)


def c64_data(case, salt=0):
    """a (B, C, H, W, N, dil, bias) tuple of C64_CASES / C128_CASES: the dense data plus the addend of the dgrad form"""
    B, C, H, W, N, dil, hb = case
    d = dense_data(c64_as_dense(case), salt)
    d["addend"] = ternary((B, N, H, W), 32, seed_of(case, salt) + 4)
    return d


def pwk_data(case, salt=0):
    """a (B, C, H, W, N) tuple of PWK_CASES: the dense data, the addend and the bits of its gate"""
    B, C, H, W, N = case
    d = dense_data(pwk_as_dense(case), salt)
    d["addend"] = ternary((B, N, H, W), 32, seed_of(case, salt) + 4)
    d["gate_bits"] = torch.randint(0, 256, (B * H * W * N // 8,), generator=torch.Generator().manual_seed(seed_of(case, salt) + 5),
                                   dtype=torch.uint8)
    return d


def unpack_gate(bits, B, N, H, W):
    """bit e & 7 of byte e >> 3, e = m * N + n over the dense [M][N] tensor -> {0, 1} as [B,N,H,W]"""
    return ((bits.view(-1, 1) >> torch.arange(8, dtype=torch.uint8)) & 1).view(B, H, W, N).permute(0, 3, 1, 2)


def dw_data(case, salt=0):
    """(B, C, H, W, stride, dil) of the depthwise list -> x, w [C,1,3,3], b, gy"""
    B, C, H, W, s, d = case
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    sd = seed_of(case, salt)
    return dict(x=ternary((B, C, H, W), 32, sd), w=ternary((C, 1, 3, 3), 32, sd + 1), b=ternary((C,), 32, sd + 2),
                gy=ternary((B, C, Ho, Wo), 32, sd + 3), geom=(s, d, d))


# ---- float64 references -------------------------------------------------------------------------------------------------------------
def ref_forward(x, w, b=None, stride=1, pad=0, dil=1, relu=False, addend=None, gate=None, groups=1, relu6=False):
    """conv(x, w) + b + addend * gate, then the activation -- float64"""
    y = F.conv2d(x.double(), w.double(), b.double() if b is not None else None, stride, pad, dil, groups)
    if addend is not None:
        y = y + (addend.double() * gate.double() if gate is not None else addend.double())
    if relu6:
        y = y.clamp(0.0, 6.0)
    elif relu:
        y = y.clamp_min(0.0)
    return y


def mag_forward(x, w, b=None, stride=1, pad=0, dil=1, addend=None, groups=1):
    """the sum of the magnitudes of ref_forward's terms (fp32: see the module docstring)"""
    m = F.conv2d(x.abs().float(), w.abs().float(), b.abs().float() if b is not None else None, stride, pad, dil, groups)
    return m + addend.abs().float() if addend is not None else m


def ref_dgrad(xshape, w, gy, stride=1, pad=0, dil=1, addend=None, gate=None, groups=1):
    dx = torch.nn.grad.conv2d_input(tuple(xshape), w.double(), gy.double(), stride, pad, dil, groups)
    if addend is not None:
        dx = dx + (addend.double() * gate.double() if gate is not None else addend.double())
    return dx


def mag_dgrad(xshape, w, gy, stride=1, pad=0, dil=1, addend=None, groups=1):
    m = torch.nn.grad.conv2d_input(tuple(xshape), w.abs().float(), gy.abs().float(), stride, pad, dil, groups)
    return m + addend.abs().float() if addend is not None else m


def ref_wgrad(x, wshape, gy, stride=1, pad=0, dil=1, groups=1):
    return torch.nn.grad.conv2d_weight(x.double(), tuple(wshape), gy.double(), stride, pad, dil, groups)


def mag_wgrad(x, wshape, gy, stride=1, pad=0, dil=1, groups=1):
    return torch.nn.grad.conv2d_weight(x.abs().float(), tuple(wshape), gy.abs().float(), stride, pad, dil, groups)


def ref_dbias(gy):
    return gy.double().sum((0, 2, 3))


def ref_dbias_as_computed(gy):
    """The bias gradient as ops.channel_sums states it: NOT the plain sum.  channel_sums takes the column MEAN from the statistics pass
    and the BatchNorm finalize (csrc/stats.hip bn_finalize_kernel: the float64 sum of the partial rows divided by the count in float64,
    rounded to fp32) and multiplies it by the count in fp32.  No term is lost, but the quotient is rounded and the product is rounded
    again, so the result can miss the integer sum by an ulp (1.9e-6 at 27).  On exact data the sum itself is exact, so this expression
    is owed bit for bit: fp32(fp32(float64(sum) / n) * n)."""
    n = gy.shape[0] * gy.shape[2] * gy.shape[3]
    return (gy.double().sum((0, 2, 3)) / float(n)).float() * torch.tensor(float(n), dtype=torch.float32)


def big(shape_a, shape_b=()):
    """an activation of 2^24 elements or more: the cases whose type repetitions are dropped first to keep the GPU file short"""
    return max(math.prod(shape_a), math.prod(shape_b) if shape_b else 0) >= TWO24


def ref_stats(y, mult=None):
    """-> (per-image sum [B][N], per-image sum of squares [B][N]) of a float64 [B,N,H,W]; mult [H,W]: pixel multiplicities.  The
    per-channel totals are their sums over the images."""
    y = y.double()
    m = mult.double()[None, None] if mult is not None else 1.0
    return (y * m).sum((2, 3)), (y * y * m).sum((2, 3))


# ---- conditions (on the reference) --------------------------------------------------------------------------------------------------
def check_output(label, ref, mag, T=torch.bfloat16):
    """The reference is integer-valued, at most LIMIT[T] in magnitude, and its terms' magnitudes sum to less than 2^24."""
    assert bool((ref == ref.round()).all()), (label, "not integer-valued")
    top = float(ref.abs().max()) if ref.numel() else 0.0
    assert top <= LIMIT[T], (label, dname(T), "max|ref| = %g above %d: lower the density" % (top, LIMIT[T]))
    if mag is not None:
        mtop = float(mag.max()) if mag.numel() else 0.0
        assert mtop < TWO24, (label, "sum of |terms| = %g reaches 2^24" % mtop)
    return top


def check_terms(label, count):
    """The same bound without a convolution: on data of magnitude at most 1 the magnitudes of `count` terms sum to at most `count`."""
    assert count < TWO24, (label, count)


def check_stats(label, ref, mult=None):
    s, q = ref_stats(ref, mult)
    top = float(q.sum(0).max())
    assert top < TWO24, (label, "per-channel sum of ref^2 = %g reaches 2^24: lower the density" % top)
    return top


# ---- mismatch reporter --------------------------------------------------------------------------------------------------------------
def mismatch(label, got, want, first=8):
    """'' when got == want element for element (after conversion to float64 on the host), else a report: the count of differing
    elements and the first few as (b, channel, h, w, got, want) with the position modulo the kernels' tile sizes."""
    g, r = got.detach().double().cpu(), want.detach().double().cpu()
    if tuple(g.shape) != tuple(r.shape):
        return "%s: shape %s, reference %s" % (label, tuple(g.shape), tuple(r.shape))
    bad = ~((g == r) | (torch.isnan(g) & torch.isnan(r)))
    nbad = int(bad.sum())
    if nbad == 0:
        return ""
    lines = ["%s: %d of %d elements differ (largest |got - want| = %g)" % (label, nbad, g.numel(), float((g - r)[bad].abs().nan_to_num(float("inf")).max()))]
    idx = bad.nonzero()[:first].tolist()
    for ix in idx:
        gv, rv = float(g[tuple(ix)]), float(r[tuple(ix)])
        if len(ix) == 4:
            b, c, h, w = ix
            m = (b * g.shape[2] + h) * g.shape[3] + w
            lines.append("  (b %d, ch %d, h %d, w %d) got %g want %g | row m = %d, m mod %s = %s | ch mod %s = %s | h mod 2 = %d, w mod 2 = %d"
                         % (b, c, h, w, gv, rv, m, list(TILE_ROWS), [m % t for t in TILE_ROWS], list(TILE_COLS), [c % t for t in TILE_COLS],
                            h % 2, w % 2))
        else:
            lines.append("  %s got %g want %g" % (tuple(ix), gv, rv))
    return "\n".join(lines)


def assert_equal(label, got, want):
    """torch.equal on the values, with the report above when it fails"""
    msg = mismatch(label, got, want)
    assert msg == "", "\n" + msg


# ---- fp32 host evaluation in a scrambled order --------------------------------------------------------------------------------------
def _tap_view(xp, r, s, dil, stride, Ho, Wo):
    return xp[:, :, r * dil: r * dil + (Ho - 1) * stride + 1: stride, s * dil: s * dil + (Wo - 1) * stride + 1: stride]


def _chunks(n, parts, g):
    """`parts` contiguous ranges of a random permutation of range(n) (uneven), in a random order"""
    perm = torch.randperm(n, generator=g)
    cuts = sorted(set([0, n] + torch.randint(0, n + 1, (max(0, parts - 1),), generator=g).tolist()))
    out = [perm[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    return [out[i] for i in torch.randperm(len(out), generator=g).tolist()]


def scrambled_forward(x, w, b, stride, pad, dil, seed=0, parts=3):
    """conv(x, w) + b in fp32, one (tap, channel chunk) product at a time, taps and chunks in a random order, channels permuted"""
    g = torch.Generator().manual_seed(seed)
    N, C, R, S = w.shape
    Ho, Wo = out_size(x.shape[2], R, stride, pad, dil), out_size(x.shape[3], S, stride, pad, dil)
    xp = F.pad(x.float(), (pad, pad, pad, pad))
    acc = torch.zeros(x.shape[0], N, Ho, Wo)
    jobs = [(r, s, ch) for r in range(R) for s in range(S) for ch in _chunks(C, parts, g)]
    for j in torch.randperm(len(jobs), generator=g).tolist():
        r, s, ch = jobs[j]
        acc += torch.einsum("bchw,nc->bnhw", _tap_view(xp, r, s, dil, stride, Ho, Wo)[:, ch], w.float()[:, ch, r, s])
    return acc + b.float().view(1, -1, 1, 1) if b is not None else acc


def scrambled_dgrad(xshape, w, gy, stride, pad, dil, seed=0, parts=3):
    g = torch.Generator().manual_seed(seed)
    N, C, R, S = w.shape
    B, _, H, W = xshape
    Ho, Wo = gy.shape[2], gy.shape[3]
    acc = torch.zeros(B, C, H + 2 * pad, W + 2 * pad)
    jobs = [(r, s, ch) for r in range(R) for s in range(S) for ch in _chunks(N, parts, g)]
    for j in torch.randperm(len(jobs), generator=g).tolist():
        r, s, ch = jobs[j]
        _tap_view(acc, r, s, dil, stride, Ho, Wo).add_(torch.einsum("bnhw,nc->bchw", gy.float()[:, ch], w.float()[ch, :, r, s]))
    return acc[:, :, pad: pad + H, pad: pad + W]


def scrambled_wgrad(x, wshape, gy, stride, pad, dil, seed=0, parts=5):
    """split-K form: the pixels in `parts` slabs of a random permutation of the output rows of every image, summed in a random order"""
    g = torch.Generator().manual_seed(seed)
    N, C, R, S = wshape
    Ho, Wo = gy.shape[2], gy.shape[3]
    xp = F.pad(x.float(), (pad, pad, pad, pad))
    acc = torch.zeros(N, C, R, S)
    for rows in _chunks(Ho, parts, g):
        gs = gy.float()[:, :, rows]
        for r in range(R):
            for s in range(S):
                acc[:, :, r, s] += torch.einsum("bnhw,bchw->nc", gs, _tap_view(xp, r, s, dil, stride, Ho, Wo)[:, :, rows])
    return acc


def scrambled_dw(x, w, gy, stride, dil, seed=0):
    """depthwise 3x3 (padding = dilation): forward, dgrad and wgrad in fp32, taps in a random order, the weight gradient in row slabs"""
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = x.shape
    Ho, Wo = gy.shape[2], gy.shape[3]
    xp = F.pad(x.float(), (dil, dil, dil, dil))
    y, dxp, dw = torch.zeros(B, C, Ho, Wo), torch.zeros_like(xp), torch.zeros(C, 1, 3, 3)
    for t in torch.randperm(9, generator=g).tolist():
        r, s = divmod(t, 3)
        wt = w.float()[:, 0, r, s].view(1, C, 1, 1)
        y += _tap_view(xp, r, s, dil, stride, Ho, Wo) * wt
        _tap_view(dxp, r, s, dil, stride, Ho, Wo).add_(gy.float() * wt)
        for rows in _chunks(Ho, 3, g):
            dw[:, 0, r, s] += (gy.float()[:, :, rows] * _tap_view(xp, r, s, dil, stride, Ho, Wo)[:, :, rows]).sum((0, 2, 3))
    return y, dxp[:, :, dil: dil + H, dil: dil + W], dw


def lowrank_data(case, salt=0):
    """(B, C, H, W, N, dil) of the low-rank list: the 3x3 operands, the score gradient dp [B,32,H,W] and the classifier pack wf [N,32].
    The rank-32 product sums 32 products: dp at density 1/6 keeps it (and the convolution it is added to) inside the bf16 limit."""
    B, C, H, W, N, dil = case
    sd = seed_of(case, salt)
    d = conv_data(B, C, H, W, N, 3, 1, dil, dil, False, sd, stats=False)
    d["dp"], d["wf"] = ternary((B, 32, H, W), 8, sd + 6), ternary((N, 32), 32, sd + 7)
    return d


# ---- kernels that small shapes reach only behind a switch ---------------------------------------------------------------------------
# The switches are read once per process: one child process per switch set.  The switch sets and shape lists restate those of the
# *_in_subprocess tests of tests/test_conv_gpu.py, where they live inside the text of the child programs and cannot be imported.
def _d(B, Cin, H, W, Cout, k, pad, dil, st):
    return (B, Cin, H, W, Cout, k, st, pad, dil, False)


_ALT = [_d(*s) for s in [(2, 128, 240, 240, 256, 3, 1, 1, 1), (2, 304, 120, 120, 256, 3, 1, 1, 1), (3, 64, 33, 31, 64, 3, 1, 1, 1),
                         (2, 256, 48, 40, 512, 1, 0, 1, 1), (4, 128, 32, 32, 128, 3, 1, 1, 2), (4, 256, 32, 32, 512, 1, 0, 1, 2),
                         (2, 32, 20, 18, 256, 1, 0, 1, 1), (3, 32, 33, 31, 136, 1, 0, 1, 1), (2, 32, 96, 96, 256, 1, 0, 1, 1)]]
_RR = [(B, Cin, H, W, Cout, 3, 1, pad, pad, False) for (B, Cin, H, W, Cout, pad) in
       [(2, 128, 192, 192, 256, 1), (2, 64, 96, 96, 128, 1), (3, 256, 48, 48, 256, 1), (2, 128, 48, 48, 128, 2), (1, 64, 384, 384, 128, 1),
        (2, 64, 192, 384, 192, 1), (4, 64, 48, 16, 128, 1), (2, 192, 96, 192, 320, 1), (1, 64, 24, 32, 128, 2),
        (1, 128, 384, 384, 64, 1), (2, 64, 192, 192, 64, 1), (3, 64, 96, 96, 64, 2), (2, 64, 48, 48, 64, 1), (2, 128, 192, 192, 48, 1),
        (1, 64, 384, 384, 64, 2)]]
# (B, C, H, W, N, dil, problems, true channels, type)
_WG3 = [(2, 64, 16, 64, 64, 1, 1, 64, 'b'), (1, 64, 24, 128, 128, 1, 1, 64, 'b'), (2, 128, 12, 96, 128, 1, 3, 128, 'b'), (2, 64, 8, 48, 64, 1, 1, 64, 'b'),
        (2, 128, 16, 48, 256, 2, 2, 128, 'b'), (2, 64, 20, 64, 128, 2, 1, 64, 'h'), (2, 320, 12, 64, 256, 1, 1, 304, 'b'), (3, 64, 40, 192, 64, 1, 1, 64, 'b'),
        (5, 128, 40, 64, 128, 1, 7, 128, 'b'), (4, 256, 48, 48, 256, 1, 22, 256, 'b'), (2, 128, 24, 96, 64, 2, 2, 128, 'h'), (1, 64, 4, 144, 64, 1, 1, 64, 'b'),
        (2, 64, 8, 144, 128, 2, 1, 64, 'b'), (1, 128, 2, 64, 64, 1, 32, 128, 'b'), (4, 128, 48, 192, 128, 1, 5, 128, 'b'), (16, 64, 96, 192, 64, 1, 3, 64, 'b')]
# (B, C, H, W, N, problems, type)
_WG1 = [(2, 256, 8, 16, 256, 1, 'b'), (1, 512, 16, 16, 256, 3, 'b'), (2, 256, 12, 16, 1024, 5, 'b'), (4, 1024, 48, 48, 256, 22, 'b'), (2, 256, 10, 16, 256, 1, 'h'),
        (1, 2048, 8, 8, 512, 2, 'b'), (1, 256, 4, 8, 256, 1, 'b'), (4, 256, 48, 48, 1024, 23, 'b'), (2, 512, 24, 24, 2048, 3, 'h')]
# (B, C, H, W, N, k, stride, pad, dil, problems)
_BIG = [(4, 256, 48, 48, 1024, 1, 1, 0, 1, 5), (4, 1024, 48, 48, 256, 1, 1, 0, 1, 3), (4, 256, 48, 48, 256, 3, 1, 1, 1, 4), (3, 128, 33, 31, 256, 3, 2, 1, 1, 2),
        (2, 512, 24, 24, 512, 3, 1, 2, 2, 1), (2, 256, 40, 36, 256, 1, 1, 0, 1, 1), (2, 64, 96, 96, 256, 1, 1, 0, 1, 1)]

# name -> (kind, switches, shapes)
SWITCH_SETS = {
    "generic_on_pointwise": ("dense", {"MRFP_CONV_PW": "0", "MRFP_WGRAD_DENSE": "0"}, _ALT),
    "tile_96_rows": ("dense", {"MRFP_CONV_T96": "2", "MRFP_CONV_C64": "0"}, _ALT),
    "tile_192_rows": ("dense", {"MRFP_CONV_T192": "2", "MRFP_CONV_RR": "0", "MRFP_CONV_C64": "0"}, _ALT),
    "pointwise_k32_half": ("dense", {"MRFP_CONV_PW32": "1"}, _ALT),
    "row_reuse": ("dense", {"MRFP_CONV_RR": "3", "MRFP_CONV_C64": "0"}, _RR),
    "weight_stationary_128": ("c64", {"MRFP_CONV_C128": "2"}, C128_CASES),
    "wgrad_acc_stationary_3x3": ("wg3", {"MRFP_WGRAD3": "2"}, _WG3),
    "wgrad_acc_stationary_1x1": ("wg1", {"MRFP_WGRAD1": "2"}, _WG1),
    "wgrad_tile_256x128": ("big", {"MRFP_WGRAD_BIG": "2"}, _BIG),
}


def wgrad_child_case(kind, sh):
    """a shape of a weight-gradient child list -> ((B, C, H, W, N, k, stride, pad, dil, problems), true channels, type)"""
    types = {'b': torch.bfloat16, 'h': torch.float16}
    if kind == "wg3":
        B, C, H, W, N, dil, n, Ct, t = sh
        return (B, C, H, W, N, 3, 1, dil, dil, n), Ct, types[t]
    if kind == "wg1":
        B, C, H, W, N, n, t = sh
        return (B, C, H, W, N, 1, 1, 0, 1, n), C, types[t]
    assert kind == "big"
    return tuple(sh), sh[1], torch.bfloat16
