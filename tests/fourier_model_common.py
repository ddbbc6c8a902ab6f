"""Per-element model of the Fourier amplitude mix (csrc/fft.hip): designed inputs, float64 reference, metric, emulations, cases.

Host only (torch on the CPU; nothing here imports the HIP library).  tests/test_fourier_model_cpu.py proves the model on the host,
tests/test_fourier_exact_gpu.py holds every kernel route of mrfp_fourier_mix to it.

Designed inputs.  On random data the operator is ill-conditioned: where a plane's own amplitude |F| is small the ratio
((1 - lam) |F| + lam |F'|) / |F| reaches 10^2..10^3 and multiplies the rounding error of F; no per-element bound holds.  So the
spectrum is designed: phases of rfft2 of a real white-noise plane (Hermitian-consistent by construction), amplitudes uniform in
[1, 2] sqrt(H W) (symmetrised on the self-mirrored columns kw = 0 and kw = W / 2), x = irfft2 in float64, THEN rounded to the
activation type T before either side sees it.  After the rounding every |F| is still >= 0.9 sqrt(H W) and <= 2.1 sqrt(H W)
(asserted per case, check_conditioning), so every ratio lies in [1 - lam + lam 0.9 / 2.1, 1 - lam + lam 2.1 / 0.9]: a case that
drifts into the ill-conditioned regime fails instead of passing loosely.  The upstream gradient is plain noise rounded to T (the
backward loads the saved ratio: it is as well conditioned as the ratio).

Reference.  The definition in float64 (torch.fft): band min(kh, H - kh)^2 + kw^2 <= r^2 or its complement, ratio 1 where
|F| <= 1e-20, dx from float64 autograd with the ratio detached.

Metric, per element:   scaled = |got - ref| / (u_T |ref| + 2^-24 A1[b, c])
u_T the unit roundoff of the output type (2^-8 bf16, 2^-11 f16, 2^-24 fp32: the constants of rounding_model_common), A1[b, c] =
(1 / H W) sum_bins w_k |F ratio| the largest value a pixel of that plane could take (w_k = 2 for the bins of the half spectrum that
have a mirror, 1 on the self-mirrored columns).  explain() names plane, pixel and the BIN THAT CARRIES THE ERROR -- the arg-max of
|rfft2(got - ref)| -- which tells a lost bin from a wrong twiddle from a mirror error.

Constants.  Per (type, arithmetic class) the bound is 2 x the largest scaled value the honest CPU emulation of that class reaches
over all cases of the table, rounded up to an integer; the factor 2 covers the summation order and the sqrt(log N) growth of an
fp32 FFT, which torch's FFT on the host does not share with the device.  Class "fp32" (FFT passes and the direct sum): the definition
in float32, output rounded to T.  Class "split" (the matrix-core row passes, bf16): the band-limited form y = x + irfft2(F (ratio -
1)) with both row passes as matrix products of split-bf16 factors -- forward x (exact in bf16) times hi + lo of the trigonometric
matrix, inverse hi*hi + lo*hi + hi*lo of the column results and the scaled trigonometric matrix, fp32 accumulation -- as the
comments of dft_rows_fwd_mfma_kernel / dft_rows_inv_mfma_kernel state it.

    type, class       largest scaled value of the emulation     bound
    ---------------   -------------------------------------     -----
    float32, fp32                    0.938                        2
    bfloat16, fp32                   0.996                        2
    float16, fp32                    0.997                        2
    bfloat16, split                  1.417                        3

(The 16-bit values of the fp32 class are the one rounding to T: u_T |ref| of the denominator.  The fp32 maximum is the smallest
plane, 8 x 8, where A1 -- a sum over 64 bins -- is closest to the pixels' own magnitude.)

test_fourier_model_cpu.py re-measures the table and fails when a value has outgrown its record.
"""
import math
from collections import namedtuple
from functools import lru_cache

import torch

from rounding_model_common import BF16, F16, F32, F64, U, U32, dname, relerr  # noqa: F401

UT = {F32: U32, BF16: U[BF16], F16: U[F16]}
LENS = (32, 48, 64, 96, 128, 192, 256, 384, 512)                      # the two-step plans of csrc/fft.hip
GEN_LENS = (8, 12, 18, 24, 36, 54, 72, 108, 144, 162, 216, 288, 432, 486)
GENERIC, TWOSTEP, PAIR, DIRECT, MFMA = range(5)                       # MRFP_FOURIER_ROUTE_* of include/mrfp_hip.h
ROUTE_NAMES = ("generic", "two-step", "pair", "direct", "mfma")
AMP_LO, AMP_HI = 0.9, 2.1                                             # of sqrt(H W): what a designed plane keeps after rounding to T

# largest scaled value of the honest emulation over all cases (test_fourier_model_cpu.py::test_emulation_table_is_current)
MEASURED = {(F32, "fp32"): 0.938, (BF16, "fp32"): 0.996, (F16, "fp32"): 0.997, (BF16, "split"): 1.417}


def bound_for(measured):
    return int(math.ceil(2.0 * measured))


BOUND = {k: bound_for(v) for k, v in MEASURED.items()}
assert __doc__ is None or all(("%.3f" % v) in __doc__ for v in MEASURED.values())


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def designed_input(B, C, H, W, T, seed):
    """[B, C, H, W] float64 holding values of T: designed spectrum (module docstring), rounded to T."""
    g = torch.Generator().manual_seed(seed)
    P = torch.fft.rfft2(torch.randn(B, C, H, W, generator=g, dtype=F64))
    amp = (1.0 + torch.rand(B, C, H, W // 2 + 1, generator=g, dtype=F64)) * math.sqrt(H * W)
    mir = (-torch.arange(H)) % H
    for col in (0, W // 2):
        amp[..., col] = 0.5 * (amp[..., col] + amp[..., mir, col])
    x = torch.fft.irfft2(amp * P / P.abs(), s=(H, W))
    return x.to(T).double()


def noise_input(B, C, H, W, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, H, W, generator=g, dtype=F64).to(T).double()


def band(H, W, radius, high, strict=False):
    kh = torch.arange(H)
    d2 = (torch.minimum(kh, H - kh).double()[:, None] ** 2 + torch.arange(W // 2 + 1).double()[None, :] ** 2)
    sel = d2 < radius * radius if strict else d2 <= radius * radius
    return ~sel if high else sel


def mirror_weights(W):
    w = torch.full((W // 2 + 1,), 2.0, dtype=F64)
    w[0] = 1.0
    if W % 2 == 0:
        w[W // 2] = 1.0
    return w


# ---------------------------------------------------------------------------------------------------------------------------------
# reference and metric
# ---------------------------------------------------------------------------------------------------------------------------------
def reference(x, gy, perm, radius, lam, high):
    """float64: dict(y, dx, A1y, A1dx, ratio, amp_min, amp_max) -- amp_* the extreme |F| in units of sqrt(H W)."""
    H, W = x.shape[-2:]
    perm = torch.as_tensor(perm)
    F_ = torch.fft.rfft2(x)
    A = F_.abs()
    sel = band(H, W, radius, high)
    ratio = torch.where(sel & (A > 1e-20), ((1.0 - lam) * A + lam * A[perm]) / A.clamp_min(1e-30), torch.ones_like(A))
    xr = x.clone().requires_grad_(True)
    y = torch.fft.irfft2(torch.fft.rfft2(xr) * ratio, s=(H, W))
    y.backward(gy)
    wk = mirror_weights(W)
    A1y = (wk * (F_ * ratio).abs()).sum((-1, -2)) / (H * W)
    A1dx = (wk * (torch.fft.rfft2(gy) * ratio).abs()).sum((-1, -2)) / (H * W)
    s = math.sqrt(H * W)
    return dict(y=y.detach(), dx=xr.grad, A1y=A1y, A1dx=A1dx, ratio=ratio, amp_min=float(A.min()) / s, amp_max=float(A.max()) / s)


def check_conditioning(ref, lam):
    """The input conditions of the module docstring, on the float64 reference of the ROUNDED input."""
    assert ref["amp_min"] >= AMP_LO and ref["amp_max"] <= AMP_HI, (ref["amp_min"], ref["amp_max"])
    lo, hi = 1.0 - lam + lam * AMP_LO / AMP_HI, 1.0 - lam + lam * AMP_HI / AMP_LO
    assert float(ref["ratio"].min()) >= lo - 1e-12 and float(ref["ratio"].max()) <= hi + 1e-12, (float(ref["ratio"].min()), float(ref["ratio"].max()))


def scaled_map(got, ref, A1, T):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "non-finite values in the result"
    return (got - ref).abs() / (UT[T] * ref.abs() + U32 * A1[:, :, None, None])


def scaled(got, ref, A1, T):
    return float(scaled_map(got, ref, A1, T).max())


def explain(got, ref, A1, T):
    """Where the largest scaled value sits and which bin of the plane carries the error."""
    q = scaled_map(got, ref, A1, T)
    b, c, h, w = (int(i) for i in torch.unravel_index(q.argmax(), q.shape))
    e = (got.detach().double().cpu() - ref.detach().double().cpu())[b, c]
    E = torch.fft.rfft2(e).abs()
    kh, kw = (int(i) for i in torch.unravel_index(E.argmax(), E.shape))
    return ("scaled %.4g at plane (b=%d, c=%d) pixel (h=%d, w=%d): got %.9g, reference %.9g; the error is carried by bin (kh=%d, kw=%d), "
            "|E| = %.3g of sum |E| = %.3g" % (float(q[b, c, h, w]), b, c, h, w, float(got[b, c, h, w]), float(ref[b, c, h, w]), kh, kw,
                                              float(E[kh, kw]), float(E.sum())))


# ---------------------------------------------------------------------------------------------------------------------------------
# emulations (float32 on the CPU) and planted defects
# ---------------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("unmixed", "conj_twiddle", "mirror_off", "nyq_col_drop", "nyq_col_double", "nyq_row_drop", "nyq_row_double", "band_lt",
           "ws_floor", "partner_ignored", "scale_half", "lam_flip", "bwd_recompute", "chan_neighbour")
DEFECT_OUTPUT = {"bwd_recompute": ("dx",)}                              # every other defect shows in y


def stored_bins(H, W, radius, high):
    """mrfp_fourier_stored_bins on planned lengths with no switch set."""
    Wh = W // 2 + 1
    if high or H not in LENS or W not in LENS or not radius >= 0:
        return Wh
    return min(int(math.floor(radius)) + 1, Wh)


def applies(defect, case):
    moves = case.lam != 0.0 and any(p != b for b, p in enumerate(case.perm))
    H, W = case.H, case.W
    sel = band(H, W, case.radius, case.high)
    if defect in ("unmixed", "partner_ignored", "bwd_recompute"):
        return moves and bool(sel.any())
    if defect == "lam_flip":
        return moves and case.lam != 0.5 and bool(sel.any())
    if defect == "band_lt":
        return moves and bool((sel != band(H, W, case.radius, case.high, strict=True)).any())
    if defect == "ws_floor":
        return moves and not case.high and math.floor(case.radius) + 1 < W // 2 + 1
    if defect in ("nyq_row_drop", "nyq_row_double"):
        return H % 2 == 0
    if defect == "lo_dropped":                                   # (an identity mix adds a zero correction to x: nothing to lose)
        return moves and split_applies(case)
    return True


def split_applies(case):
    """The cases the split-bf16 class describes: a band-limited low band of at most 24 stored bins on whole 16-pixel tiles."""
    ws = stored_bins(case.H, case.W, case.radius, case.high)
    return ws < case.W // 2 + 1 and 2 * ws <= 48 and case.W % 16 == 0


def _ratio32(F_, perm, sel, lam, load=None):
    if load is not None:
        return load
    A = F_.abs()
    lam = torch.tensor(lam, dtype=F32)
    return torch.where(sel & (A > 1e-20), ((1.0 - lam) * A + lam * A[perm]) / A.clamp_min(1e-30), torch.ones_like(A))


def _mix_fp32(x, perm, sel, lam, T, defect, load=None):
    """One pass of the operator in float32 over the whole half spectrum -> (values rounded to T as float64, ratio)."""
    B, C, H, W = x.shape
    S = torch.fft.rfft(x.float(), dim=-1)
    if defect == "conj_twiddle":
        S[..., 1] = S[..., 1].conj()
    F_ = torch.fft.fft(S, dim=-2)
    if defect == "partner_ignored" and load is None:
        b0 = next(b for b, p in enumerate(perm.tolist()) if p != b)
        perm = perm.clone()
        perm[b0] = b0
    ratio = _ratio32(F_, perm, sel, (1.0 - lam) if defect == "lam_flip" else lam, load)
    if defect == "unmixed" and load is None:
        idx = torch.nonzero(sel)
        kh0, kw0 = (int(i) for i in (idx[idx[:, 1] > 0][0] if bool((idx[:, 1] > 0).any()) else idx[0]))
        ratio = ratio.clone()
        ratio[..., kh0, kw0] = 1.0
    Fm = F_ * ratio
    if defect in ("nyq_row_drop", "nyq_row_double"):
        Fm[..., H // 2, :] *= 0.0 if defect == "nyq_row_drop" else 2.0
    G = torch.fft.ifft(Fm, dim=-2)
    if defect in ("nyq_col_drop", "nyq_col_double"):
        G[..., W // 2] *= 0.0 if defect == "nyq_col_drop" else 2.0
    if defect == "mirror_off":                                   # the mirrored half taken one bin off: Z[k] = conj G[W - k + 1]
        k = torch.arange(W // 2 + 1, W)
        Z = torch.cat([G, G[..., W - k + 1].conj()], -1)
        y = torch.fft.ifft(Z, dim=-1).real
    else:
        y = torch.fft.irfft(G, n=W, dim=-1)
    if defect == "scale_half":
        y = y * (W / (W // 2 + 1.0))
    y = y.to(T).double()
    if defect == "chan_neighbour":
        y[:, 5] = y[:, 6]
    return y, ratio


def _split(v):
    hi = v.to(BF16).float()
    return hi, (v - hi).to(BF16).float()


@lru_cache(maxsize=None)
def _trig(W, ws):
    """fp32 (cos, -sin)(2 pi k w / W), k < ws, as the kernels read them from the host's twiddle table -> [ws, W] each."""
    t = (torch.arange(ws)[:, None] * torch.arange(W)[None, :]) % W
    ang = 2.0 * math.pi * t.double() / W
    return torch.cos(ang).float(), (-torch.sin(ang)).float()


def _mix_split(x, perm, sel, lam, ws, defect, load=None):
    """The band-limited form with both row passes as split-bf16 matrix products (bf16 activations)."""
    B, C, H, W = x.shape
    x32 = x.float()
    tc, ts = _trig(W, ws)
    drop = defect == "lo_dropped"
    # forward rows: S[k] = sum_w x[w] (cos, -sin)[k, w], the trigonometric matrix as hi + lo (two products)
    parts = []
    for t in (tc, ts):
        hi, lo = _split(t)
        acc = x32 @ lo.t() if not drop else torch.zeros(B, C, H, ws)
        parts.append(acc + x32 @ hi.t())
    S = torch.complex(parts[0], parts[1])                        # [B, C, H, ws]
    F_ = torch.fft.fft(S, dim=-2)
    ratio = _ratio32(F_, perm, sel[:, :ws], lam, load)
    G = torch.fft.ifft(F_ * (ratio - 1.0), dim=-2, norm="forward")
    # inverse rows: y = x + sum_k g_k / (H W) (Re G_k cos - Im G_k sin), three products hi*hi + lo*hi + hi*lo
    g = torch.full((ws, 1), 2.0)
    g[0] = 1.0
    g = g * torch.tensor(1.0 / (H * W), dtype=F32)
    acc = torch.zeros(B, C, H, W)
    for v, t in ((G.real, g * tc), (G.imag, g * ts)):
        vh, vl = _split(v.contiguous())
        th, tl = _split(t)
        if not drop:
            acc = acc + vl @ th
            acc = acc + vh @ tl
        acc = acc + vh @ th
    return (x32 + acc).to(BF16).double(), ratio


def emulate(x, gy, perm, radius, lam, high, T, cls="fp32", defect=None):
    """Forward and backward of the operator as the class `cls` computes it -> dict(y, dx) of T values in float64."""
    H, W = x.shape[-2:]
    perm = torch.as_tensor(perm)
    sel = band(H, W, radius, high, strict=(defect == "band_lt"))
    if defect == "ws_floor":
        sel = sel.clone()
        sel[:, int(math.floor(radius)):] = False
    if cls == "split":
        assert T == BF16
        ws = stored_bins(H, W, radius, high)
        y, ratio = _mix_split(x, perm, sel, lam, ws, defect)
        dx, _ = _mix_split(gy, perm, sel, lam, ws, defect, load=ratio)
        return dict(y=y, dx=dx)
    y, ratio = _mix_fp32(x, perm, sel, lam, T, defect)
    if defect == "bwd_recompute":
        dx, _ = _mix_fp32(gy, perm, sel, lam, T, None)
    else:
        dx, _ = _mix_fp32(gy, perm, sel, lam, T, defect, load=ratio)
    return dict(y=y, dx=dx)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases.  One line dimension is the length under test, the other is 32; C is the smallest count that reaches the route.
# expect: {dtype: (route of pass 0, pass 1, pass 2)}, a route being (family, kb, tu, nh) -- written down here, asserted against
# mrfp_fourier_route before a case runs.
# ---------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name B C H W radius lam high perm expect")

# instance parameters of the matrix-core passes as csrc/fft.hip chooses them (fwd_tu: the largest of 12, 8, 6, 4, 3, 2 pixel tiles
# that divides W / 16 and fits 160 KB of LDS next to the table; inv_tu: the largest of 6, 4, 3, 2 that divides W / 16)
FWD_TU = {32: 2, 48: 3, 64: 4, 96: 6, 128: 8, 192: 12, 256: 8, 384: 12, 512: 8}
FWD_TU_KB3 = {**FWD_TU, 384: 8, 512: 4}            # 3 k blocks: the table leaves less room (W = 512: 98304 + 65536 + 4096 B > 160 KB)
INV_TU = {32: 2, 48: 3, 64: 4, 96: 6, 128: 4, 192: 6, 256: 4, 384: 6, 512: 4}
_T = (TWOSTEP, 0, 0, 0)
_G = (GENERIC, 0, 0, 0)
_P = (PAIR, 0, 0, 0)
_D = (DIRECT, 0, 0, 0)
ALL_TWOSTEP = (_T, _T, _T)
ALL_GENERIC = (_G, _G, _G)


def mfma_routes(W, C, kb):
    return ((MFMA, kb, (FWD_TU_KB3 if kb == 3 else FWD_TU)[W], 0), _T, (MFMA, kb, INV_TU[W], 2 if C % 64 == 0 else 1))


def _roll(B):
    return tuple((b + 1) % B for b in range(B))


def _case(name, B, C, H, W, radius, expect, lam=0.8, high=False, perm=None):
    return Case(name, B, C, H, W, float(radius), float(lam), bool(high), tuple(perm) if perm is not None else _roll(B), expect)


def _table():
    t = []
    # -- the whole half spectrum on the register path: high band, and a low band whose radius passes the last column
    for L in LENS:
        t.append(_case("full-high-W%d" % L, 2, 16, 32, L, 5, {F32: ALL_TWOSTEP, BF16: ALL_TWOSTEP}, high=True))
        t.append(_case("full-low-W%d" % L, 2, 16, 32, L, L // 2 + 2, {F16: ALL_TWOSTEP}))
        if L != 32:
            t.append(_case("full-high-H%d" % L, 2, 16, L, 32, 5, {F32: ALL_TWOSTEP, F16: ALL_TWOSTEP}, high=True))
            t.append(_case("full-low-H%d" % L, 2, 16, L, 32, 18, {BF16: ALL_TWOSTEP}))
    # -- band-limited, one channel per transform (C % 32 != 0)
    for L in LENS:
        t.append(_case("bl16-W%d" % L, 2, 16, 32, L, 5, {F32: ALL_TWOSTEP, BF16: ALL_TWOSTEP}))
        if L != 32:
            t.append(_case("bl16-H%d" % L, 2, 16, L, 32, 5, {F32: ALL_TWOSTEP, F16: ALL_TWOSTEP}))
    t.append(_case("bl48-W48", 2, 48, 32, 48, 3.5, {F16: ALL_TWOSTEP, BF16: ALL_TWOSTEP}))
    t.append(_case("bl48-W192", 2, 48, 32, 192, 3.5, {F32: ALL_TWOSTEP, BF16: ALL_TWOSTEP}))
    # -- band-limited, C % 32 == 0: channel pairs / direct sum (fp32, f16), matrix cores (bf16) with 1, 2, 3 k blocks
    for L in LENS:
        for r, kb in ((3, 1), (11, 2), (19, 3)):
            if r + 1 >= L // 2 + 1:
                continue                                     # (W = 32, r = 19: the whole half spectrum)
            for C in (32, 64):
                other = (_P, _T, _P) if C == 32 else (_P, _T, _D)
                exp = {BF16: mfma_routes(L, C, kb)}
                if kb == 2:
                    exp.update({F32: other, F16: other})
                t.append(_case("bl%d-W%d-r%d" % (C, L, r), 2, C, 32, L, r, exp))
        if L != 32:
            t.append(_case("bl32-H%d" % L, 2, 32, L, 32, 3, {BF16: mfma_routes(32, 32, 1), F32: (_P, _T, _P)}))
            t.append(_case("bl64-H%d" % L, 2, 64, L, 32, 3, {BF16: mfma_routes(32, 64, 1), F16: (_P, _T, _D)}))
    t.append(_case("bl96-W96", 2, 96, 32, 96, 11, {BF16: mfma_routes(96, 96, 2), F32: (_P, _T, _P), F16: (_P, _T, _P)}))
    # more than 24 stored bins: bf16 leaves the matrix cores; more than 64: the direct sum gives way to the pair transform
    t.append(_case("bl32-W128-r30", 2, 32, 32, 128, 30, {BF16: (_P, _T, _P)}))
    t.append(_case("bl64-W128-r30", 2, 64, 32, 128, 30, {BF16: (_P, _T, _D), F32: (_P, _T, _D)}))
    t.append(_case("bl64-W192-r63", 2, 64, 32, 192, 63, {F32: (_P, _T, _D), F16: (_P, _T, _D)}))
    t.append(_case("bl64-W192-r64", 2, 64, 32, 192, 64, {F32: (_P, _T, _P), BF16: (_P, _T, _P)}))
    # -- the generic Stockham passes: radix 2 only (8 x 32), radix 3 only (H = 27), mixed; the longest lines 486 and 432
    for i, L in enumerate(GEN_LENS):
        t.append(_case("gen-W%d" % L, 2, 16, 32, L, 3, {F32: ALL_GENERIC, (BF16, F16)[i % 2]: ALL_GENERIC}, high=bool(i % 2)))
    for i, L in enumerate((8, 12, 27, 54, 162, 432, 486)):
        t.append(_case("gen-H%d" % L, 2, 16, L, 32, 3, {F32: ALL_GENERIC, (F16, BF16)[i % 2]: ALL_GENERIC}, high=not i % 2))
    t.append(_case("gen-8x8", 2, 16, 8, 8, 2, {F32: ALL_GENERIC, BF16: ALL_GENERIC}))
    # -- the persistent loops of the matrix-core passes: 3 * 128 lines * 9 channel blocks = 3456 items > 256 workgroups x 8 waves
    # (forward) and > 768 workgroups x 4 waves (inverse: two items per wave)
    t.append(_case("persistent", 3, 288, 128, 32, 3, {BF16: mfma_routes(32, 288, 1)}))
    # -- edges
    t.append(_case("edge-r0", 2, 32, 32, 48, 0, {F32: (_P, _T, _P), BF16: mfma_routes(48, 32, 1)}))
    t.append(_case("edge-r3.5", 2, 64, 32, 64, 3.5, {F32: (_P, _T, _D), BF16: mfma_routes(64, 64, 1)}))
    t.append(_case("edge-r5-circle16", 2, 16, 32, 32, 5, {F32: ALL_TWOSTEP, F16: ALL_TWOSTEP}))
    t.append(_case("edge-r5-circle32", 2, 32, 32, 48, 5, {F16: (_P, _T, _P), BF16: mfma_routes(48, 32, 1)}))
    t.append(_case("edge-r16-half-H", 2, 32, 32, 64, 16, {F32: (_P, _T, _P), BF16: mfma_routes(64, 32, 3)}))
    t.append(_case("edge-high-nyquist", 2, 32, 48, 64, 2, {F16: ALL_TWOSTEP, BF16: ALL_TWOSTEP}, high=True))
    t.append(_case("edge-identity", 1, 32, 32, 48, 5, {F32: (_P, _T, _P), BF16: mfma_routes(48, 32, 1)}, lam=1.0, perm=(0,)))
    t.append(_case("edge-identity-full", 1, 16, 32, 48, 5, {F32: ALL_TWOSTEP}, lam=1.0, perm=(0,), high=True))
    t.append(_case("edge-fixed-point", 3, 64, 32, 48, 5, {F32: (_P, _T, _D), BF16: mfma_routes(48, 64, 1)}, perm=(1, 0, 2)))
    t.append(_case("edge-non-injective", 3, 32, 32, 48, 5, {F32: (_P, _T, _P), BF16: mfma_routes(48, 32, 1)}, perm=(0, 0, 0)))
    t.append(_case("edge-lam0", 2, 64, 32, 48, 5, {F32: (_P, _T, _D), BF16: mfma_routes(48, 64, 1)}, lam=0.0))
    t.append(_case("edge-lam1", 2, 64, 32, 48, 5, {F32: (_P, _T, _D), BF16: mfma_routes(48, 64, 1)}, lam=1.0))
    return t


TABLE = _table()
CASES = {c.name: c for c in TABLE}
assert len(CASES) == len(TABLE)
RUNS = [(c.name, T) for c in TABLE for T in c.expect]          # every (case, activation type) the GPU file runs


def run_id(run):
    return "%s-%s" % (run[0], dname(run[1]))


def _seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)) % 100003


@lru_cache(maxsize=None)
def inputs(name, T):
    c = CASES[name]
    return designed_input(c.B, c.C, c.H, c.W, T, _seed(c)), noise_input(c.B, c.C, c.H, c.W, T, _seed(c) + 1)


@lru_cache(maxsize=4)
def reference_of(name, T):
    """The float64 reference of a (case, type): computed once, shared by the tests that need it, never written to."""
    c = CASES[name]
    x, gy = inputs(name, T)
    return reference(x, gy, c.perm, c.radius, c.lam, c.high)


def emulate_case(name, T, cls="fp32", defect=None):
    c = CASES[name]
    x, gy = inputs(name, T)
    return emulate(x, gy, c.perm, c.radius, c.lam, c.high, T, cls, defect)


def worst(out, ref, T):
    return dict(y=scaled(out["y"], ref["y"], ref["A1y"], T), dx=scaled(out["dx"], ref["dx"], ref["A1dx"], T))


# ---------------------------------------------------------------------------------------------------------------------------------
# the A/B switches: one short sub-table, and what every case's routes become under each switch (None: no switch set)
# ---------------------------------------------------------------------------------------------------------------------------------
SWITCHES = (("MRFP_FFT_GENERIC", "1"), ("MRFP_FFT_FULL", "1"), ("MRFP_FFT_NOPAIR", "1"), ("MRFP_FFT_NODIRECT", "1"), ("MRFP_FFT_MFMA", "0"))
_M96 = mfma_routes(96, 64, 1)
_M192 = mfma_routes(192, 32, 3)
SWITCH_TABLE = [
    # (case, type, {switch name or None: routes})
    (_case("sw-bf16-c64", 2, 64, 32, 96, 5, None), BF16,
     {None: _M96, "MRFP_FFT_GENERIC": ALL_GENERIC, "MRFP_FFT_FULL": ALL_TWOSTEP, "MRFP_FFT_NOPAIR": _M96,
      "MRFP_FFT_NODIRECT": (_M96[0], _T, _P), "MRFP_FFT_MFMA": (_P, _T, _D)}),
    (_case("sw-bf16-c32-kb3", 2, 32, 32, 192, 19, None), BF16,
     {None: _M192, "MRFP_FFT_GENERIC": ALL_GENERIC, "MRFP_FFT_FULL": ALL_TWOSTEP, "MRFP_FFT_NOPAIR": _M192,
      "MRFP_FFT_NODIRECT": (_M192[0], _T, _P), "MRFP_FFT_MFMA": (_P, _T, _P)}),
    (_case("sw-f32-c64", 2, 64, 32, 48, 5, None), F32,
     {None: (_P, _T, _D), "MRFP_FFT_GENERIC": ALL_GENERIC, "MRFP_FFT_FULL": ALL_TWOSTEP, "MRFP_FFT_NOPAIR": ALL_TWOSTEP,
      "MRFP_FFT_NODIRECT": (_P, _T, _P), "MRFP_FFT_MFMA": (_P, _T, _D)}),
    (_case("sw-f16-c64-H192", 2, 64, 192, 32, 3, None), F16,
     {None: (_P, _T, _D), "MRFP_FFT_GENERIC": ALL_GENERIC, "MRFP_FFT_FULL": ALL_TWOSTEP, "MRFP_FFT_NOPAIR": ALL_TWOSTEP,
      "MRFP_FFT_NODIRECT": (_P, _T, _P), "MRFP_FFT_MFMA": (_P, _T, _D)}),
    (_case("sw-f16-c32", 2, 32, 32, 64, 11, None), F16,
     {None: (_P, _T, _P), "MRFP_FFT_GENERIC": ALL_GENERIC, "MRFP_FFT_FULL": ALL_TWOSTEP, "MRFP_FFT_NOPAIR": ALL_TWOSTEP,
      "MRFP_FFT_NODIRECT": (_P, _T, _P), "MRFP_FFT_MFMA": (_P, _T, _P)}),
    (_case("sw-f32-c16", 2, 16, 48, 128, 5, None), F32,
     {None: ALL_TWOSTEP, "MRFP_FFT_GENERIC": ALL_GENERIC, "MRFP_FFT_FULL": ALL_TWOSTEP, "MRFP_FFT_NOPAIR": ALL_TWOSTEP,
      "MRFP_FFT_NODIRECT": ALL_TWOSTEP, "MRFP_FFT_MFMA": ALL_TWOSTEP}),
    (_case("sw-bf16-high", 2, 32, 192, 32, 5, None, high=True), BF16,
     {None: ALL_TWOSTEP, "MRFP_FFT_GENERIC": ALL_GENERIC, "MRFP_FFT_FULL": ALL_TWOSTEP, "MRFP_FFT_NOPAIR": ALL_TWOSTEP,
      "MRFP_FFT_NODIRECT": ALL_TWOSTEP, "MRFP_FFT_MFMA": ALL_TWOSTEP}),
    # the one long line: under MRFP_FFT_GENERIC the Stockham kernel asks for its largest LDS buffer (2 x 512 x 16 x 8 B = 128 KB)
    (_case("sw-f32-c16-W512", 2, 16, 32, 512, 5, None), F32,
     {None: ALL_TWOSTEP, "MRFP_FFT_GENERIC": ALL_GENERIC, "MRFP_FFT_FULL": ALL_TWOSTEP, "MRFP_FFT_NOPAIR": ALL_TWOSTEP,
      "MRFP_FFT_NODIRECT": ALL_TWOSTEP, "MRFP_FFT_MFMA": ALL_TWOSTEP}),
]
for _c, _t, _ in SWITCH_TABLE:
    CASES[_c.name] = _c
SWITCH_WS_FULL = ("MRFP_FFT_GENERIC", "MRFP_FFT_FULL")                 # switches under which every case stores the whole half spectrum


def route_class(routes):
    """The arithmetic class (key of BOUND) of a run from its routes."""
    return "split" if any(r[0] == MFMA for r in routes) else "fp32"


# ---------------------------------------------------------------------------------------------------------------------------------
# routes: what mrfp_fourier_route says (`lib` is the loaded library; this module does not load it)
# ---------------------------------------------------------------------------------------------------------------------------------
DT = {F32: 0, BF16: 1, F16: 2}
_SWITCH_DEFAULT = {"MRFP_FFT_GENERIC": 0, "MRFP_FFT_FULL": 0, "MRFP_FFT_NOPAIR": 0, "MRFP_FFT_NODIRECT": 0, "MRFP_FFT_MFMA": 1}


def active_switch():
    """The one A/B switch this process runs under (None: none); the library reads them once per process, from the same environment."""
    import os
    on = [n for n, d in _SWITCH_DEFAULT.items() if os.environ.get(n) not in (None, "") and int(os.environ[n]) != d]
    assert len(on) <= 1, on
    return on[0] if on else None


def routes_of(lib, c, T, passes=(0, 1, 2)):
    import ctypes
    out = []
    for p in passes:
        kb, tu, nh = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        k = lib.mrfp_fourier_route(DT[T], c.H, c.W, c.C, c.radius, int(c.high), p, ctypes.byref(kb), ctypes.byref(tu), ctypes.byref(nh))
        out.append((k, kb.value, tu.value, nh.value))
    return tuple(out)


def check_completeness(lib):
    """The table runs every kernel instance a call can reach, proved from mrfp_fourier_route (not from the table's own labels)."""
    bins = lambda c: int(lib.mrfp_fourier_stored_bins(c.H, c.W, c.radius, int(c.high)))
    runs = [(CASES[n], T, routes_of(lib, CASES[n], T)) for n, T in RUNS]
    # 1. the instances: every type x planned W x C in {32, 64} x 1, 2, 3 k blocks (4, 12, 20 stored bins), band-limited
    grid_r = (3.0, 11.0, 19.0)
    reach = set()
    for T in (F32, BF16, F16):
        for W in LENS:
            for C in (32, 64):
                for r in grid_r:
                    c = _case("enum", 2, C, 32, W, r, None)
                    if bins(c) < W // 2 + 1:
                        rt = routes_of(lib, c, T)
                        reach |= {(T, W, 0) + rt[0], (T, W, 2) + rt[2]}
    ran = set()
    for c, T, rt in runs:
        if c.H == 32 and c.C in (32, 64) and c.radius in grid_r and not c.high and bins(c) < c.W // 2 + 1:
            ran |= {(T, c.W, 0) + rt[0], (T, c.W, 2) + rt[2]}
    assert reach == ran, (sorted(reach - ran, key=str), sorted(ran - reach, key=str))
    inst = lambda s: {(p,) + tuple(t) for (T, W, p, *t) in s if t[0] == MFMA}
    fwd = {(kb, tu) for (p, k, kb, tu, nh) in inst(reach) if p == 0}
    inv = {(kb, tu, nh) for (p, k, kb, tu, nh) in inst(reach) if p == 2}
    # what csrc/fft.hip instantiates: KB x TU (x NH), without the segment sizes no planned width produces
    assert fwd == {(kb, tu) for kb in (1, 2, 3) for tu in (12, 8, 6, 4, 3, 2)} - {(3, 2)}, sorted(fwd)
    assert inv == {(kb, tu, nh) for kb in (1, 2, 3) for tu in (6, 4, 3, 2) for nh in (1, 2)} - {(3, 2, 1), (3, 2, 2)}, sorted(inv)
    assert (MFMA, 3, 8, 0) == routes_of(lib, CASES["bl32-W256-r19"], BF16)[0] and (MFMA, 3, 4, 0) == routes_of(lib, CASES["bl32-W512-r19"], BF16)[0]
    # 2. every planned length as W and as H (the other dimension 32) on the whole-spectrum and the band-limited routes
    for L in LENS:
        for axis in ("W", "H"):
            seen = set()
            for c, T, rt in runs:
                if (c.W, c.H) != ((L, 32) if axis == "W" else (32, L)):
                    continue
                full = bins(c) == c.W // 2 + 1
                if full:
                    assert all(r[0] == TWOSTEP for r in rt)
                    seen.add("full-high" if c.high else "full-low")
                else:
                    seen |= {"bl0-%s" % ROUTE_NAMES[rt[0][0]], "bl2-%s" % ROUTE_NAMES[rt[2][0]]}
            want = {"full-high", "full-low", "bl0-two-step", "bl2-two-step", "bl0-pair", "bl2-pair", "bl2-direct", "bl0-mfma", "bl2-mfma"}
            assert seen == want, (L, axis, sorted(want - seen), sorted(seen - want))
    # 3. every family in fp32 and in a 16-bit type
    types = {}
    for c, T, rt in runs:
        for p in (0, 2):
            types.setdefault((p, rt[p][0], bins(c) < c.W // 2 + 1), set()).add(T)
    for key in ((0, TWOSTEP, True), (2, TWOSTEP, True), (0, TWOSTEP, False), (0, PAIR, True), (2, PAIR, True), (2, DIRECT, True), (0, GENERIC, False)):
        assert F32 in types[key] and types[key] & {BF16, F16}, (key, types.get(key))
    assert BF16 in types[2, DIRECT, True] and BF16 in types[0, PAIR, True]          # bf16 past 24 stored bins
    assert types[0, MFMA, True] == {BF16} and types[2, MFMA, True] == {BF16}
    # 4. the generic passes: the lengths, radix 2 only, radix 3 only, mixed, the longest lines
    gen = [(c, T) for c, T, rt in runs if rt[0][0] == GENERIC]
    assert all(routes_of(lib, c, T, (0, 1, 2, 3)) == (_G,) * 4 for c, T in gen)
    assert {c.W for c, _ in gen} >= set(GEN_LENS) and {c.H for c, _ in gen} >= {8, 12, 27, 54, 162, 432, 486}
    pure = lambda n, p: n > 1 and p ** round(math.log(n, p)) == n
    assert any(pure(c.H, 2) and pure(c.W, 2) for c, _ in gen) and any(pure(c.H, 3) for c, _ in gen)
    # 5. the persistent loops of the matrix-core passes (csrc/fft.hip: 256 workgroups x 8 waves forward, 768 x 4 inverse)
    items0 = max(c.B * c.H * (c.C // 32) for c, T, rt in runs if rt[0][0] == MFMA)
    items2 = max(c.B * c.H * (c.C // (32 * rt[2][3])) * ((c.W // 16) // rt[2][2]) for c, T, rt in runs if rt[2][0] == MFMA)
    assert items0 > 256 * 8 and items2 > 768 * 4, (items0, items2)
