"""Per-element rounding model of the 16-bit row operators: metric, designed inputs, float64 references, fp32 emulation.

Host only (torch on the CPU; nothing here imports the HIP library).  tests/test_rounding_model_cpu.py proves the model on the host,
tests/test_ops_16bit_gpu.py holds the kernels of csrc/stats.hip, csrc/affine.hip and csrc/resize_pool.hip to it.

The metric.  The kernels compute in fp32 and round ONCE, at the store, to the activation type T.  For a device result d stored in
T, the float64 reference r and the magnitude mag (both from inputs already rounded to T):

    scaled(d, r, mag) = max_i  (|d_i - r_i| - u_T |r_i| - h_T)+ / (u_32 mag_i)   u_bf16 = 2^-8, u_f16 = 2^-11, u_32 = 2^-24

h_T is half the spacing of T's subnormal numbers (f16: 2^-25; bf16: 2^-134, nothing): below 2^-14 an f16 store rounds to multiples
of 2^-24, so the correctly rounded float64 reference itself is up to 2^-25 away from r, which u_T |r| does not cover (a gradient
P*dy of 3e-5 would score 0.5 / mag > 4096 with a perfect kernel; test_rounding_model_cpu.py shows it).  scaled() is
what is left of the error after the one rounding to T, in units of one fp32 rounding of the terms of the expression.  mag_i is
the sum of the absolute values of the terms of the float64 expression at element i (forward apply |x*A| + |S| + |res|; input
gradient |P*dy| + |Q*x| + |R|, behind a nearest resize |P| sum|dy| + n (|Q*x| + |R|); bilinear sum_k |w_k x_k|; max-pool backward
sum |dy| over the windows routed to i).  fp32 outputs of reductions (dweight, dbias, running statistics, plane means) have no u_T
term and mag = sum |terms|.  There is no tensor-max normalisation: a wrong value in a small-magnitude channel fails.  An element
passes when scaled < C_F32[op].  The allowance u_T |r| is the LARGEST error of one rounding to T, so the metric does not see an
error that stays below one T-ulp of its own element (the emulation's 0.000 for max_pool and the elementwise operators is that,
not exactness to fp32): C_F32 bounds what exceeds the rounding, it is not a bound of so many fp32 roundings on the total error.

C_F32 is measured against the REFERENCE, never against the kernels: 16 x the largest scaled value the fp32 emulation below (plain
torch float32 on the CPU: fp32 sums, coefficients as the *_finalize_kernels of csrc/stats.hip form them, fp32 apply, one rounding
to T at the store, the ReLU gate read from the stored output) reaches over all cases and both types of the operator, rounded up to
a power of two.  The factor 16 covers the accumulation order (torch sums pairwise; the kernels run short per-thread chains and
combine them in float64) and a fused multiply-add in the apply expressions.  An operator whose emulation is exact (largest scaled
value below 1: max-pool backward with one routed window, add) gets the floor 16 = 16 x one fp32 rounding of the terms, the unit of
the metric.  test_rounding_model_cpu.py re-measures the table below and fails if a value has outgrown its record (by more than a
factor of 2: the last digits depend on how the host's torch build orders its fp32 sums).

    operator     largest scaled value of the emulation (bf16 / f16)       C_F32
    ----------   ----------------------------------------------------     -----
    batch_norm                  5.547 / 2.473                             128
    batch_norm_eval             1.601 / 1.920                              32
    batch_norm_relu6            1.681 / 1.657                              32
    batch_norm_resize           2.139 / 2.995                              64
    instance_norm              11.082 / 6.039                             256
    np_plus                     0.287 / 1.331                              32
    bilinear                    6.216 / 4.363                             128
    max_pool                    0.000 / 0.000                              16
    instance_norm_relu_pool     0.842 / 0.799                              16
    elementwise                 0.000 / 0.000                              16

Every constant is <= 4096 (asserted at import): the weakest planted defect (one line left out of dbeta) scores about 1e6, so a
constant above 4096 would mean that mag is wrong, not that the arithmetic is loose.

Designed upstream gradients.  An i.i.d. zero-mean gy hides the statistic terms of a normalisation backward (Q*x + R; the constant
K of NP+): they are O(1/sqrt(B H W)) of the result.  Here gy = round_T(0.5 s1 + 0.7 s2 xhat + noise) with fixed signs s1, s2 per
channel (BatchNorm) or per (image, channel) (InstanceNorm), and round_T(0.8 s + noise) for NP+; every case asserts on its float64
reference that max|dx - P*dy| >= 0.25 max|dx|.

ReLU gates and pool ties are properties of the input, not of a kernel: settle() moves the input values whose float64
pre-activation lies within BAND x the magnitude of its terms of a gate (at most 1e-4 of a case's elements, asserted; none is left),
no_tie_planes() builds max-pool inputs without ties inside a window.
"""
import math

import torch
import torch.nn.functional as F

from oracle import mrfp_oracle as orc

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
F64 = torch.float64
TYPES = (BF16, F16)
U = {BF16: 2.0 ** -8, F16: 2.0 ** -11}
HALF_SUB = {BF16: 2.0 ** -134, F16: 2.0 ** -25}      # h_T: half the spacing of T's subnormal numbers
U32 = 2.0 ** -24
EPS = 1e-5
MOMENTUM = 0.1
BAND = 4e-6          # 16 x the fp32 error of x*A + S (+ res) with rounded coefficients (4 roundings of 2^-24 each), relative to its terms
SETTLE_CAP = 1e-4    # the largest fraction of a case's elements settle() may move

# largest scaled value of the honest emulation over all cases of the operator, per type (measured on the CPU: test_rounding_model_cpu.py
# test_emulation_table_is_current prints and re-checks them), and the constant derived from it
MEASURED = {
    "batch_norm": (5.547, 2.473),
    "batch_norm_eval": (1.601, 1.920),
    "batch_norm_relu6": (1.681, 1.657),
    "batch_norm_resize": (2.139, 2.995),
    "instance_norm": (11.082, 6.039),
    "np_plus": (0.287, 1.331),
    "bilinear": (6.216, 4.363),
    "max_pool": (0.000, 0.000),
    "instance_norm_relu_pool": (0.842, 0.799),
    "elementwise": (0.000, 0.000),
}


def constant_for(measured):
    """16 x the measured value, rounded up to a power of two; floor 16 (one fp32 rounding of the terms, times the same factor)."""
    return float(2 ** max(4, math.ceil(math.log2(16.0 * max(measured, 1e-30)))))


C_F32 = {op: constant_for(max(v)) for op, v in MEASURED.items()}
assert all(c <= 4096 for c in C_F32.values()), C_F32
assert __doc__ is None or all(("%.3f / %.3f" % v) in __doc__ for v in MEASURED.values())      # the docstring's table is this record


def dname(dtype):
    return str(dtype).replace("torch.", "")


def rt(x, T):
    """x rounded to T, held in x's own type (T None: unchanged)."""
    return x if T is None else x.to(T).to(x.dtype)


def rnd(*shape, seed=0, scale=1.0, shift=0.0, dtype=F32):
    """scale * randn + shift, rounded to `dtype` (returned as float32 on the host)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype).float()


def signs(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()


def scaled(d, r, mag, T=None):
    """The metric of the module docstring (T None: an fp32 reduction output, no u_T term).  A difference where mag is zero is infinite."""
    d, r, mag = d.detach().double().cpu(), r.detach().double().cpu(), mag.detach().double().cpu()
    assert d.shape == r.shape, (d.shape, r.shape)
    mag = mag.expand_as(r)
    assert bool(torch.isfinite(d).all()), "non-finite values in the result"
    num = ((d - r).abs() - ((U[T] * r.abs() + HALF_SUB[T]) if T is not None else 0.0)).clamp_min(0.0)
    den = U32 * mag
    q = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, math.inf), torch.zeros_like(num)))
    return float(q.max()) if q.numel() else 0.0


def relerr(a, b):
    """The old measure (tests/test_ops_gpu.py): largest difference over the largest reference value of the tensor."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


# ---------------------------------------------------------------------------------------------------------------------------------
# ReLU gates and pool ties
# ---------------------------------------------------------------------------------------------------------------------------------
def settle(x, dtype, pre, tries=16, moved=None):
    """x with no ReLU pre-activation within BAND of its gate.  pre(x float64) -> [(distance to the gate, magnitude of the terms)].
    moved: a list that receives the number of elements that differ from the x passed in."""
    x0 = x
    for _ in range(tries):
        near = None
        for z, mag in pre(x.double()):
            n = z.abs() <= BAND * mag
            near = n if near is None else (near | n)
        if not bool(near.any()):
            if moved is not None:
                moved.append(int((x != x0).sum()))
            return x
        x = torch.where(near, x + x.abs().clamp_min(1.0) * 2.0 ** -5, x).to(dtype).float()
    raise AssertionError("could not move the inputs away from the ReLU gate")


def settled(make, dtype, pre, tries=8):
    """make(k) -> the k-th draw of a case's input.  The first draw that settle() leaves within its cap -- at most SETTLE_CAP of the
    elements moved, which for a case of fewer than 10^4 elements means none -- settled (none is left in the band: settle() raises
    otherwise).  The choice is a property of the input alone: it is made on the float64 pre-activations, before any kernel runs."""
    for k in range(tries):
        moved = []
        x = settle(make(k), dtype, pre, moved=moved)
        if moved[0] <= SETTLE_CAP * x.numel():
            return x
    raise AssertionError("no draw of the input within the settle() cap")


def norm_pre(w, b, res, dims, gates=(0.0,), stats=None):
    """The pre-activation (x - m) * w / sqrt(v + eps) + b + res of a normalisation over `dims` as the kernels evaluate it, x*A + S
    + res with A = w / sqrt(v + eps), S = b - m*A: (distance to each gate, |x*A| + |m*A| + |b| + |res| + |gate|)."""
    def pre(x):
        if stats is None:
            m, v = x.mean(dims, keepdim=True), x.var(dims, unbiased=False, keepdim=True)
        else:
            m, v = (s.double().view(1, -1, 1, 1) for s in stats)
        wv = w.double().view(1, -1, 1, 1) if w is not None else 1.0
        bv = b.double().view(1, -1, 1, 1) if b is not None else torch.zeros(())
        a = wv / (v + EPS).sqrt()
        r = res.double() if res is not None else torch.zeros(())
        z = (x - m) * a + bv + r
        mag = (x * a).abs() + (m * a).abs() + bv.abs() + r.abs()
        return [(z - g, mag + abs(g)) for g in gates]
    return pre


def no_tie_planes(shape, seed, spread=16):
    """Max-pool inputs without ties inside any 3x3 window, exactly representable in bf16 / fp16 / fp32: pixel (h, w) of a plane
    holds 16 * P[(h % 3, w % 3)] + n - 72 with P a per-plane permutation of 0..8 and n a random integer of 0..spread-1 -- a window
    holds every residue class at most once, classes differ by at least 17 - spread > 0, and all values are integers of magnitude < 128."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    perm = torch.rand(B, C, 9, generator=g).argsort(-1)
    cls = (torch.arange(H).view(H, 1) % 3) * 3 + (torch.arange(W).view(1, W) % 3)
    base = torch.gather(perm, 2, cls.flatten().expand(B, C, H * W)).view(B, C, H, W)
    return (16 * base + torch.randint(0, spread, (B, C, H, W), generator=g) - 72).float()


def window_max_count(z):
    """How often each 3x3 / stride 2 / pad 1 window of z attains its maximum -> (count, maximum)."""
    zp = F.pad(z, (1, 1, 1, 1), value=-math.inf)
    win = zp.unfold(2, 3, 2).unfold(3, 3, 2)                      # [B, C, Ho, Wo, 3, 3]
    mx = win.amax((-1, -2))
    return (win == mx[..., None, None]).sum((-1, -2)), mx


def window_gap_ok(z, T):
    """Every window of z (float64) keeps its arg-max after a rounding to T: the runner-up lies more than 4 u_T below a positive
    maximum (two roundings of u_T each cannot reorder them), or the maximum is not positive (behind a ReLU: no gradient)."""
    zp = F.pad(z, (1, 1, 1, 1), value=-math.inf)
    win = zp.unfold(2, 3, 2).unfold(3, 3, 2).flatten(-2)
    top = win.topk(2, -1).values
    mx, second = top[..., 0], top[..., 1]
    return bool(((mx <= 0) | (mx - second > 4 * U[T] * mx.abs())).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# nearest resize (ops.nearest_plan): index tables of F.interpolate(mode="nearest")
# ---------------------------------------------------------------------------------------------------------------------------------
def nearest_tables(Hs, Ws, scale=None, size=None):
    if scale is not None:
        Ho, Wo = orc.nearest_out_size(Hs, scale), orc.nearest_out_size(Ws, scale)
    else:
        Ho, Wo = size
    th = torch.from_numpy(orc.nearest_src_index(Hs, Ho, scale)).long()
    tw = torch.from_numpy(orc.nearest_src_index(Ws, Wo, scale)).long()
    return th, tw


def _resize(x, tabs):
    return x if tabs is None else x[:, :, tabs[0]][:, :, :, tabs[1]]


def _fold(g, tabs, Hs, Ws):
    """Sum of the destination values that read each source pixel."""
    if tabs is None:
        return g
    out = torch.zeros(g.shape[0], g.shape[1], Hs, g.shape[3], dtype=g.dtype).index_add_(2, tabs[0], g)
    return torch.zeros(g.shape[0], g.shape[1], Hs, Ws, dtype=g.dtype).index_add_(3, tabs[1], out)


def _last_vec_zero(t, C):
    """Planted defect: the last channel vector (8 channels; the last channel on the scalar path) of a line's last pixel not written."""
    t = t.clone()
    t[:, C - (8 if C % 8 == 0 else 1):, :, -1] = 0
    return t


# ---------------------------------------------------------------------------------------------------------------------------------
# normalisations: one restatement in two precisions.  fd = float64, T = None: the reference expression with its magnitudes;
# fd = float32, T = bf16 / f16: the emulation of the kernels (and of the planted defects)
# ---------------------------------------------------------------------------------------------------------------------------------
DEFECTS_NORM = ("qr0", "roll", "lastline", "lastvec", "gate_left", "double_round", "mult1")
DEFECTS_NP = ("k0", "roll", "lastline", "lastvec")


def norm_model(kind, x, w, b, gy, *, res=None, act=None, training=True, rm=None, rv=None, tabs=None, fd=F64, T=None, defect=None):
    """kind "bn" (statistics over batch and plane) or "in" (per image).  act None / "relu" / "relu6".  tabs: index tables of a
    nearest resize in front.
    -> dict of outputs (y, dx, dres, dw, db, rm, rv as they apply); with fd = float64 also out["mag"] (same keys) and out["stat"],
    the statistic part dx - P*dy of the input gradient."""
    B, C, Hs, Ws = x.shape
    dims = (0, 2, 3) if kind == "bn" else (2, 3)
    cshape = (1, C, 1, 1) if kind == "bn" else (B, C, 1, 1)
    xs = x.to(fd)
    up = _resize(xs, tabs)
    N = float(up.numel() // (C if kind == "bn" else B * C))
    wd = w.double().view(1, C, 1, 1) if w is not None else torch.ones(1, 1, 1, 1, dtype=F64)
    bd = b.double().view(1, C, 1, 1) if b is not None else torch.zeros(1, 1, 1, 1, dtype=F64)
    roll = (lambda t: t.roll(1, 1)) if defect == "roll" else (lambda t: t)
    out, mag = {}, {}
    if training:
        s = roll(up.sum(dims, keepdim=True).double())
        q = roll((up * up).sum(dims, keepdim=True).double())
        m = s / N
        var = (q / N - m * m).clamp_min(0.0)
        inv = 1.0 / (var + EPS).sqrt()
        mean_f, inv_f = m.to(fd), inv.to(fd)
        A = (wd * inv).to(fd)
        S = (bd - m * A.double()).to(fd)
        if rm is not None:
            unb = var * N / (N - 1.0) if N > 1 else var
            out["rm"] = ((1.0 - MOMENTUM) * rm.double() + MOMENTUM * m.flatten()).to(fd)
            out["rv"] = ((1.0 - MOMENTUM) * rv.double() + MOMENTUM * unb.flatten()).to(fd)
            if fd == F64:
                mag["rm"] = (1.0 - MOMENTUM) * rm.double().abs() + MOMENTUM * up.abs().sum(dims) / N
                mag["rv"] = (1.0 - MOMENTUM) * rv.double().abs() + MOMENTUM * (N / max(N - 1.0, 1.0)) * (q.flatten() / N + m.flatten() ** 2)
    else:                                       # bn_eval_coef_kernel: fp32 throughout
        mean_f = rm.to(fd).view(1, C, 1, 1)
        inv_f = 1.0 / (rv.to(fd).view(1, C, 1, 1) + torch.tensor(EPS, dtype=fd)).sqrt()
        A = wd.to(fd) * inv_f
        S = bd.to(fd) - mean_f * A
    A, S = A.expand(cshape), S.expand(cshape)
    z = up * A + S
    r_ = res.to(fd) if res is not None else None
    if r_ is not None:
        z = (rt(z, T) if defect == "double_round" else z) + r_
    if act == "relu":
        y = z.clamp_min(0.0)
    elif act == "relu6":
        y = z.clamp(0.0, 6.0)
    else:
        y = z
    ys = rt(y, T)
    if act == "relu":                           # the residual tail reads its gate from the stored output (or its sign mask)
        gate = (ys > 0) if (r_ is not None and T is not None) else (z > 0)
    elif act == "relu6":                        # the pass mask of the fp32 pre-activation
        gate = (z > 0) & (z < 6)
    else:
        gate = torch.ones_like(z, dtype=torch.bool)
    if defect == "gate_left":
        gate = gate.roll(1, 3)
    g = gy.to(fd)
    out["y"] = ys if defect != "lastvec" else _last_vec_zero(ys, C)
    gabs = g.abs()
    dyp = torch.where(gate, g, torch.zeros_like(g))
    if res is not None:
        out["dres"] = rt(dyp, T) if defect != "lastvec" else _last_vec_zero(rt(dyp, T), C)
    red = dyp if defect != "lastline" else torch.cat([dyp[:, :, :-1], torch.zeros_like(dyp[:, :, -1:])], 2)
    Ss = roll(red.sum(dims, keepdim=True).double())
    Sq = roll((red * (up - mean_f)).sum(dims, keepdim=True).double())
    isd, md = inv_f.double(), mean_f.double()
    out["db"] = Ss.sum(0).flatten().to(fd)
    out["dw"] = (Sq * isd).sum(0).flatten().to(fd)
    P = wd * isd
    Q = -wd * isd * isd * isd * Sq / N
    R = -P * Ss / N - Q * md
    if not training or defect == "qr0":
        Q, R = torch.zeros_like(Q), torch.zeros_like(R)
    P, Q, R = P.to(fd).expand(cshape), Q.to(fd).expand(cshape), R.to(fd).expand(cshape)
    acc = _fold(dyp, tabs, Hs, Ws)
    if tabs is None:
        n = 1.0
        dx = P * acc + (Q * xs + R)
    else:
        n = _fold(torch.ones(1, 1, up.shape[2], up.shape[3], dtype=fd), tabs, Hs, Ws)
        if defect == "mult1":
            n = torch.ones_like(n)
        dx = P * acc + n * (Q * xs + R)
    out["dx"] = rt(dx, T) if defect != "lastvec" else _last_vec_zero(rt(dx, T), C)
    if fd == F64:
        gatef = gate.double()
        mag["y"] = (up * A).abs() + S.abs() + (r_.abs() if r_ is not None else 0.0)
        if res is not None:
            mag["dres"] = dyp.abs()
        aabs = gabs * gatef
        mag["db"] = aabs.sum(dims, keepdim=True).sum(0).flatten()
        mag["dw"] = ((aabs * (up.abs() + md.abs())).sum(dims, keepdim=True) * isd).sum(0).flatten()
        mag["dx"] = P.abs() * _fold(aabs, tabs, Hs, Ws) + n * ((Q * xs).abs() + R.abs())
        out["mag"] = mag
        out["stat"] = dx - P * acc
        out["xhat"] = (up - md) * isd
    return out


def norm_autograd(kind, x, w, b, gy, *, res=None, act=None, training=True, rm=None, rv=None, tabs=None, scale=None, size=None):
    """The same operator through torch's own float64 functions and autograd: the reference values."""
    x64 = x.double().clone().requires_grad_(True)
    w64 = w.double().clone().requires_grad_(True) if w is not None else None
    b64 = b.double().clone().requires_grad_(True) if b is not None else None
    r64 = res.double().clone().requires_grad_(True) if res is not None else None
    rm64 = rm.double().clone() if rm is not None else None
    rv64 = rv.double().clone() if rv is not None else None
    up = x64
    if tabs is not None:
        up = F.interpolate(x64, scale_factor=scale, mode="nearest") if scale is not None else F.interpolate(x64, size=size, mode="nearest")
    if kind == "bn":
        y = F.batch_norm(up, rm64, rv64, w64, b64, training, MOMENTUM, EPS)
    else:
        y = F.instance_norm(up, None, None, w64, b64, True, MOMENTUM, EPS)
    if r64 is not None:
        y = y + r64
    if act == "relu":
        y = F.relu(y)
    elif act == "relu6":
        y = F.hardtanh(y, 0.0, 6.0)
    y.backward(gy.double())
    out = dict(y=y.detach(), dx=x64.grad)
    if w64 is not None:
        out.update(dw=w64.grad, db=b64.grad)
    if r64 is not None:
        out["dres"] = r64.grad
    if training and rm is not None:
        out.update(rm=rm64, rv=rv64)
    return out


def norm_reference(kind, x, w, b, gy, **kw):
    """Float64 reference of a normalisation case: torch's autograd values, the magnitudes of norm_model, and the proof that the two
    restatements are the same expression (they agree to 2^-5 of the metric's unit)."""
    mkw = {k: v for k, v in kw.items() if k not in ("scale", "size")}
    ref = norm_model(kind, x, w, b, gy, fd=F64, T=None, **mkw)
    auto = norm_autograd(kind, x, w, b, gy, **kw)
    for k, v in auto.items():
        s = scaled(ref[k], v, ref["mag"][k])
        assert s < 2.0 ** -5, (k, s)
        ref[k] = v
    for k in [k for k in ref["mag"] if k not in auto]:         # (no affine part: no dweight / dbias; no running buffers: no update)
        ref.pop(k, None), ref["mag"].pop(k)
    return ref


def pool_norm_model(x, w, b, gy, *, T, emulate=False, defect=None):
    """instance_norm_relu_pool: InstanceNorm -> ReLU -> max pool 3x3 / 2 / 1 with the contract of the two-operator sequence, which
    the fused kernels keep on purpose (csrc/resize_pool.hip pool_norm_bwd_kernel): the gradient of the pool's input -- the sum of
    the up to four pooled gradients routed to a pixel -- is rounded to T, as maxpool_bwd_kernel stores it, before the
    normalisation's backward reads it.  That rounding is part of the operator, so it is part of the float64 reference too (the
    sum itself is exact in fp32: at most four T values of like magnitude); everything behind it is held to one rounding.
    emulate False: the float64 reference (values through torch's autograd); True: the fp32 emulation storing T."""
    fd, store = (F32, T) if emulate else (F64, None)
    inner = norm_model("in", x, w, b, torch.zeros_like(x), act="relu", fd=fd, T=store)
    zr = inner["y"].detach().clone().requires_grad_(True)
    yp = F.max_pool2d(zr, 3, 2, 1)
    (dz,) = torch.autograd.grad(yp, zr, gy.to(fd))
    dz = rt(dz, T).float()
    if emulate:
        out = norm_model("in", x, w, b, dz, act="relu", fd=fd, T=store, defect=defect)
    else:
        out = norm_reference("in", x, w, b, dz, act="relu")
        out["mag"]["y"] = F.max_pool2d(inner["mag"]["y"], 3, 2, 1)      # (an upper bound of the arg-max element's magnitude)
    out["y"] = yp.detach()
    return out


def designed_gy(kind, x, T, seed, tabs=None, m=0.5, k=0.7, noise=0.5):
    """round_T(m s1 + k s2 xhat + noise): an upstream gradient under which the statistic terms of the backward are a large part of dx."""
    B, C = x.shape[:2]
    up = _resize(x.double(), tabs)
    dims = (0, 2, 3) if kind == "bn" else (2, 3)
    xhat = (up - up.mean(dims, keepdim=True)) / (up.var(dims, unbiased=False, keepdim=True) + EPS).sqrt()
    sh = (1, C, 1, 1) if kind == "bn" else (B, C, 1, 1)
    g = torch.Generator().manual_seed(seed)
    nz = torch.randn(up.shape, generator=g).double() * noise
    return (m * signs(*sh, seed=seed + 1) + k * signs(*sh, seed=seed + 2) * xhat + nz).to(T).float()


def stat_share(ref):
    """max|dx - P*dy| / max|dx| of a float64 reference: the input condition (>= 0.25)."""
    return float(ref["stat"].abs().max() / ref["dx"].abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------
# NP+
# ---------------------------------------------------------------------------------------------------------------------------------
def np_model(x, alpha, noise, gy, *, res=None, fd=F64, T=None, defect=None):
    """NP+ as np_coef_kernel / np_bwd_coef_kernel state it: y = alpha x + (beta - alpha) mu (+ res), dx = alpha dy + K."""
    B, C, H, W = x.shape
    hw = float(H * W)
    roll = (lambda t: t.roll(1, 1)) if defect == "roll" else (lambda t: t)
    xs, g = x.to(fd), gy.to(fd)
    al, nz = alpha.float().to(fd).view(B, C), noise.float().to(fd).view(B, C)
    mu = (roll(xs.sum((2, 3)).double()) / hw).to(fd)
    mud = mu.double()
    mbar = mud.mean(0, keepdim=True)
    sigma = (((mud - mbar) ** 2).sum(0) / (B - 1.0)).sqrt().to(fd)
    M = sigma.max()
    scale = sigma / M * 1.5
    beta = 1.0 + nz * scale
    S = (beta - al) * mu
    y = xs * al.view(B, C, 1, 1) + S.view(B, C, 1, 1)
    r_ = res.to(fd) if res is not None else None
    if r_ is not None:
        y = y + r_
    out = dict(y=rt(y, T))
    red = g if defect != "lastline" else g[:, :, :-1]
    G = roll(red.sum((2, 3)).double()).to(fd).double()
    ald, nzd, sgd, Md = al.double(), nz.double(), sigma.double(), M.double()
    ds = (mud * G * nzd).sum(0)
    Tt = (ds * sgd).sum()
    dsig = 1.5 * ds / Md
    cstar = int(torch.nonzero(sigma == M)[0])
    dsig[cstar] -= 1.5 * Tt / (Md * Md)
    betad = 1.0 + nzd * (sgd / Md * 1.5)
    dmu = (betad - ald) * G + dsig * (mud - mbar) / ((B - 1.0) * sgd)
    K = (dmu / hw).to(fd)
    if defect == "k0":
        K = torch.zeros_like(K)
    dx = g * al.view(B, C, 1, 1) + K.view(B, C, 1, 1)
    out["dx"] = rt(dx, T)
    if res is not None:
        out["dres"] = rt(g, T)
    if defect == "lastvec":
        out = {k: _last_vec_zero(v, C) for k, v in out.items()}
    if fd == F64:
        out["mag"] = dict(y=(xs * al.view(B, C, 1, 1)).abs() + S.abs().view(B, C, 1, 1) + (r_.abs() if r_ is not None else 0.0),
                          dx=(g * al.view(B, C, 1, 1)).abs() + K.abs().view(B, C, 1, 1))
        if res is not None:
            out["mag"]["dres"] = g.abs()
        out["stat"] = K.view(B, C, 1, 1).expand_as(dx)
    return out


def np_reference(x, alpha, noise, gy, res=None):
    """oracle.mrfp_oracle.np_plus in float64 through autograd, with the magnitudes of np_model."""
    ref = np_model(x, alpha, noise, gy, res=res)
    x64 = x.double().clone().requires_grad_(True)
    r64 = res.double().clone().requires_grad_(True) if res is not None else None
    y = orc.np_plus(x64, alpha.float().double(), noise.float().double())
    y = y + r64 if r64 is not None else y
    y.backward(gy.double())
    auto = dict(y=y.detach(), dx=x64.grad)
    if r64 is not None:
        auto["dres"] = r64.grad
    for k, v in auto.items():
        assert scaled(ref[k], v, ref["mag"][k]) < 2.0 ** -5, k
        ref[k] = v
    return ref


def np_gy(shape, T, seed, offset=0.8, noise=0.5):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    return (offset * signs(B, C, 1, 1, seed=seed + 1) + torch.randn(shape, generator=g).double() * noise).to(T).float()


# ---------------------------------------------------------------------------------------------------------------------------------
# bilinear (align_corners), max pool, global average pool, add, channel scale
# ---------------------------------------------------------------------------------------------------------------------------------
def bilinear_model(x, size, gy, *, addend=None, channels=None, fd=F64, T=None):
    """F.interpolate(align_corners=True) of the first `channels` channels (+ addend); in float32 ATen's source position is the same
    fp32 product scale * dst the kernel forms (csrc/resize_pool.hip ac_tap)."""
    C = x.shape[1] if channels is None else channels
    xs = x.to(fd).clone().requires_grad_(True)
    y = orc.upsample_bilinear_ac(xs[:, :C], size)
    if addend is not None:
        y = y + addend.to(fd)
    (dx,) = torch.autograd.grad(y, xs, gy.to(fd))
    out = dict(y=rt(y.detach(), T), dx=rt(dx, T))
    if addend is not None:
        out["dadd"] = rt(gy.to(fd), T)
    if fd == F64:
        xa = x.double().abs().clone().requires_grad_(True)
        ya = orc.upsample_bilinear_ac(xa[:, :C], size)
        (da,) = torch.autograd.grad(ya, xa, gy.double().abs())
        out["mag"] = dict(y=ya.detach() + (addend.double().abs() if addend is not None else 0.0), dx=da)
        if addend is not None:
            out["mag"]["dadd"] = gy.double().abs()
    return out


def max_pool_model(x, gy, *, fd=F64, T=None):
    xs = x.to(fd).clone().requires_grad_(True)
    y = F.max_pool2d(xs, 3, 2, 1)
    (dx,) = torch.autograd.grad(y, xs, gy.to(fd))
    out = dict(y=rt(y.detach(), T), dx=rt(dx, T))
    if fd == F64:
        xa = x.double().clone().requires_grad_(True)
        (da,) = torch.autograd.grad(F.max_pool2d(xa, 3, 2, 1), xa, gy.double().abs())
        out["mag"] = dict(y=y.detach().abs(), dx=da)
    return out


def elementwise_model(a, b, m, gp, *, fd=F64, T=None):
    """global_avg_pool(a) and its backward for the pooled gradient gp, add(a, b), relu(add(a, b)), channel_scale(a, m) forward and
    backward (gradient b)."""
    B, C, H, W = a.shape
    a_, b_, m_ = a.to(fd), b.to(fd), m.float().to(fd).view(B, C, 1, 1)
    hw = float(H * W)
    out = dict(gap=rt((a_.sum((2, 3), keepdim=True).double() / hw).to(fd), T),
               gap_dx=rt((gp.to(fd) / torch.tensor(hw, dtype=fd)).expand(B, C, H, W), T),
               add=rt(a_ + b_, T), relu_add=rt((a_ + b_).clamp_min(0.0), T), cs=rt(a_ * m_, T), cs_dx=rt(b_ * m_, T))
    if fd == F64:
        out["mag"] = dict(gap=a_.abs().sum((2, 3), keepdim=True) / hw, gap_dx=(gp.double().abs() / hw).expand(B, C, H, W),
                          add=a_.abs() + b_.abs(), relu_add=a_.abs() + b_.abs(), cs=(a_ * m_).abs(), cs_dx=(b_ * m_).abs())
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases.  Channel counts select every lane layout of csrc/common.hpp make_lanes / pick_vec for 2-byte types: 8 (one vector, 256
# row threads), 24 (3 column threads: 85 row threads and one idle thread), 48, 64, 2048 (256 vectors = kThreads), 19 and 12 (scalar
# path).  Lines and widths are few and odd.
# ---------------------------------------------------------------------------------------------------------------------------------
BN_SHAPES = [(2, 8, 7, 5), (3, 24, 1, 23), (2, 48, 17, 1), (2, 64, 7, 31), (2, 2048, 1, 5), (3, 19, 7, 23), (2, 12, 17, 5)]
BN_COMBOS = [(False, False), (True, False), (False, True), (True, True)]             # (relu, res)
IN_SHAPES = [(1, 8, 7, 5), (3, 24, 1, 23), (2, 48, 17, 5), (3, 64, 7, 31), (1, 2048, 1, 5), (3, 19, 7, 23), (2, 12, 17, 1)]
IN_COMBOS = [(True, False), (True, True), (False, False), (False, True)]             # (affine, relu)
IN_COMBO_IDS = ["affine", "affine_relu", "plain", "plain_relu"]


def in_cases(shapes, combos, swap):
    """(shape, affine, relu) of the InstanceNorm cases.  ReLU without the affine part gates on (x - m) * a alone, and 16-bit inputs
    at the stem's magnitudes are integer-spaced: a plane's mean is now and then itself an input value, a pre-activation of exactly
    zero that settle() has to move.  Over 2048 planes of 5 (bf16) or 20 pixels no draw stays under the cap of one or two moved
    elements, so that one combination takes the shape of `swap` (more pixels per plane, same channel count) at C = 2048."""
    return [(swap.get(s, s) if (relu and not affine) else s, affine, relu) for s in shapes for affine, relu in combos]


def in_case_id(c):
    return "%s-%s" % (sid(c[0]), IN_COMBO_IDS[IN_COMBOS.index((c[1], c[2]))])


NP_SHAPES = [(2, 8, 7, 5), (4, 24, 1, 23), (16, 48, 7, 5), (2, 64, 17, 31), (2, 2048, 1, 5), (4, 19, 7, 23), (2, 12, 17, 1)]
RESIZE_CASES = {"up": ((2, 24, 12, 12), dict(scale=1.205)), "down": ((2, 64, 20, 20), dict(scale=0.798)),
                "up_c19": ((2, 19, 12, 12), dict(scale=1.205)), "size": ((3, 8, 7, 5), dict(size=(17, 7)))}
BILINEAR_CASES = {"up2": ((2, 24, 7, 5), (14, 10), None), "up4": ((1, 8, 5, 7), (20, 28), None), "up_odd": ((3, 64, 7, 5), (17, 23), None),
                  "src1x1": ((2, 48, 1, 1), (7, 5), None), "identity": ((2, 12, 7, 5), (7, 5), None), "down": ((2, 8, 17, 23), (7, 5), None),
                  "pad24": ((2, 24, 7, 5), (17, 23), 19), "pad32": ((1, 32, 5, 5), (10, 10), 19), "c2048": ((1, 2048, 1, 5), (3, 7), None)}
POOL_SHAPES = [(2, 8, 16, 16), (2, 24, 17, 13), (1, 8, 1, 1), (2, 48, 2, 5), (3, 19, 7, 6), (1, 2048, 4, 5), (2, 64, 7, 31)]
IN_POOL_SHAPES = [(2, 8, 14, 16), (2, 24, 17, 13), (2, 48, 2, 5), (3, 19, 7, 6), (1, 2048, 4, 5), (2, 64, 7, 31)]
EW_SHAPES = [(2, 8, 7, 5), (3, 24, 1, 23), (2, 64, 17, 31), (1, 2048, 1, 5), (3, 19, 7, 23)]


def sid(shape):
    return "x".join(str(s) for s in shape)


IN_CASES = in_cases(IN_SHAPES, IN_COMBOS, {(1, 2048, 1, 5): (1, 2048, 7, 5)})
# (the plain pool case at C = 8 also takes another even-sized shape: on 14 x 16 its designed gradient leaves the statistic terms at
#  0.23 of dx, below the input condition of 0.25)
IN_POOL_CASES = in_cases(IN_POOL_SHAPES, [(True, True), (False, True)], {(1, 2048, 4, 5): (1, 2048, 4, 7), (2, 8, 14, 16): (2, 8, 10, 8)})


def bn_params(C, seed=0):
    g = torch.Generator().manual_seed(1000 + C + seed)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    return w, b, rm, rv


def bn_case(shape, T, relu, res, act=None):
    """Inputs of one BatchNorm training case (all rounded to T; x settled away from the gates), and its designed gy."""
    B, C, H, W = shape
    w, b, rm, rv = bn_params(C)
    r = rnd(*shape, seed=2, dtype=T) if res else None
    make = lambda k: rnd(*shape, seed=1 + 100 * k, scale=3.0, shift=1.5, dtype=T)
    act = act or ("relu" if relu else None)
    if act == "relu6":                          # outputs of about 2 +- 3: both gates cut a good part of the elements
        w, b = 2.0 * w, 2.0 + 10.0 * b
    x = make(0) if act is None else settled(make, T, norm_pre(w, b, r, (0, 2, 3), gates=(0.0, 6.0) if act == "relu6" else (0.0,)))
    gy = designed_gy("bn", x, T, seed=3)
    return dict(x=x, w=w, b=b, rm=rm, rv=rv, res=r, gy=gy, act=act)


def bn_eval_case(shape, T, relu):
    B, C, H, W = shape
    w, b, rm, rv = bn_params(C)
    rm = rm + 1.5
    rv = rv * 9.0
    make = lambda k: rnd(*shape, seed=1 + 100 * k, scale=3.0, shift=1.5, dtype=T)
    x = settled(make, T, norm_pre(w, b, None, None, stats=(rm, rv))) if relu else make(0)
    gy = designed_gy("bn", x, T, seed=3)
    return dict(x=x, w=w, b=b, rm=rm, rv=rv, gy=gy, act="relu" if relu else None)


def in_case(shape, T, affine, relu, pool=False):
    """InstanceNorm at the stem's magnitudes (inputs are 0..255: scale 50, shift 120)."""
    B, C, H, W = shape
    w, b, _, _ = bn_params(C, seed=1)
    if not affine:
        w = b = None
    if pool:
        # integers of magnitude < 256 (exact in T) whose order inside a window survives the normalisation's rounding
        make = lambda k: no_tie_planes(shape, seed=41 + 100 * k, spread=8) + 100.0
        assert torch.equal(make(0).to(T).float(), make(0))
    else:
        make = lambda k: rnd(*shape, seed=4 + 100 * k, scale=50.0, shift=120.0, dtype=T)
    x = settled(make, T, norm_pre(w, b, None, (2, 3))) if relu else make(0)
    if pool:
        # (the pooled shape: values of the window centres.  The pool routes them to a quarter of the pixels, so the plane sums
        #  are a quarter as large: the sign term leads and the noise is small, which keeps the statistic terms above their share)
        gy = designed_gy("in", x, T, seed=5, k=0.0, noise=0.1)[:, :, ::2, ::2].contiguous()
    else:
        gy = designed_gy("in", x, T, seed=5)
    return dict(x=x, w=w, b=b, gy=gy, act="relu" if relu else None)


def np_case(shape, T, with_res):
    B, C, H, W = shape
    x = (rnd(*shape, seed=6, scale=2.0) + rnd(B, C, 1, 1, seed=7, scale=3.0)).to(T).float()
    alpha, noise = 1 + 0.75 * rnd(B, C, 1, 1, seed=8), 0.75 * rnd(B, C, 1, 1, seed=9)
    r = rnd(*shape, seed=11, dtype=T) if with_res else None
    return dict(x=x, alpha=alpha, noise=noise, res=r, gy=np_gy(shape, T, seed=10))


def resize_case(name, T):
    shape, rs = RESIZE_CASES[name]
    B, C, H, W = shape
    tabs = nearest_tables(H, W, **rs)
    w = torch.randn(C, generator=torch.Generator().manual_seed(5)) * 0.5
    w = torch.where(w.abs() < 0.05, torch.full_like(w, 0.25), w)
    b = torch.zeros(C)
    make = lambda k: rnd(*shape, seed=11 + 100 * k, scale=2.0, shift=0.3, dtype=T)

    def pre(v):      # the statistics are those of the RESIZED tensor; every resized pixel is a source pixel, gated as x*A + S
        up = _resize(v, tabs)
        m, var = up.mean((0, 2, 3)), up.var((0, 2, 3), unbiased=False)
        return norm_pre(w, b, None, None, stats=(m, var))(v)
    x = settled(make, T, pre)
    gy = designed_gy("bn", x, T, seed=12, tabs=tabs)
    return dict(x=x, w=w, b=b, gy=gy, act="relu", tabs=tabs, **rs)


def bilinear_case(name, T):
    shape, size, channels = BILINEAR_CASES[name]
    B, ld, Hi, Wi = shape
    C = ld if channels is None else channels
    return dict(x=rnd(*shape, seed=13, dtype=T), size=size, channels=channels, addend=rnd(B, C, *size, seed=14, dtype=T),
                gy=rnd(B, C, *size, seed=15, dtype=T))


def pool_case(shape, T):
    x = no_tie_planes(shape, seed=16)
    assert torch.equal(x.to(T).float(), x)
    cnt, _ = window_max_count(x.double())
    assert int(cnt.max()) == 1                                    # a tie is a property of the input, not a kernel error
    B, C, H, W = shape
    return dict(x=x, gy=rnd(B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, seed=17, dtype=T))


def ew_case(shape, T):
    B, C, H, W = shape
    return dict(a=rnd(*shape, seed=20, scale=2.0, shift=0.5, dtype=T), b=rnd(*shape, seed=21, dtype=T),
                m=(torch.rand(B, C, generator=torch.Generator().manual_seed(22)) < 0.7).float() / 0.7,
                gp=rnd(B, C, 1, 1, seed=19, dtype=T))


def worst(outs, ref, T, keys=None):
    """{output: scaled value} of a set of results against a reference (fp32 reduction outputs without the u_T term)."""
    res = {}
    for k in (keys or [k for k in outs if k in ref["mag"]]):
        res[k] = scaled(outs[k], ref[k], ref["mag"][k], None if k in ("dw", "db", "rm", "rv") else T)
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# every case of every operator: (operator of C_F32, case id, float64 reference, emulate(defect) -> outputs, defects that apply)
# ---------------------------------------------------------------------------------------------------------------------------------
def _norm_entry(op, cid, kind, c, T, defects, **kw):
    c = dict(c)
    args = (kind, c.pop("x"), c.pop("w"), c.pop("b"), c.pop("gy"))
    mk = {k: v for k, v in c.items() if k not in ("scale", "size")}
    mk.update(kw)
    ref = norm_reference(*args, **c, **kw)
    return op, cid, ref, (lambda defect=None: norm_model(*args, fd=F32, T=T, defect=defect, **mk)), defects


def all_cases(T):
    t = dname(T)
    for shape in BN_SHAPES:
        for relu, res in BN_COMBOS:
            d = [x for x in DEFECTS_NORM if x != "mult1" and (x != "gate_left" or relu) and (x != "double_round" or res)]
            yield _norm_entry("batch_norm", "bn-%s-relu%d-res%d-%s" % (sid(shape), relu, res, t), "bn", bn_case(shape, T, relu, res), T, d)
    for shape in BN_SHAPES[:4] + BN_SHAPES[5:6]:
        for relu in (False, True):
            yield _norm_entry("batch_norm_eval", "bneval-%s-relu%d-%s" % (sid(shape), relu, t), "bn", bn_eval_case(shape, T, relu), T, (),
                              training=False)
        yield _norm_entry("batch_norm_relu6", "bn6-%s-%s" % (sid(shape), t), "bn", bn_case(shape, T, False, False, act="relu6"), T,
                          ("qr0", "gate_left", "lastline"))
    for name in RESIZE_CASES:
        yield _norm_entry("batch_norm_resize", "resize-%s-%s" % (name, t), "bn", resize_case(name, T), T, ("qr0", "mult1", "lastline"))
    for shape, affine, relu in IN_CASES:
        d = [x for x in ("qr0", "roll", "lastline", "lastvec", "gate_left") if x != "gate_left" or relu]
        yield _norm_entry("instance_norm", "in-%s-affine%d-relu%d-%s" % (sid(shape), affine, relu, t), "in",
                          in_case(shape, T, affine, relu), T, d)
    for shape, affine, _ in IN_POOL_CASES:
        c = in_case(shape, T, affine, True, pool=True)
        a = (c["x"], c["w"], c["b"], c["gy"])
        yield ("instance_norm_relu_pool", "inpool-%s-affine%d-%s" % (sid(shape), affine, t), pool_norm_model(*a, T=T),
               (lambda defect=None, a=a: pool_norm_model(*a, T=T, emulate=True, defect=defect)), ("qr0", "lastline"))
    for shape in NP_SHAPES:
        for with_res in (False, True):
            c = np_case(shape, T, with_res)
            ref = np_reference(**c)
            yield ("np_plus", "np-%s-res%d-%s" % (sid(shape), with_res, t), ref,
                   (lambda defect=None, c=c: np_model(fd=F32, T=T, defect=defect, **c)), DEFECTS_NP)
    for name in BILINEAR_CASES:
        for with_add in (False, True):
            c = bilinear_case(name, T)
            if not with_add:
                c["addend"] = None
            yield ("bilinear", "bilinear-%s-add%d-%s" % (name, with_add, t), bilinear_model(**c),
                   (lambda defect=None, c=c: bilinear_model(fd=F32, T=T, **c)), ())
    for shape in POOL_SHAPES:
        c = pool_case(shape, T)
        yield ("max_pool", "pool-%s-%s" % (sid(shape), t), max_pool_model(**c), (lambda defect=None, c=c: max_pool_model(fd=F32, T=T, **c)), ())
    for shape in EW_SHAPES:
        c = ew_case(shape, T)
        yield ("elementwise", "ew-%s-%s" % (sid(shape), t), elementwise_model(**c),
               (lambda defect=None, c=c: elementwise_model(fd=F32, T=T, **c)), ())


def gated_tail_case(shape, T, y1):
    """The residual tail behind a plain BatchNorm whose stored output y1 (float32 on the host) is the tail's residual: the tail's
    input (settled against that residual), its parameters, and an upstream gradient designed for the FIRST BatchNorm -- its gated
    gradient gy * [tail > 0] is what that layer's backward is held to."""
    B, C, H, W = shape
    w2, b2, rm2, rv2 = bn_params(C, seed=7)
    make = lambda k: rnd(*shape, seed=51 + 100 * k, scale=2.0, shift=-0.5, dtype=T)
    x2 = settled(make, T, norm_pre(w2, b2, y1, (0, 2, 3)))
    return dict(x=x2, w=w2, b=b2, rm=rm2, rv=rv2, res=y1, act="relu")
