"""Fourier amplitude perturbation (north_star extension; PARITY UNPINNED: no reference function
exists) -- HIP kernels against the CPU oracle built on torch.fft, forward and backward."""
import pytest
import torch

from oracle import mrfp_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


GENERIC, TWOSTEP, PAIR, DIRECT, MFMA = range(5)          # MRFP_FOURIER_ROUTE_* (include/mrfp_hip.h)


def routes(dtype, shape, radius, high):
    """((family, kb, tu, nh) of passes 0, 1, 2 as mrfp_fourier_route reports them, stored bins along W)."""
    import ctypes
    from mrfp_amd import _lib
    B, C, H, W = shape
    out = []
    for p in range(3):
        kb, tu, nh = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        k = _lib.lib().mrfp_fourier_route(_lib._DT[dtype], H, W, C, float(radius), int(high), p, ctypes.byref(kb), ctypes.byref(tu), ctypes.byref(nh))
        out.append((k, kb.value, tu.value, nh.value))
    return out, int(_lib.lib().mrfp_fourier_stored_bins(H, W, float(radius), int(high)))


# what the comments of the case list below say about the kernels a case reaches, as assertions: {(shape, radius): check(dtype, routes, stored bins)}
_two_step = lambda dt, r, ws: all(k[0] != GENERIC for k in r) and r[1][0] == TWOSTEP
_direct = lambda dt, r, ws: r[2][0] == (MFMA if dt == torch.bfloat16 else DIRECT) and r[0][0] == (MFMA if dt == torch.bfloat16 else PAIR)
CLAIMS = {
    # two-step register path: every planned line length
    ((2, 16, 192, 192), 16.0): _two_step, ((2, 32, 128, 256), 20.0): _two_step, ((1, 16, 384, 512), 16.0): _two_step,
    ((2, 16, 32, 48), 5.0): _two_step, ((3, 16, 256, 64), 16.0): _two_step,
    # band-limited low-band path: floor(radius) + 1 stored columns; a radius past the last column: the whole half spectrum
    ((2, 16, 64, 64), 0.0): lambda dt, r, ws: ws == 1 and _two_step(dt, r, ws),
    ((3, 32, 64, 128), 3.5): lambda dt, r, ws: ws == 4 and r[0][0] == (MFMA if dt == torch.bfloat16 else PAIR),
    ((2, 16, 32, 48), 30.0): lambda dt, r, ws: ws == 25 and all(k[0] == TWOSTEP for k in r),
    ((2, 48, 128, 96), 24.0): lambda dt, r, ws: ws == 25 and all(k[0] == TWOSTEP for k in r),
    # 64-channel tiles: the inverse row pass as a direct trigonometric sum (bf16: both row passes on the matrix cores instead)
    ((2, 64, 96, 192), 16.0): _direct, ((2, 128, 64, 128), 5.5): _direct, ((1, 64, 32, 48), 3.0): _direct, ((2, 64, 48, 32), 0.0): _direct,
    # bf16 on the matrix cores: two k blocks, 32-channel items, a line longer than one LDS segment (W / 16 = 24 tiles in segments of 8)
    ((2, 64, 64, 96), 10.0): lambda dt, r, ws: dt != torch.bfloat16 or (r[0][:2] == (MFMA, 2) and r[2][:2] == (MFMA, 2)),
    ((2, 96, 96, 96), 12.0): lambda dt, r, ws: dt != torch.bfloat16 or (r[0][0] == MFMA and r[2] == (MFMA, 2, 6, 1)),
    ((1, 32, 48, 384), 16.0): lambda dt, r, ws: dt != torch.bfloat16 or (r[0] == (MFMA, 3, 8, 0) and r[2][0] == MFMA),
}


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,radius,lam,high", [((2, 16, 8, 8), 2.0, 1.0, False), ((3, 32, 48, 64), 6.0, 1.0, False),
                                                   ((2, 64, 64, 64), 16.0, 0.5, True), ((2, 16, 96, 192), 16.0, 1.0, False),
                                                   ((4, 16, 12, 18), 3.0, 0.7, True),
                                                   # two-step register path: every planned line length
                                                   ((2, 16, 192, 192), 16.0, 1.0, False), ((2, 32, 128, 256), 20.0, 0.6, True),
                                                   ((1, 16, 384, 512), 16.0, 1.0, False), ((2, 16, 32, 48), 5.0, 1.0, True),
                                                   ((3, 16, 256, 64), 16.0, 0.3, True),
                                                   # band-limited low-band path (floor(radius)+1 stored columns): one bin,
                                                   # fractional radius, a radius past the last column (full spectrum)
                                                   ((2, 16, 64, 64), 0.0, 1.0, False), ((3, 32, 64, 128), 3.5, 0.8, False),
                                                   ((2, 16, 32, 48), 30.0, 1.0, False), ((2, 48, 128, 96), 24.0, 1.0, False),
                                                   # 64-channel tiles: inverse row pass as a direct trigonometric sum
                                                   ((2, 64, 96, 192), 16.0, 1.0, False), ((2, 128, 64, 128), 5.5, 0.7, False),
                                                   ((1, 64, 32, 48), 3.0, 1.0, False), ((2, 64, 48, 32), 0.0, 1.0, False),
                                                   # bf16: band-limited row passes on the matrix cores -- two k blocks (9..16 stored
                                                   # bins), 32-channel items (C % 64 != 0), a line longer than one LDS segment
                                                   ((2, 64, 64, 96), 10.0, 1.0, False), ((2, 96, 96, 96), 12.0, 0.5, False),
                                                   ((1, 32, 48, 384), 16.0, 1.0, False)])
def test_fourier_amplitude_mix(dtype, shape, radius, lam, high):
    from mrfp_amd import ops
    B, C, H, W = shape
    if (shape, radius) in CLAIMS:
        r, ws = routes(dtype, shape, radius, high)
        assert CLAIMS[shape, radius](dtype, r, ws), (r, ws)
    g = torch.Generator().manual_seed(H * W + C)
    x = torch.randn(*shape, generator=g) + 0.3
    if dtype == torch.bfloat16:
        x = x.bfloat16().float()
    perm = torch.randperm(B, generator=g)
    xc = x.clone().requires_grad_(True)
    yc = orc.fourier_amplitude_mix(xc, perm, radius, lam, high)
    gy = torch.randn(yc.shape, generator=g)
    yc.backward(gy)
    xd = x.to(DEV, dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    yd = ops.fourier_amplitude_mix(xd, perm, radius, lam, high)
    yd.backward(gy.to(DEV, dtype).contiguous(memory_format=torch.channels_last))
    tol = 2e-5 if dtype == torch.float32 else 1.5e-2
    assert relerr(yd, yc) < tol
    assert relerr(xd.grad, xc.grad) < tol


@pytest.mark.parametrize("shape,radius", [((4, 128, 96, 192), 16.0), ((2, 64, 64, 96), 10.0), ((2, 32, 48, 64), 5.0), ((2, 64, 32, 384), 16.0)])
def test_bf16_matrix_core_row_passes_stay_within_two_output_ulps(shape, radius):
    """The bf16 band-limited path forms its row sums with MFMA products of split-bf16 factors (csrc/fft.hip).  Against the fp32
    definition evaluated with torch.fft on the SAME bf16 input: every output within 2.5 ulps of ITS OWN magnitude (bf16: 2^-8
    relative), more than 99 % of them the correctly rounded value -- what the fp32 direct-sum path delivers (tools/fourier_ab.py
    prints both; the loose norm-relative bound of the parametrised test above would not see a lost low-order part)."""
    from mrfp_amd import ops
    B, C, H, W = shape
    r, _ = routes(torch.bfloat16, shape, radius, False)
    assert r[0][0] == MFMA and r[2][0] == MFMA, r
    g = torch.Generator().manual_seed(7 * H + W)
    x = (torch.randn(*shape, generator=g) * 3 + 1).to(DEV, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    perm = torch.roll(torch.arange(B), 1)
    y = ops.fourier_amplitude_mix(x, perm, radius, 1.0, False)
    xf = x.float()
    F = torch.fft.rfft2(xf)
    A = F.abs()
    kh = torch.arange(H, device=DEV)
    dh = torch.minimum(kh, H - kh).float()
    kw = torch.arange(W // 2 + 1, device=DEV).float()
    band = (dh[:, None] ** 2 + kw[None, :] ** 2) <= radius * radius
    rat = torch.where(band[None, None] & (A > 1e-20), A[perm.to(DEV)] / A.clamp_min(1e-30), torch.ones_like(A))
    ref = torch.fft.irfft2(F * rat, s=(H, W))
    err = (y.float() - ref).abs() / (ref.abs().clamp_min(1e-2) * 2.0 ** -8)
    assert err.max().item() < 2.5, err.max().item()
    assert (y == ref.to(torch.bfloat16)).float().mean().item() > 0.99


def test_identity_when_partner_is_self():
    from mrfp_amd import ops
    x = torch.randn(2, 16, 24, 32).to(DEV).contiguous(memory_format=torch.channels_last)
    y = ops.fourier_amplitude_mix(x, torch.arange(2), 8.0, 1.0, False)
    assert relerr(y, x) < 1e-5


def test_unsupported_length_fails_loudly():
    from mrfp_amd import _lib, ops
    x = torch.randn(1, 16, 10, 14).to(DEV).contiguous(memory_format=torch.channels_last)   # 14 = 2*7
    assert _lib.lib().mrfp_fourier_route(0, 10, 14, 16, 2.0, 0, 0, None, None, None) < 0
    with pytest.raises(_lib.MrfpHipError):
        ops.fourier_amplitude_mix(x, torch.arange(1), 2.0)


@pytest.mark.parametrize("trunk,size", [("resnet-50", 192), ("resnet-101", 256)])
def test_multi_resolution_injection_vs_oracle(trunk, size):
    """perturb.MultiResolutionFourier attached to MRFPPlus (after the stem, layer1 and layer2: three plane sizes, one partner
    permutation) against the oracle's restatement of the same injection (torch.fft), together with HRFP / NP+ (all toggles
    on): loss, every per-stage statistic and the head gradients, fp32, 1e-3.  BUILD-DEFINED: parity unpinned."""
    import contextlib
    import io
    import numpy as np
    from mrfp_amd import deepv3, synth
    from mrfp_amd.config import cfg
    from mrfp_amd.perturb import MultiResolutionFourier
    cfg.MODEL.ACT_DTYPE = torch.float32
    with contextlib.redirect_stdout(io.StringIO()):
        model = deepv3.MRFPPlus(19, trunk=trunk, criterion=torch.nn.CrossEntropyLoss(ignore_index=255))
    sd = synth.synth_state_dict(synth.spec_of(model.state_dict()), seed=0, residual_gain=0.3)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    B = 4
    x, y = synth.synth_batch(B, size, size, seed=91)
    noise = synth.synth_noise(B, seed=92, channels=(64 if trunk == "resnet-50" else 128, 256))
    fp = MultiResolutionFourier(radii=(6.0, 6.0, 3.0), lam=0.8)
    fp.perm = torch.tensor([2, 0, 3, 1])
    model.fourier_perturb = fp
    model.rng = deepv3.InjectedRandom((True, True, True), noise)
    taps = {}
    model._taps = taps
    loss = model(x.to(DEV), y.to(DEV), training=True)
    loss.backward()
    model._taps = None
    keys = ["final2.0.weight", "final1.3.weight", "layer2.0.conv1.weight", "layer1.0.conv1.weight"]
    leaf = {k: sd[k].clone().requires_grad_(True) for k in keys}
    work = {k: v.clone() for k, v in sd.items()}
    work.update(leaf)
    otaps = {}
    lo = orc.mrfp_forward(work, x, y, training=True, toggles=(True, True, True), noise=noise, taps=otaps,
                          fourier={"perm": fp.perm, "levels": fp.spec()})
    assert abs(loss.item() - lo.item()) / lo.item() < 1e-3

    def st(t):
        t = t.detach().double().cpu()
        return np.array([t.abs().mean().item(), t.pow(2).sum().sqrt().item()])
    for name, t in taps.items():
        got, want = st(t.float()), st(otaps[name])
        assert np.abs(got / want - 1).max() < 1e-3, (name, got, want)
    # the perturbation really acted at all three resolutions (against a run without it)
    plain = {}
    with torch.no_grad():
        orc.mrfp_forward({k: v.clone() for k, v in sd.items()}, x, y, training=True, toggles=(True, True, True), noise=noise, taps=plain)
    for name in ("stem", "layer1", "layer2"):
        d = ((otaps[name] - plain[name]).double().norm() / plain[name].double().norm()).item()
        assert d > 1e-2, (name, d)
    grads = torch.autograd.grad(lo, [leaf[k] for k in keys])
    params = dict(model.named_parameters())
    for k, g in zip(keys, grads):
        r = g.double().norm().item()
        assert abs(params[k].grad.double().norm().item() - r) / r < 2e-2, k      # gradients flow through the mix (ratio detached)
    # eval: nothing happens
    model.eval()
    with torch.no_grad():
        l1 = model(x.to(DEV), training=False)
        model.fourier_perturb = None
        l0 = model(x.to(DEV), training=False)
    assert torch.equal(l0, l1)
