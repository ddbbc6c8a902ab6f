"""Depthwise 3x3 convolution (csrc/conv_dw.hip through ops.depthwise_conv2d) and the BatchNorm + ReLU6 apply on the GPU.

Against F.conv2d(groups=C) / F.batch_norm + F.hardtanh evaluated in fp64 on the CPU from the same (dtype-rounded) inputs.
Tolerances (max abs error over max abs reference): fp32 1e-3; bf16 / fp16 2e-2 -- the output is stored in the 16-bit type
(bf16: 2^-8 relative rounding) and the weight gradient sums bf16 products over every pixel of the batch.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mrfp_amd import _lib, conv, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
TOL = {torch.float32: 1e-3, torch.bfloat16: 2e-2, torch.float16: 2e-2}


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _case(B, C, H, W, stride, dil, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g).to(dtype)
    w = (torch.randn(C, 1, 3, 3, generator=g) / 3.0)
    gy_shape = (B, C, (H - 1) // stride + 1, (W - 1) // stride + 1)
    gy = torch.randn(*gy_shape, generator=g).to(dtype)
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    y = ops.depthwise_conv2d(xd, wd, None, stride, dil, dil)
    y.backward(gy.to(DEV).contiguous(memory_format=CL))
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, stride, dil, dil, C)
    y64.backward(gy.double())
    return y, xd.grad, wd.grad, y64, x64.grad, w64.grad


SHAPES = [(1, 1, 1), (7, 33, 1), (47, 29, 1), (16, 16, 2), (7, 33, 2), (47, 29, 4), (1, 1, 2), (9, 9, 4)]
CASES = [(B, C, H, W, s, d, dt)
         for dt in (torch.float32, torch.bfloat16)
         for C in (8, 24, 32, 96, 144, 960)
         for (H, W, d) in SHAPES[:4] if not (C == 960 and H > 16)
         for s in (1, 2)
         for B in ((1, 3) if C in (24, 144) else (3,))]
CASES += [(2, 12, 13, 11, s, d, torch.bfloat16) for s in (1, 2) for d in (1, 2)]      # Cphys 16 > C
CASES += [(2, 6, 13, 11, 2, 1, torch.float32), (2, 20, 9, 10, 1, 4, torch.float16), (3, 96, 47, 29, 2, 4, torch.float16),
          (1, 32, 7, 33, 2, 2, torch.float16), (2, 40, 1, 1, 2, 1, torch.bfloat16)]


@pytest.mark.parametrize("B,C,H,W,stride,dil,dtype", CASES)
def test_dwconv_fwd_dgrad_wgrad_vs_fp64(B, C, H, W, stride, dil, dtype):
    y, dx, dw, y64, dx64, dw64 = _case(B, C, H, W, stride, dil, dtype)
    tol = TOL[dtype]
    assert tuple(y.shape) == tuple(y64.shape) and y.dtype == dtype
    assert relerr(y, y64) < tol
    assert relerr(dx, dx64) < tol
    assert relerr(dw, dw64) < tol


def test_dgrad_pad_channels_are_zero():
    B, C, H, W, Cp = 2, 12, 9, 7, 16
    dtype = torch.bfloat16
    dy = torch.randn(B, H, W, Cp, device=DEV).to(dtype)          # pad channels of dy hold garbage
    w = torch.randn(C, 1, 3, 3, device=DEV)
    dx = torch.full((B, H, W, Cp), 7.0, device=DEV, dtype=dtype)
    _lib.call("mrfp_dwconv_dgrad", dy.data_ptr(), w.data_ptr(), dx.data_ptr(), _lib.BF16, B, H, W, Cp, C, H, W, 1, 1, _lib.stream())
    assert (dx[..., C:] == 0).all()
    ref = F.conv_transpose2d(dy[..., :C].permute(0, 3, 1, 2).double().cpu(), w.double().cpu(), None, 1, 1, 0, C)
    assert relerr(dx[..., :C].permute(0, 3, 1, 2), ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_statistics_equal_a_separate_pass(dtype):
    B, C, H, W = 3, 96, 47, 29
    x = torch.randn(B, C, H, W, device=DEV).to(dtype).contiguous(memory_format=CL)
    w = torch.randn(C, 1, 3, 3, device=DEV) / 3
    y = ops.depthwise_conv2d(x, w, None, 2, 1, 1)
    st = y._mrfp_colstats
    assert st.elements == B * y.shape[2] * y.shape[3] and st.final.numel() == st.final_count * 2 * C

    def finalize(ws, nb, nslab):
        out = torch.empty(4 * C, device=DEV)
        _lib.call("mrfp_bn_finalize", ws.data_ptr(), nb, nslab, st.elements, C, None, None, 1e-5, 0.0, None, None,
                  out[:C].data_ptr(), out[C:2 * C].data_ptr(), out[2 * C:3 * C].data_ptr(), out[3 * C:].data_ptr(), _lib.stream())
        return out[:2 * C].cpu()

    fused = finalize(st.final, 1, st.final_count)
    nslab, ws = ops._stats_fwd(y, None)
    sep = finalize(ws, B, nslab)
    torch.testing.assert_close(fused, sep, rtol=2e-5, atol=1e-6)


def test_wgrad_and_statistics_bitwise_reproducible():
    B, C, H, W = 3, 144, 47, 29
    x = torch.randn(B, C, H, W, device=DEV).to(torch.bfloat16).contiguous(memory_format=CL)
    gy = torch.randn(B, C, H, W, device=DEV).to(torch.bfloat16).contiguous(memory_format=CL)
    outs = []
    for _ in range(2):
        w = (torch.randn(C, 1, 3, 3, generator=torch.Generator().manual_seed(1)) / 3).to(DEV).requires_grad_(True)
        y = ops.depthwise_conv2d(x, w, None, 1, 2, 2)
        rows = y._mrfp_colstats.final.clone()
        y.backward(gy)
        outs.append((w.grad.clone(), rows, y.detach().clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][2], outs[1][2])


def test_hipconv2d_routes_depthwise():
    from mrfp_amd.network.mynn import HipConv2d
    m = HipConv2d(32, 32, 3, stride=2, padding=2, dilation=2, groups=32, bias=False).to(DEV)
    x = torch.randn(2, 32, 17, 15, device=DEV).contiguous(memory_format=CL)
    ref = F.conv2d(x.double().cpu(), m.weight.double().cpu(), None, 2, 2, 2, 32)
    assert relerr(m(x), ref) < 1e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_relu6_gate_at_the_boundaries(dtype):
    C = 8
    vals = torch.tensor([-0.03125, 0.0, 0.03125, 5.96875, 6.0, 6.03125, 3.0, -6.0])
    x = vals.reshape(1, 1, 1, 8).repeat(2, C, 3, 1)          # [2, C, 3, 8]: every channel sees every value along W
    x = x.to(dtype).to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    w = torch.ones(C, device=DEV, requires_grad=True)
    b = torch.zeros(C, device=DEV, requires_grad=True)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y = ops.batch_norm_relu6(x, w, b, rm, rv, training=False)
    gy = torch.ones_like(y)
    y.backward(gy)
    A = 1.0 / np.sqrt(1.0 + 1e-5)
    pre = x.detach().double().cpu() * A
    gate = ((pre > 0) & (pre < 6)).double()
    ref_y = pre.clamp(0, 6).to(dtype).double()
    torch.testing.assert_close(y.detach().double().cpu(), ref_y, rtol=1e-6, atol=0)
    # the 6.0 input: pre-activation 5.99997 -- stored as 6.0 in bf16, yet the gate passes
    assert gate[0, :, 0, 4].eq(1).all() and gate[0, :, 0, 5].eq(0).all() and gate[0, :, 0, 1].eq(0).all()
    torch.testing.assert_close(x.grad.double().cpu(), (gate * A).to(dtype).double(), rtol=1e-2 if dtype != torch.float32 else 1e-6,
                               atol=0)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 2e-2)])
def test_batch_norm_relu6_train_vs_fp64(dtype, tol):
    B, C, H, W = 2, 24, 9, 11
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(B, C, H, W, generator=g) * 3 + 2).to(dtype)
    w = torch.rand(C, generator=g) + 0.5
    b = torch.randn(C, generator=g)
    gy = torch.randn(B, C, H, W, generator=g).to(dtype)
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y = ops.batch_norm_relu6(xd, wd, bd, rm, rv, training=True)
    y.backward(gy.to(DEV).contiguous(memory_format=CL))
    x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    rm64, rv64 = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    y64 = F.hardtanh(F.batch_norm(x64, rm64, rv64, w64, b64, True, 0.1, 1e-5), 0.0, 6.0)
    y64.backward(gy.double())
    assert relerr(y, y64) < tol
    assert relerr(xd.grad, x64.grad) < 5 * tol
    assert relerr(wd.grad, w64.grad) < 5 * tol and relerr(bd.grad, b64.grad) < 5 * tol
    assert relerr(rm, rm64) < 1e-4 and relerr(rv, rv64) < 1e-4
