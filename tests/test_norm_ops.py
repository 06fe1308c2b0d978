"""Op-level RMSNorm contract, on the CPU implementations.

rms_norm_bwd returns (dx in x's dtype, dw fp32 [D]) from the CPU impl and
from the fake alike, and dw is sum over rows of grad * xhat whether a weight
is given or not: that is what the HIP kernel produces, and the gradient
feeds an fp32 optimizer. RMSNorm(dim) is differentiable: x.grad and
weight.grad are held to fp64 autograd of the written-out formula.

Bounds (u16 = 2^-8, u32 = 2^-24, every term in fp64), the ones of
tests/test_gpu_norm_exact.py:
  dx  |dx - ref| <= rnd * |ref| + 1e-5 * r * (|gw| + |xhat * mean(gw*xhat)|),
      rnd = u16 for bf16, 16 * u32 for fp32 (one rounding of the result
      plus fp32 arithmetic on the terms)
  dw  |dw - ref| <= (rows + 8) * u32 * sum_r |g * xhat|  (any fp32 summation
      order plus the rounding of each term)
"""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import easydist_amd.ops  # noqa: F401  (registers the ops)
from easydist_amd.ops.norms import RMSNorm

U16, U32 = 2.0 ** -8, 2.0 ** -24
ROWS, D, EPS = 37, 72, 1e-6


def _inputs(dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = (1.5 * torch.randn(3, ROWS, D, generator=gen) + 0.25).to(dtype)
    g = torch.randn(3, ROWS, D, generator=gen).to(dtype)
    w = torch.randn(D, generator=gen)
    return x, g, w


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_w", [True, False])
def test_rms_norm_bwd_impl_and_fake_agree(dtype, with_w):
    x, g, w = _inputs(dtype)
    w = w if with_w else None
    _, rstd = torch.ops.easydist_amd.rms_norm_fwd(x, w, EPS)
    dx, dw = torch.ops.easydist_amd.rms_norm_bwd(g, x, rstd, w)
    with FakeTensorMode() as mode:
        f = lambda t: None if t is None else mode.from_tensor(t)
        fdx, fdw = torch.ops.easydist_amd.rms_norm_bwd(f(g), f(x), f(rstd),
                                                       f(w))
    assert dx.dtype == fdx.dtype == dtype
    assert dx.shape == fdx.shape == x.shape
    assert dw.dtype == fdw.dtype == torch.float32
    assert tuple(dw.shape) == tuple(fdw.shape) == (D,)

    # dw = sum g * xhat over every leading dim, with or without a weight
    x64, g64 = x.double(), g.double()
    xh = x64 * rstd.double()
    t = (g64 * xh).reshape(-1, D)
    bound = (t.shape[0] + 8) * U32 * t.abs().sum(0)
    assert bool(((dw.double() - t.sum(0)).abs() <= bound).all())


def _ref(x, g, w, eps):
    x64 = x.double().requires_grad_()
    w64 = w.double().requires_grad_()
    r = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + eps)
    out = x64 * r * w64
    out.backward(g.double())
    return out.detach(), x64.grad, w64.grad, r.detach()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rms_norm_module_differentiable(dtype):
    x, g, w = _inputs(dtype, seed=1)
    mod = RMSNorm(D, eps=EPS)
    with torch.no_grad():
        mod.weight.copy_(w)
    assert mod.weight.dtype == torch.float32
    xin = x.clone().requires_grad_()
    out = mod(xin)
    assert out.dtype == dtype and out.requires_grad
    out.backward(g)
    assert xin.grad is not None and xin.grad.dtype == dtype
    assert mod.weight.grad is not None
    assert mod.weight.grad.dtype == mod.weight.dtype
    assert mod.weight.grad.shape == mod.weight.shape

    out64, dx64, dw64, r = _ref(x, g, mod.weight.detach(), EPS)
    rnd = U16 if dtype == torch.bfloat16 else 16 * U32
    xh = x.double() * r
    gw = g.double() * mod.weight.detach().double()
    c2 = (gw * xh).mean(-1, keepdim=True)
    slack = 1e-5 * r * (gw.abs() + (xh * c2).abs())
    err = (xin.grad.double() - dx64).abs()
    bound = rnd * dx64.abs() + slack
    print(f"dx worst err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())

    t = (g.double() * xh).reshape(-1, D)
    wbound = (t.shape[0] + 8) * U32 * t.abs().sum(0)
    werr = (mod.weight.grad.double() - dw64).abs()
    print(f"dw worst err/bound {float((werr / wbound).max()):.3f}")
    assert bool((werr <= wbound).all())

    obound = rnd * out64.abs() + 1e-5 * out64.abs()
    assert bool(((out.detach().double() - out64).abs() <= obound).all())
