"""The MoE expert FFN forward as two grouped-GEMM custom ops.

    moe_expert_up(x, w1, w3, valid)  -> (h, a, b)
        a = x @ w1, b = x @ w3, h = silu(a) * b      per expert
    moe_expert_gemm(x, w, valid)     -> x @ w         per expert

with x [E, R, K] (R capacity rows per expert), weights [E, K, N] and outputs
[E, R, N].  `valid` is the optional [E, R] bool occupancy that moe_bins
returns.  Contract on x: rows whose `valid` is False are zero (moe_bins
writes them so), hence so are their output rows, and an implementation may
skip them or not without changing the result.

On the GPU both ops run the moe_nn kernels of csrc/gemm_kernels.hip inside
this envelope: every operand bf16, contiguous, 16-byte aligned; K % 32 == 0,
N % 8 == 0; valid bool and contiguous.  One launch covers every (expert,
128-row tile, column tile); in moe_expert_up the x tile is staged once for
both products and h comes from the fp32 accumulators, rounded once (the
unfused chain rounds a and b to bf16 first); a and b are written because the
backward needs them.  A tile none of whose rows is valid is written as zeros
by the kernel without reading x or the weights.  No atomics, no workspace,
no host synchronisation; the launch goes to the current stream and records
into a captured graph.

Everything else, the CPU, and EASYDIST_MOE_HIP=0 (read at each call, as in
moe_ops.py) run aten: for fp32 and fp64 literally `bmm` and
`F.silu(a) * b`; for bf16 and fp16 the kernel's contract, the products in
fp32, h from the fp32 values, each output rounded once.  The aten path does
not look at `valid`.

Only the forward is a kernel.  The backward is written in existing ops:
swiglu_bwd (csrc/swiglu_kernels.hip) for (da, db), and bmm / baddbmm for
dx and the weight gradients.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .moe_ops import _kernels
from . import swiglu  # noqa: F401  (swiglu_bwd, used by the backward)

lib = torch.library.Library("easydist_amd", "FRAGMENT")
lib.define("moe_expert_up(Tensor x, Tensor w1, Tensor w3, Tensor? valid) "
           "-> (Tensor, Tensor, Tensor)")
lib.define("moe_expert_gemm(Tensor x, Tensor w, Tensor? valid) -> Tensor")

_EXACT = (torch.float32, torch.float64)


def _check(op, x, *weights, valid=None):
    """Shape contract, the same for every implementation and the fakes."""
    if x.dim() != 3 or any(
            w.dim() != 3 or w.shape[:2] != (x.shape[0], x.shape[2])
            or w.shape != weights[0].shape or w.dtype != x.dtype
            for w in weights):
        got = ", ".join(f"{tuple(t.shape)} {t.dtype}" for t in (x, *weights))
        raise ValueError(f"{op}: want x [E,R,K] and weights [E,K,N] of one "
                         f"dtype; got {got}")
    if valid is not None and (valid.dtype != torch.bool
                              or valid.shape != x.shape[:2]):
        raise ValueError(f"{op}: valid must be bool [E,R]; got "
                         f"{tuple(valid.shape)} {valid.dtype}")


def _up_impl(x, w1, w3, valid=None):
    _check("moe_expert_up", x, w1, w3, valid=valid)
    if x.dtype in _EXACT:
        a = torch.bmm(x, w1)
        b = torch.bmm(x, w3)
        return F.silu(a) * b, a, b
    xf = x.float()
    a = torch.bmm(xf, w1.float())
    b = torch.bmm(xf, w3.float())
    h = a * torch.sigmoid(a) * b
    return h.to(x.dtype), a.to(x.dtype), b.to(x.dtype)


def _gemm_impl(x, w, valid=None):
    _check("moe_expert_gemm", x, w, valid=valid)
    if x.dtype in _EXACT:
        return torch.bmm(x, w)
    return torch.bmm(x.float(), w.float()).to(x.dtype)


def _operand_ok(t):
    return (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()
            and t.data_ptr() % 16 == 0)


def _kernel_ok(x, valid, *weights):
    """The moe_nn kernels' envelope; anything outside goes to aten."""
    E, R, K = x.shape
    N = weights[0].shape[2]
    if not (E >= 1 and R >= 1 and K >= 32 and K % 32 == 0 and N >= 8
            and N % 8 == 0 and max(R, K, N) < 2 ** 31):
        return False
    if valid is not None and not (valid.is_cuda and valid.is_contiguous()):
        return False
    return all(_operand_ok(t) for t in (x, *weights))


def _up_cuda(x, w1, w3, valid=None):
    _check("moe_expert_up", x, w1, w3, valid=valid)
    ext = _kernels(_kernel_ok(x, valid, w1, w3))
    if ext is None:
        return _up_impl(x, w1, w3, valid)
    return ext.moe_expert_up(x, w1, w3, valid)


def _gemm_cuda(x, w, valid=None):
    _check("moe_expert_gemm", x, w, valid=valid)
    ext = _kernels(_kernel_ok(x, valid, w))
    if ext is None:
        return _gemm_impl(x, w, valid)
    return ext.moe_expert_gemm(x, w, valid)


lib.impl("moe_expert_up", _up_impl, "CPU")
lib.impl("moe_expert_up", _up_cuda, "CUDA")
lib.impl("moe_expert_gemm", _gemm_impl, "CPU")
lib.impl("moe_expert_gemm", _gemm_cuda, "CUDA")


@torch.library.register_fake("easydist_amd::moe_expert_up")
def _up_fake(x, w1, w3, valid=None):
    _check("moe_expert_up", x, w1, w3, valid=valid)
    shape = (x.shape[0], x.shape[1], w1.shape[2])
    return x.new_empty(shape), x.new_empty(shape), x.new_empty(shape)


@torch.library.register_fake("easydist_amd::moe_expert_gemm")
def _gemm_fake(x, w, valid=None):
    _check("moe_expert_gemm", x, w, valid=valid)
    return x.new_empty(x.shape[0], x.shape[1], w.shape[2])


def _up_setup(ctx, inputs, output):
    x, w1, w3, _ = inputs
    _, a, b = output
    ctx.save_for_backward(x, w1, w3, a, b)
    ctx.set_materialize_grads(False)   # a and b usually carry no gradient


def _up_backward(ctx, gh, ga, gb):
    x, w1, w3, a, b = ctx.saved_tensors
    if gh is not None:
        da, db = torch.ops.easydist_amd.swiglu_bwd(gh.contiguous(), a, b)
    else:
        da, db = torch.zeros_like(a), torch.zeros_like(b)
    if ga is not None:
        da = da + ga
    if gb is not None:
        db = db + gb
    dx = dw1 = dw3 = None
    if ctx.needs_input_grad[0]:
        dx = torch.baddbmm(torch.bmm(da, w1.transpose(1, 2)), db,
                           w3.transpose(1, 2))
    xt = x.transpose(1, 2)
    if ctx.needs_input_grad[1]:
        dw1 = torch.bmm(xt, da)
    if ctx.needs_input_grad[2]:
        dw3 = torch.bmm(xt, db)
    return dx, dw1, dw3, None


def _gemm_setup(ctx, inputs, output):
    x, w, _ = inputs
    ctx.save_for_backward(x, w)


def _gemm_backward(ctx, g):
    x, w = ctx.saved_tensors
    dx = torch.bmm(g, w.transpose(1, 2)) if ctx.needs_input_grad[0] else None
    dw = torch.bmm(x.transpose(1, 2), g) if ctx.needs_input_grad[1] else None
    return dx, dw, None


torch.library.register_autograd("easydist_amd::moe_expert_up", _up_backward,
                                setup_context=_up_setup)
torch.library.register_autograd("easydist_amd::moe_expert_gemm",
                                _gemm_backward, setup_context=_gemm_setup)


def moe_expert_up(x, w1, w3, valid=None):
    """(silu(x @ w1) * (x @ w3), x @ w1, x @ w3) per expert."""
    return torch.ops.easydist_amd.moe_expert_up(x, w1, w3, valid)


def moe_expert_gemm(x, w, valid=None):
    """x @ w per expert."""
    return torch.ops.easydist_amd.moe_expert_gemm(x, w, valid)
