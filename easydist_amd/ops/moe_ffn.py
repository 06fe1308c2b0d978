"""The MoE expert FFN as grouped-GEMM custom ops.  The forward is two:

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

The backward is swiglu_bwd (csrc/swiglu_kernels.hip) for (da, db) and three
more grouped ops, which the autograd formulas of the two above call:

    moe_expert_dx(g1, w1, g2, w2, valid) -> g1 @ w1^T (+ g2 @ w2^T)
    moe_expert_dw(x, g, valid)           -> x^T @ g
    moe_expert_dw2(x, g1, g2, valid)     -> (x^T @ g1, x^T @ g2)

with g [E, R, N], w [E, K, N], dx [E, R, K], dw [E, K, N].  Contract: rows of
x and of g whose `valid` is False are zero (moe_bins and moe_combine_bwd
write them so, and swiglu_bwd of a zero gradient row is zero).  On the GPU
they run the moe_nt / moe_tn kernels of csrc/gemm_kernels.hip: bf16,
contiguous, 16-byte aligned; dx wants N % 32 == 0 (the reduce length) and
K % 8 == 0, dw wants K % 8 == 0, N % 8 == 0 and R <= 131072.  dx sums both
products in one fp32 accumulator and rounds once (bmm then baddbmm rounds
twice) and writes a tile without a valid row as zeros; dw reduces over the
capacity rows in 32-row steps, walks only the steps that hold a valid row,
and moe_expert_dw2 stages x once for both gradients.  Outside the envelope
they are bmm / baddbmm as above.
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
lib.define("moe_expert_dx(Tensor g1, Tensor w1, Tensor? g2, Tensor? w2, "
           "Tensor? valid) -> Tensor")
lib.define("moe_expert_dw(Tensor x, Tensor g, Tensor? valid) -> Tensor")
lib.define("moe_expert_dw2(Tensor x, Tensor g1, Tensor g2, Tensor? valid) "
           "-> (Tensor, Tensor)")

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


# ---- the backward ops -----------------------------------------------------
def _check_valid(op, valid, like):
    if valid is not None and (valid.dtype != torch.bool
                              or valid.shape != like.shape[:2]):
        raise ValueError(f"{op}: valid must be bool [E,R]; got "
                         f"{tuple(valid.shape)} {valid.dtype}")


def _check_dx(g1, w1, g2, w2, valid):
    """g [E,R,N] against w [E,K,N]; g2 and w2 come together, shaped alike."""
    ok = (g1.dim() == 3 and w1.dim() == 3 and w1.dtype == g1.dtype
          and (w1.shape[0], w1.shape[2]) == (g1.shape[0], g1.shape[2])
          and (g2 is None) == (w2 is None))
    if ok and g2 is not None:
        ok = (g2.shape == g1.shape and w2.shape == w1.shape
              and g2.dtype == w2.dtype == g1.dtype)
    if not ok:
        got = ", ".join("None" if t is None else f"{tuple(t.shape)} {t.dtype}"
                        for t in (g1, w1, g2, w2))
        raise ValueError("moe_expert_dx: want g [E,R,N] and w [E,K,N] of one "
                         f"dtype, g2 and w2 both or neither; got {got}")
    _check_valid("moe_expert_dx", valid, g1)


def _check_dw(op, x, *gs, valid=None):
    if x.dim() != 3 or any(g.dim() != 3 or g.shape[:2] != x.shape[:2]
                           or g.shape != gs[0].shape or g.dtype != x.dtype
                           for g in gs):
        got = ", ".join(f"{tuple(t.shape)} {t.dtype}" for t in (x, *gs))
        raise ValueError(f"{op}: want x [E,R,K] and g [E,R,N] of one dtype; "
                         f"got {got}")
    _check_valid(op, valid, x)


def _dx_impl(g1, w1, g2=None, w2=None, valid=None):
    _check_dx(g1, w1, g2, w2, valid)
    if g1.dtype in _EXACT:
        dx = torch.bmm(g1, w1.transpose(1, 2))
        return dx if g2 is None else torch.baddbmm(dx, g2, w2.transpose(1, 2))
    dx = torch.bmm(g1.float(), w1.float().transpose(1, 2))
    if g2 is not None:
        dx = torch.baddbmm(dx, g2.float(), w2.float().transpose(1, 2))
    return dx.to(g1.dtype)


def _dw_impl(x, g, valid=None):
    _check_dw("moe_expert_dw", x, g, valid=valid)
    if x.dtype in _EXACT:
        return torch.bmm(x.transpose(1, 2), g)
    return torch.bmm(x.float().transpose(1, 2), g.float()).to(x.dtype)


def _dw2_impl(x, g1, g2, valid=None):
    _check_dw("moe_expert_dw2", x, g1, g2, valid=valid)
    return _dw_impl(x, g1), _dw_impl(x, g2)


def _valid_ok(valid):
    return valid is None or (valid.is_cuda and valid.is_contiguous())


def _dx_kernel_ok(g1, w1, g2, w2, valid):
    """The moe_nt kernels' envelope; anything outside goes to aten."""
    E, R, N = g1.shape
    K = w1.shape[1]
    if not (E >= 1 and R >= 1 and N >= 32 and N % 32 == 0 and K >= 8
            and K % 8 == 0 and max(R, K, N) < 2 ** 31):
        return False
    return _valid_ok(valid) and all(
        _operand_ok(t) for t in (g1, w1, g2, w2) if t is not None)


def _dw_kernel_ok(x, valid, *gs):
    """The moe_tn kernels' envelope."""
    E, R, K = x.shape
    N = gs[0].shape[2]
    if not (E >= 1 and R >= 1 and K >= 8 and K % 8 == 0 and N >= 8
            and N % 8 == 0 and -(-R // 32) <= 4096 and max(K, N) < 2 ** 31):
        return False
    return _valid_ok(valid) and all(_operand_ok(t) for t in (x, *gs))


def _dx_cuda(g1, w1, g2=None, w2=None, valid=None):
    _check_dx(g1, w1, g2, w2, valid)
    ext = _kernels(_dx_kernel_ok(g1, w1, g2, w2, valid))
    if ext is None:
        return _dx_impl(g1, w1, g2, w2, valid)
    return ext.moe_expert_dx(g1, w1, g2, w2, valid)


def _dw_cuda(x, g, valid=None):
    _check_dw("moe_expert_dw", x, g, valid=valid)
    ext = _kernels(_dw_kernel_ok(x, valid, g))
    if ext is None:
        return _dw_impl(x, g, valid)
    return ext.moe_expert_dw(x, g, valid)


def _dw2_cuda(x, g1, g2, valid=None):
    _check_dw("moe_expert_dw2", x, g1, g2, valid=valid)
    ext = _kernels(_dw_kernel_ok(x, valid, g1, g2))
    if ext is None:
        return _dw2_impl(x, g1, g2, valid)
    return ext.moe_expert_dw2(x, g1, g2, valid)


lib.impl("moe_expert_dx", _dx_impl, "CPU")
lib.impl("moe_expert_dx", _dx_cuda, "CUDA")
lib.impl("moe_expert_dw", _dw_impl, "CPU")
lib.impl("moe_expert_dw", _dw_cuda, "CUDA")
lib.impl("moe_expert_dw2", _dw2_impl, "CPU")
lib.impl("moe_expert_dw2", _dw2_cuda, "CUDA")


@torch.library.register_fake("easydist_amd::moe_expert_dx")
def _dx_fake(g1, w1, g2=None, w2=None, valid=None):
    _check_dx(g1, w1, g2, w2, valid)
    return g1.new_empty(g1.shape[0], g1.shape[1], w1.shape[1])


@torch.library.register_fake("easydist_amd::moe_expert_dw")
def _dw_fake(x, g, valid=None):
    _check_dw("moe_expert_dw", x, g, valid=valid)
    return x.new_empty(x.shape[0], x.shape[2], g.shape[2])


@torch.library.register_fake("easydist_amd::moe_expert_dw2")
def _dw2_fake(x, g1, g2, valid=None):
    _check_dw("moe_expert_dw2", x, g1, g2, valid=valid)
    shape = (x.shape[0], x.shape[2], g1.shape[2])
    return x.new_empty(shape), x.new_empty(shape)


def _up_setup(ctx, inputs, output):
    x, w1, w3, valid = inputs
    _, a, b = output
    ctx.save_for_backward(x, w1, w3, a, b, valid)
    ctx.set_materialize_grads(False)   # a and b usually carry no gradient


def _up_backward(ctx, gh, ga, gb):
    x, w1, w3, a, b, valid = ctx.saved_tensors
    ed = torch.ops.easydist_amd
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
        dx = ed.moe_expert_dx(da, w1, db, w3, valid)
    if ctx.needs_input_grad[1] and ctx.needs_input_grad[2]:
        dw1, dw3 = ed.moe_expert_dw2(x, da, db, valid)
    elif ctx.needs_input_grad[1]:
        dw1 = ed.moe_expert_dw(x, da, valid)
    elif ctx.needs_input_grad[2]:
        dw3 = ed.moe_expert_dw(x, db, valid)
    return dx, dw1, dw3, None


def _gemm_setup(ctx, inputs, output):
    x, w, valid = inputs
    ctx.save_for_backward(x, w, valid)


def _gemm_backward(ctx, g):
    x, w, valid = ctx.saved_tensors
    ed = torch.ops.easydist_amd
    g = g.contiguous()
    dx = ed.moe_expert_dx(g, w, None, None, valid) \
        if ctx.needs_input_grad[0] else None
    dw = ed.moe_expert_dw(x, g, valid) if ctx.needs_input_grad[1] else None
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


def moe_expert_dx(g1, w1, g2=None, w2=None, valid=None):
    """g1 @ w1^T (+ g2 @ w2^T) per expert, summed in fp32, rounded once."""
    return torch.ops.easydist_amd.moe_expert_dx(g1, w1, g2, w2, valid)


def moe_expert_dw(x, g, valid=None):
    """x^T @ g per expert."""
    return torch.ops.easydist_amd.moe_expert_dw(x, g, valid)


def moe_expert_dw2(x, g1, g2, valid=None):
    """(x^T @ g1, x^T @ g2) per expert."""
    return torch.ops.easydist_amd.moe_expert_dw2(x, g1, g2, valid)
