"""Fused SwiGLU activation as a custom op pair.

    swiglu(gate, up)           = silu(gate) * up
    swiglu_bwd(dy, gate, up)   = (d gate, d up)

with s = sigmoid(gate):  d gate = dy * up * s * (1 + gate * (1 - s)) and
d up = dy * gate * s.  The backward recomputes s from `gate`, so autograd
saves the two inputs only: the silu(gate) activation that the aten chain
`F.silu(a) * b` keeps alive from forward to backward is never written.

The HIP kernels (csrc/swiglu_kernels.hip) take bf16 operands of one shape
whose last dim is contiguous, a multiple of 8 wide, and whose leading dims
collapse to one row stride that is a multiple of 8 (the two halves of one
[.., 2F] projection, a row slice, a column slice of a wider buffer), with
16-byte aligned data; fp32 math, one rounding, contiguous outputs.
Everything else and the CPU run aten: for fp32 and fp64 literally
`F.silu(gate) * up` and aten's own silu_backward and mul, so that a graph
rewritten to these ops computes the same bits as before; for bf16 and fp16
the kernel's contract, the formulas above in fp32 rounded once.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import load_extension

lib = torch.library.Library("easydist_amd", "FRAGMENT")
lib.define("swiglu(Tensor gate, Tensor up) -> Tensor")
lib.define("swiglu_bwd(Tensor grad, Tensor gate, Tensor up) "
           "-> (Tensor, Tensor)")

_EXACT = (torch.float32, torch.float64)


def _check(op, **tensors):
    """Shape contract, the same for every implementation and the fakes:
    one shape and one dtype, no broadcasting."""
    first = next(iter(tensors.values()))
    if any(t.shape != first.shape or t.dtype != first.dtype
           for t in tensors.values()):
        got = ", ".join(f"{n} {tuple(t.shape)} {t.dtype}"
                        for n, t in tensors.items())
        raise ValueError(f"{op}: operands must have one shape and dtype "
                         f"(no broadcasting); got {got}")


def _math(gate, up):
    if gate.dtype in _EXACT:
        return F.silu(gate) * up
    g = gate.float()
    return (g * torch.sigmoid(g) * up.float()).to(gate.dtype)


def _math_bwd(grad, gate, up):
    if gate.dtype in _EXACT:
        dup = grad * F.silu(gate)
        dgate = torch.ops.aten.silu_backward(grad * up, gate)
        return dgate, dup
    dy, g, u = grad.float(), gate.float(), up.float()
    s = torch.sigmoid(g)
    dgate = dy * u * s * (1.0 + g * (1.0 - s))
    dup = dy * g * s
    return dgate.to(gate.dtype), dup.to(gate.dtype)


def _row_stride(t):
    """The stride of t seen as [R, F] rows, or None when its leading dims
    do not collapse to one.  Dims of size 1 carry no stride."""
    stride, inner = None, 1
    for d in range(t.dim() - 2, -1, -1):
        if t.size(d) == 1:
            continue
        if stride is None:
            stride = t.stride(d)
        elif t.stride(d) != stride * inner:
            return None
        inner *= t.size(d)
    return t.size(-1) if stride is None else stride


def _kernel_ok(*tensors):
    """The HIP kernels' envelope; anything outside goes to the aten path."""
    first = tensors[0]
    if first.dim() < 1 or first.numel() == 0 or first.size(-1) % 8:
        return False
    for t in tensors:
        if t.dtype != torch.bfloat16 or t.shape != first.shape \
                or t.stride(-1) != 1 or t.storage_offset() % 8:
            return False
        rs = _row_stride(t)
        if rs is None or rs < 0 or rs % 8:
            return False
    return True


def _swiglu_cpu(gate, up):
    _check("swiglu", gate=gate, up=up)
    return _math(gate, up).contiguous()


def _swiglu_bwd_cpu(grad, gate, up):
    _check("swiglu_bwd", grad=grad, gate=gate, up=up)
    dgate, dup = _math_bwd(grad, gate, up)
    return dgate.contiguous(), dup.contiguous()


def _swiglu_cuda(gate, up):
    _check("swiglu", gate=gate, up=up)
    if _kernel_ok(gate, up):
        ext = load_extension()
        if ext is not None:
            return ext.swiglu_fwd(gate, up)
        from . import require_hip_ops
        require_hip_ops()   # raises when the extension should exist
    return _math(gate, up).contiguous()


def _swiglu_bwd_cuda(grad, gate, up):
    _check("swiglu_bwd", grad=grad, gate=gate, up=up)
    if _kernel_ok(grad, gate, up):
        ext = load_extension()
        if ext is not None:
            return ext.swiglu_bwd(grad, gate, up)
        from . import require_hip_ops
        require_hip_ops()
    dgate, dup = _math_bwd(grad, gate, up)
    return dgate.contiguous(), dup.contiguous()


lib.impl("swiglu", _swiglu_cpu, "CPU")
lib.impl("swiglu", _swiglu_cuda, "CUDA")
lib.impl("swiglu_bwd", _swiglu_bwd_cpu, "CPU")
lib.impl("swiglu_bwd", _swiglu_bwd_cuda, "CUDA")


@torch.library.register_fake("easydist_amd::swiglu")
def _swiglu_fake(gate, up):
    _check("swiglu", gate=gate, up=up)
    # a new contiguous tensor whatever the input strides
    return gate.new_empty(tuple(gate.shape))


@torch.library.register_fake("easydist_amd::swiglu_bwd")
def _swiglu_bwd_fake(grad, gate, up):
    _check("swiglu_bwd", grad=grad, gate=gate, up=up)
    return (gate.new_empty(tuple(gate.shape)),
            gate.new_empty(tuple(gate.shape)))


def _swiglu_backward(ctx, grad):
    gate, up = ctx.saved_tensors
    dgate, dup = torch.ops.easydist_amd.swiglu_bwd(grad, gate, up)
    return dgate, dup


def _swiglu_setup_ctx(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


torch.library.register_autograd("easydist_amd::swiglu", _swiglu_backward,
                                setup_context=_swiglu_setup_ctx)


def swiglu(gate, up):
    """silu(gate) * up for two tensors of one shape and dtype."""
    return torch.ops.easydist_amd.swiglu(gate, up)
