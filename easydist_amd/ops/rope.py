"""Rotary position embeddings (RoPE) as a custom op on the packed qkv.

`rope_qkv` rotates the q and k column blocks of the qkv projection output
[B, S, (H + 2*Hkv)*D] (columns [q | k | v], the layout the attention kernels
and the packed attention backward share) and copies the v columns through.
Convention is "rotate-half" (HuggingFace Llama/Mixtral, GPT-NeoX): for every
head h < H + Hkv and j < D/2, with lo = x[h*D + j], hi = x[h*D + D/2 + j],
c = cos[s, j], t = sin[s, j]

    out_lo = lo*c - hi*t        out_hi = hi*c + lo*t

`inverse=True` uses -t, the transpose of the rotation: the gradient of the op
with respect to qkv is the same op with `inverse` flipped, so one op serves
forward, backward and double backward.  The tables are tensor inputs, [S, D/2]:
position offsets (a sequence shard's rows, scaled variants) are the caller's.

The HIP kernel (csrc/rope_kernels.hip) takes bf16 qkv with a contiguous last
dim and 16-byte aligned rows, fp32 tables, D % 16 == 0 and D <= 256; one
memory-bound pass, fp32 math, one rounding.  Everything else and the CPU run
the same formula in aten, in fp32 at least (fp64 for fp64 input).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import load_extension

lib = torch.library.Library("easydist_amd", "FRAGMENT")
lib.define("rope_qkv(Tensor qkv, Tensor cos, Tensor sin, int n_head, "
           "int n_kv_head, bool inverse) -> Tensor")


def _check(qkv, cos, sin, n_head, n_kv_head):
    """Shape contract, the same for every implementation and the fake."""
    if qkv.dim() != 3 or cos.dim() != 2:
        raise ValueError(
            f"rope_qkv: qkv must be [B, S, W] and cos/sin [S, D/2]; got qkv "
            f"{tuple(qkv.shape)}, cos {tuple(cos.shape)}")
    if cos.shape != sin.shape:
        raise ValueError(
            f"rope_qkv: cos and sin must have one shape; got cos "
            f"{tuple(cos.shape)}, sin {tuple(sin.shape)}")
    if n_head < 1 or n_kv_head < 1:
        raise ValueError(
            f"rope_qkv: head counts must be positive; got n_head {n_head}, "
            f"n_kv_head {n_kv_head}")
    D = 2 * cos.shape[-1]
    if qkv.shape[2] != (n_head + 2 * n_kv_head) * D:
        raise ValueError(
            f"rope_qkv: qkv {tuple(qkv.shape)} is not (n_head + 2*n_kv_head)"
            f"*D = ({n_head} + 2*{n_kv_head})*{D} columns wide (D from cos "
            f"{tuple(cos.shape)})")
    if cos.shape[0] != qkv.shape[1]:
        raise ValueError(
            f"rope_qkv: cos/sin {tuple(cos.shape)} must have one row per "
            f"position of qkv {tuple(qkv.shape)}")
    # the tables never go through autocast (the op is on none of its lists):
    # a half-precision table here is a caller's cast, and loses the angles
    assert cos.dtype == sin.dtype and cos.dtype in (torch.float32,
                                                    torch.float64), \
        f"rope_qkv: cos/sin must be fp32 (or fp64), got {cos.dtype}, " \
        f"{sin.dtype}"


def _math(qkv, cos, sin, n_head, n_kv_head, inverse):
    D = 2 * cos.shape[-1]
    R = (n_head + n_kv_head) * D
    ct = torch.promote_types(torch.promote_types(qkv.dtype, cos.dtype),
                             torch.float32)
    x = qkv[..., :R].unflatten(-1, (n_head + n_kv_head, D)).to(ct)
    lo, hi = x[..., :D // 2], x[..., D // 2:]
    c = cos.to(ct)[None, :, None, :]
    t = sin.to(ct)[None, :, None, :]
    if inverse:
        t = -t
    rot = torch.cat((lo * c - hi * t, hi * c + lo * t), dim=-1)
    return torch.cat((rot.flatten(-2).to(qkv.dtype), qkv[..., R:]), dim=-1)


def _kernel_ok(qkv, cos, sin):
    """The HIP kernel's envelope; anything outside goes to the aten path."""
    D = 2 * cos.shape[-1]
    return (qkv.dtype == torch.bfloat16 and cos.dtype == torch.float32
            and sin.dtype == torch.float32
            and D % 16 == 0 and 16 <= D <= 256 and qkv.numel() > 0
            and qkv.stride(2) == 1
            and qkv.stride(0) >= 0 and qkv.stride(0) % 8 == 0
            and qkv.stride(1) >= 0 and qkv.stride(1) % 8 == 0
            and qkv.storage_offset() % 8 == 0
            and cos.storage_offset() % 4 == 0
            and sin.storage_offset() % 4 == 0)


def _rope_cpu(qkv, cos, sin, n_head, n_kv_head, inverse):
    _check(qkv, cos, sin, n_head, n_kv_head)
    return _math(qkv, cos, sin, n_head, n_kv_head, inverse)


def _rope_cuda(qkv, cos, sin, n_head, n_kv_head, inverse):
    _check(qkv, cos, sin, n_head, n_kv_head)
    ext = load_extension()
    if _kernel_ok(qkv, cos, sin):
        if ext is not None:
            return ext.rope_qkv(qkv, cos.contiguous(), sin.contiguous(),
                                n_head, n_kv_head, inverse)
        from . import require_hip_ops
        require_hip_ops()   # raises when the extension should exist
    return _math(qkv, cos, sin, n_head, n_kv_head, inverse)


lib.impl("rope_qkv", _rope_cpu, "CPU")
lib.impl("rope_qkv", _rope_cuda, "CUDA")


@torch.library.register_fake("easydist_amd::rope_qkv")
def _rope_fake(qkv, cos, sin, n_head, n_kv_head, inverse):
    _check(qkv, cos, sin, n_head, n_kv_head)
    # a new contiguous tensor whatever the input strides
    return qkv.new_empty(tuple(qkv.shape))


def _rope_backward(ctx, grad):
    cos, sin = ctx.saved_tensors
    dqkv = torch.ops.easydist_amd.rope_qkv(grad, cos, sin, ctx.n_head,
                                           ctx.n_kv_head, not ctx.inverse)
    return dqkv, None, None, None, None, None


def _rope_setup_ctx(ctx, inputs, output):
    _, cos, sin, n_head, n_kv_head, inverse = inputs
    ctx.save_for_backward(cos, sin)
    ctx.n_head, ctx.n_kv_head, ctx.inverse = n_head, n_kv_head, inverse


torch.library.register_autograd("easydist_amd::rope_qkv", _rope_backward,
                                setup_context=_rope_setup_ctx)


def rope_tables(seq_len: int, head_dim: int, base: float = 10000.0,
                device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 (cos, sin) of shape [seq_len, head_dim/2]: angles
    pos * base^(-2j/head_dim), computed in fp64 and cast once."""
    if head_dim % 2:
        raise ValueError(f"rope_tables: head_dim {head_dim} must be even")
    j = torch.arange(head_dim // 2, dtype=torch.float64)
    inv_freq = torch.pow(torch.tensor(float(base), dtype=torch.float64),
                         -2.0 * j / head_dim)
    ang = torch.arange(seq_len, dtype=torch.float64)[:, None] * inv_freq
    return (ang.cos().to(torch.float32).to(device),
            ang.sin().to(torch.float32).to(device))


def apply_rope(qkv, cos, sin, n_head: int, n_kv_head: Optional[int] = None):
    """Rotate the q and k columns of a packed qkv [B, S, (H + 2*Hkv)*D]."""
    if n_kv_head is None:
        n_kv_head = n_head
    return torch.ops.easydist_amd.rope_qkv(qkv, cos, sin, n_head, n_kv_head,
                                           False)
