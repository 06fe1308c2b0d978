"""Flash attention as a custom op: HIP kernels forward and backward on gfx950.

Forward: hand-written CDNA4 flash kernel (csrc/attn_kernels.hip) — online
softmax, MFMA 16x16x32 bf16 tiles, K/V staged through swizzled LDS images.
Backward: two hand-written kernels from the same file (dq, and dk+dv), which
recompute P from the saved LSE; `flash_attention_bwd_pack` writes the three
gradients straight into one [B, S, (H + 2*Hkv)*D] buffer.

The kernels take bf16 q [B, H, S, D] and k, v [B, Hkv, S, D] with
H % Hkv == 0, D in {64, 128}, any S >= 1 and any last-dim-contiguous
strides.  Hkv < H is grouped-query attention in torch's repeat_interleave
convention: with G = H // Hkv, query head h attends K/V head h // G; dk and
dv have K/V's shape, the sum over a group taken in fp32 inside the dkv
kernel and rounded once.  Everything else (Sq != Sk, other head dims or
dtypes) and the CPU run the same math in aten.  A query head count that is
no multiple of the K/V head count is an error everywhere: nothing
broadcasts.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch

from . import load_extension

lib = torch.library.Library("easydist_amd", "DEF")
lib.define("flash_attention(Tensor q, Tensor k, Tensor v, bool causal) "
           "-> (Tensor, Tensor)")
lib.define("flash_attention_bwd(Tensor grad, Tensor q, Tensor k, Tensor v, "
           "Tensor out, Tensor lse, bool causal) -> (Tensor, Tensor, Tensor)")
# packed variant: dq/dk/dv written straight into one [B, S, (H + 2*Hkv)*D]
# buffer, dq at column 0, dk at H*D, dv at (H + Hkv)*D
# (the qkv-projection-backward layout) — the lowering pass substitutes it
# for the flash_bwd -> transpose -> clone -> cat chain (lower_hip.py)
lib.define("flash_attention_bwd_pack(Tensor grad, Tensor q, Tensor k, "
           "Tensor v, Tensor out, Tensor lse, bool causal) -> Tensor")


def _group(q, k, v):
    """G = H // Hkv of q [B, H, S, D] and k, v [B, Hkv, T, D]."""
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        return 1        # no head dim to group: plain matmul semantics
    H, Hkv = q.shape[1], k.shape[1]
    if v.shape[1] != Hkv or Hkv < 1 or H % Hkv != 0:
        raise ValueError(
            f"flash_attention: {H} query heads need a K/V head count that "
            f"divides them, the same for k and v; got k {tuple(k.shape)}, "
            f"v {tuple(v.shape)}")
    return H // Hkv


def _expand_kv(t, G):
    # [B, Hkv, T, D] -> [B, Hkv * G, T, D], head h <- head h // G
    return t if G == 1 else t.repeat_interleave(G, dim=1)


def _reduce_kv(d, G, dtype):
    # fp32 [B, Hkv * G, T, D] -> [B, Hkv, T, D]: the group sum in fp32,
    # one rounding
    if G > 1:
        B, H, T, D = d.shape
        d = d.view(B, H // G, G, T, D).sum(2)
    return d.to(dtype)


def _math_fwd(q, k, v, causal):
    # q: [B, H, S, D]; k,v: [B, Hkv, T, D]
    G = _group(q, k, v)
    k, v = _expand_kv(k, G), _expand_kv(v, G)
    scale = 1.0 / math.sqrt(q.shape[-1])
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    if causal:
        S, T = s.shape[-2], s.shape[-1]
        mask = torch.ones(S, T, dtype=torch.bool, device=s.device).tril()
        s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    out = torch.matmul(p.to(v.dtype), v)
    return out, lse


def _math_bwd(grad, q, k, v, out, lse, causal):
    G = _group(q, k, v)
    kdt, vdt = k.dtype, v.dtype
    k, v = _expand_kv(k, G), _expand_kv(v, G)
    scale = 1.0 / math.sqrt(q.shape[-1])
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    if causal:
        S, T = s.shape[-2], s.shape[-1]
        mask = torch.ones(S, T, dtype=torch.bool, device=s.device).tril()
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.exp(s - lse.unsqueeze(-1).float())
    gradf = grad.float()
    dv = torch.matmul(p.transpose(-1, -2), gradf)
    dp = torch.matmul(gradf, v.float().transpose(-1, -2))
    d = (gradf * out.float()).sum(-1, keepdim=True)
    ds = p * (dp - d) * scale
    dq = torch.matmul(ds, k.float())
    dk = torch.matmul(ds.transpose(-1, -2), q.float())
    return dq.to(q.dtype), _reduce_kv(dk, G, kdt), _reduce_kv(dv, G, vdt)


def _fwd_cpu(q, k, v, causal):
    return _math_fwd(q, k, v, causal)


def _kernel_ok(q, k, v):
    """The HIP kernel's supported envelope. Discovery probes this op with
    arbitrarily sharded shapes — anything outside goes to the math path.
    Any sequence length is inside (S % 128 != 0 runs the ragged kernels),
    and so is any K/V head count that divides q's (the GQA kernels)."""
    return (q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16
            and v.dtype == torch.bfloat16
            and q.dim() == 4 and k.dim() == 4 and k.shape == v.shape
            and k.shape[0] == q.shape[0] and k.shape[2:] == q.shape[2:]
            and q.numel() > 0 and k.numel() > 0
            and q.shape[1] % k.shape[1] == 0
            and q.shape[-1] in (64, 128))


def _fwd_cuda(q, k, v, causal):
    ext = load_extension()
    if ext is not None and _kernel_ok(q, k, v):
        # the kernel takes any last-dim-contiguous layout directly (the
        # [B,S,H,D] qkv-split views) — no activation-sized copies
        return ext.flash_attn_fwd(q, k, v, causal)
    from . import require_hip_ops
    if _kernel_ok(q, k, v):
        require_hip_ops()   # raises when the extension should exist
    return _math_fwd(q, k, v, causal)


def _bwd_cpu(grad, q, k, v, out, lse, causal):
    return _math_bwd(grad, q, k, v, out, lse, causal)


def _bwd_cuda(grad, q, k, v, out, lse, causal):
    ext = load_extension()
    if ext is not None and _kernel_ok(q, k, v):
        return ext.flash_attn_bwd(grad, q, k, v, out.contiguous(),
                                  lse.contiguous(), causal)
    return _math_bwd(grad, q, k, v, out, lse, causal)


def _pack3(dq, dk, dv):
    B, _, S, D = dq.shape
    return torch.cat([d.transpose(1, 2).reshape(B, S, d.shape[1] * D)
                      for d in (dq, dk, dv)], dim=-1)


def _bwd_pack_cpu(grad, q, k, v, out, lse, causal):
    return _pack3(*_math_bwd(grad, q, k, v, out, lse, causal))


def _bwd_pack_cuda(grad, q, k, v, out, lse, causal):
    ext = load_extension()
    if ext is not None and _kernel_ok(q, k, v):
        return ext.flash_attn_bwd_pack(grad, q, k, v, out.contiguous(),
                                       lse.contiguous(), causal)
    return _pack3(*_math_bwd(grad, q, k, v, out, lse, causal))


lib.impl("flash_attention", _fwd_cpu, "CPU")
lib.impl("flash_attention", _fwd_cuda, "CUDA")
lib.impl("flash_attention_bwd", _bwd_cpu, "CPU")
lib.impl("flash_attention_bwd", _bwd_cuda, "CUDA")
lib.impl("flash_attention_bwd_pack", _bwd_pack_cpu, "CPU")
lib.impl("flash_attention_bwd_pack", _bwd_pack_cuda, "CUDA")


@torch.library.register_fake("easydist_amd::flash_attention")
def _fa_fake(q, k, v, causal):
    lse = q.new_empty(q.shape[:-1], dtype=torch.float32)
    # the kernel returns a CONTIGUOUS [B,H,S,D] tensor regardless of input
    # strides — the fake must match or view/reshape traces diverge
    return q.new_empty(tuple(q.shape)), lse


@torch.library.register_fake("easydist_amd::flash_attention_bwd")
def _fab_fake(grad, q, k, v, out, lse, causal):
    # contiguous outputs (matmul results), independent of input strides
    return (q.new_empty(tuple(q.shape)), k.new_empty(tuple(k.shape)),
            v.new_empty(tuple(v.shape)))


@torch.library.register_fake("easydist_amd::flash_attention_bwd_pack")
def _fabp_fake(grad, q, k, v, out, lse, causal):
    B, H, S, D = q.shape
    return q.new_empty((B, S, (H + 2 * k.shape[1]) * D))


def _fa_backward(ctx, grad_out, grad_lse):
    q, k, v, out, lse = ctx.saved_tensors
    dq, dk, dv = torch.ops.easydist_amd.flash_attention_bwd(
        grad_out, q, k, v, out, lse, ctx.causal)
    return dq, dk, dv, None


def _fa_setup_ctx(ctx, inputs, output):
    q, k, v, causal = inputs
    out, lse = output
    ctx.save_for_backward(q, k, v, out, lse)
    ctx.causal = causal


torch.library.register_autograd("easydist_amd::flash_attention", _fa_backward,
                                setup_context=_fa_setup_ctx)


def scaled_dot_product_attention(q, k, v, causal: bool = True):
    out, _ = torch.ops.easydist_amd.flash_attention(q, k, v, causal)
    return out
