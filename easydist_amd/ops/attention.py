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

`flash_attention_swa` is sliding-window causal self-attention (Mistral's
`sliding_window = W`): query row i attends keys j with i - W < j <= i, W
keys with itself.  The window instantiations of the same three kernels walk
only the tiles the band touches, O(S * W) with no mask tensor; W >= S is
plain causal attention and runs the causal kernels.  The packed backward and
the sequence-parallel (ring) rewrite do not know windows yet.

`flash_attention_doc` is document-masked causal self-attention for packed
sequences: a row of S tokens holds several documents and token i attends
only the earlier tokens of its own, keys lo[b, i] <= j <= i.  The bounds are
two int32 [B, S] tensors from `document_bounds(doc_ids)`, computed once per
step and shared by all layers and heads; there is no [S, S] mask.  The
document instantiations of the same three kernels walk only the tiles a
block's documents touch: the sum of L_k^2 / 2 pairs over the document
lengths L_k in place of S^2 / 2.  The launches never read the bounds on the
host.  The packed backward and ring attention do not know documents, and a
window inside documents is not offered.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

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
# sliding-window causal attention: ops of their own, so that whatever
# matches the schemas above (lowering passes, presets, the ring-attention
# rewrite) keeps matching exactly what it did
lib.define("flash_attention_swa(Tensor q, Tensor k, Tensor v, int window) "
           "-> (Tensor, Tensor)")
lib.define("flash_attention_swa_bwd(Tensor grad, Tensor q, Tensor k, "
           "Tensor v, Tensor out, Tensor lse, int window) "
           "-> (Tensor, Tensor, Tensor)")
# document-masked causal attention (packed sequences): ops of their own for
# the same reason; lo and hi are the int32 [B, S] bounds of document_bounds
lib.define("flash_attention_doc(Tensor q, Tensor k, Tensor v, Tensor lo, "
           "Tensor hi) -> (Tensor, Tensor)")
lib.define("flash_attention_doc_bwd(Tensor grad, Tensor q, Tensor k, "
           "Tensor v, Tensor out, Tensor lse, Tensor lo, Tensor hi) "
           "-> (Tensor, Tensor, Tensor)")


def document_bounds(doc_ids):
    """(lo, hi) int32 [B, S] of integer ids [B, S] that are constant on each
    document and change at each boundary: lo[b, i] is the first token of the
    document of token i, hi[b, i] one past its last.  Compute it once per
    step; every layer and head shares it."""
    if doc_ids.dim() != 2:
        raise ValueError("document_bounds: doc_ids must be [B, S], got "
                         f"{tuple(doc_ids.shape)}")
    B, S = doc_ids.shape
    pos = torch.arange(S, device=doc_ids.device)
    edge = doc_ids[:, 1:] != doc_ids[:, :-1]        # token i + 1 starts one
    first = torch.ones(B, 1, dtype=torch.bool, device=doc_ids.device)
    # the latest start at or before i; the earliest end after i
    start = torch.where(torch.cat([first, edge], 1), pos, 0)
    lo = torch.cummax(start, dim=1).values
    end = torch.where(torch.cat([edge, first], 1), pos + 1, S)
    hi = torch.cummin(end.flip(1), dim=1).values.flip(1)
    return lo.to(torch.int32), hi.to(torch.int32)


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


def _mask(S, T, window, device):
    """Causal mask [S, T], True = visible; with a window the band
    i - window < j <= i."""
    mask = torch.ones(S, T, dtype=torch.bool, device=device).tril()
    if window is not None:
        mask = mask & ~torch.ones(S, T, dtype=torch.bool,
                                  device=device).tril(-window)
    return mask


def _check_window(q, k, window):
    if window < 1:
        raise ValueError(f"flash_attention_swa: window must be >= 1, got "
                         f"{window}")
    if q.shape[-2] != k.shape[-2]:
        raise ValueError("flash_attention_swa: self-attention only, got "
                         f"Sq {q.shape[-2]} and Sk {k.shape[-2]}")


def _doc_mask(lo, S):
    """[B, 1, S, S], True = visible: lo[b, i] <= j <= i."""
    j = torch.arange(S, device=lo.device)
    return ((j[None, None, :] >= lo[:, :, None])
            & (j[None, None, :] <= j[None, :, None])).unsqueeze(1)


def _check_doc(q, k, lo, hi):
    if q.dim() != 4 or q.shape[-2] != k.shape[-2]:
        raise ValueError("flash_attention_doc: 4-D self-attention only, got "
                         f"q {tuple(q.shape)} and k {tuple(k.shape)}")
    want = (q.shape[0], q.shape[2])
    for t in (lo, hi):
        if t.dtype != torch.int32 or tuple(t.shape) != want:
            raise ValueError(
                f"flash_attention_doc: lo and hi must be int32 {want}, got "
                f"{t.dtype} {tuple(t.shape)}")


def _math_fwd(q, k, v, causal, window=None, doc=None):
    # q: [B, H, S, D]; k,v: [B, Hkv, T, D]; a window implies causal; doc =
    # (lo, hi) implies causal and replaces the mask by lo[b, i] <= j <= i
    G = _group(q, k, v)
    k, v = _expand_kv(k, G), _expand_kv(v, G)
    scale = 1.0 / math.sqrt(q.shape[-1])
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    if doc is not None:
        s = s.masked_fill(~_doc_mask(doc[0], s.shape[-1]), float("-inf"))
    elif causal:
        mask = _mask(s.shape[-2], s.shape[-1], window, s.device)
        s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    out = torch.matmul(p.to(v.dtype), v)
    return out, lse


def _math_bwd(grad, q, k, v, out, lse, causal, window=None, doc=None):
    G = _group(q, k, v)
    kdt, vdt = k.dtype, v.dtype
    k, v = _expand_kv(k, G), _expand_kv(v, G)
    scale = 1.0 / math.sqrt(q.shape[-1])
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    if doc is not None:
        s = s.masked_fill(~_doc_mask(doc[0], s.shape[-1]), float("-inf"))
    elif causal:
        mask = _mask(s.shape[-2], s.shape[-1], window, s.device)
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


def _swa_fwd_cpu(q, k, v, window):
    _check_window(q, k, window)
    return _math_fwd(q, k, v, True, window)


def _swa_fwd_cuda(q, k, v, window):
    _check_window(q, k, window)
    ext = load_extension()
    if ext is not None and _kernel_ok(q, k, v):
        return ext.flash_attn_fwd(q, k, v, True, window)
    from . import require_hip_ops
    if _kernel_ok(q, k, v):
        require_hip_ops()   # raises when the extension should exist
    return _math_fwd(q, k, v, True, window)


def _swa_bwd_cpu(grad, q, k, v, out, lse, window):
    _check_window(q, k, window)
    return _math_bwd(grad, q, k, v, out, lse, True, window)


def _swa_bwd_cuda(grad, q, k, v, out, lse, window):
    _check_window(q, k, window)
    ext = load_extension()
    if ext is not None and _kernel_ok(q, k, v):
        return ext.flash_attn_bwd(grad, q, k, v, out.contiguous(),
                                  lse.contiguous(), True, window)
    return _math_bwd(grad, q, k, v, out, lse, True, window)


def _doc_fwd_cpu(q, k, v, lo, hi):
    _check_doc(q, k, lo, hi)
    return _math_fwd(q, k, v, True, None, (lo, hi))


def _doc_fwd_cuda(q, k, v, lo, hi):
    _check_doc(q, k, lo, hi)
    ext = load_extension()
    if ext is not None and _kernel_ok(q, k, v):
        return ext.flash_attn_fwd(q, k, v, True, None, lo.contiguous(),
                                  hi.contiguous())
    from . import require_hip_ops
    if _kernel_ok(q, k, v):
        require_hip_ops()   # raises when the extension should exist
    return _math_fwd(q, k, v, True, None, (lo, hi))


def _doc_bwd_cpu(grad, q, k, v, out, lse, lo, hi):
    _check_doc(q, k, lo, hi)
    return _math_bwd(grad, q, k, v, out, lse, True, None, (lo, hi))


def _doc_bwd_cuda(grad, q, k, v, out, lse, lo, hi):
    _check_doc(q, k, lo, hi)
    ext = load_extension()
    if ext is not None and _kernel_ok(q, k, v):
        return ext.flash_attn_bwd(grad, q, k, v, out.contiguous(),
                                  lse.contiguous(), True, None,
                                  lo.contiguous(), hi.contiguous())
    return _math_bwd(grad, q, k, v, out, lse, True, None, (lo, hi))


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
lib.impl("flash_attention_swa", _swa_fwd_cpu, "CPU")
lib.impl("flash_attention_swa", _swa_fwd_cuda, "CUDA")
lib.impl("flash_attention_swa_bwd", _swa_bwd_cpu, "CPU")
lib.impl("flash_attention_swa_bwd", _swa_bwd_cuda, "CUDA")
lib.impl("flash_attention_doc", _doc_fwd_cpu, "CPU")
lib.impl("flash_attention_doc", _doc_fwd_cuda, "CUDA")
lib.impl("flash_attention_doc_bwd", _doc_bwd_cpu, "CPU")
lib.impl("flash_attention_doc_bwd", _doc_bwd_cuda, "CUDA")


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


@torch.library.register_fake("easydist_amd::flash_attention_swa")
def _swa_fake(q, k, v, window):
    return _fa_fake(q, k, v, True)


@torch.library.register_fake("easydist_amd::flash_attention_swa_bwd")
def _swab_fake(grad, q, k, v, out, lse, window):
    return _fab_fake(grad, q, k, v, out, lse, True)


@torch.library.register_fake("easydist_amd::flash_attention_doc")
def _doc_fake(q, k, v, lo, hi):
    return _fa_fake(q, k, v, True)


@torch.library.register_fake("easydist_amd::flash_attention_doc_bwd")
def _docb_fake(grad, q, k, v, out, lse, lo, hi):
    return _fab_fake(grad, q, k, v, out, lse, True)


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


def _swa_backward(ctx, grad_out, grad_lse):
    q, k, v, out, lse = ctx.saved_tensors
    dq, dk, dv = torch.ops.easydist_amd.flash_attention_swa_bwd(
        grad_out, q, k, v, out, lse, ctx.window)
    return dq, dk, dv, None


def _swa_setup_ctx(ctx, inputs, output):
    q, k, v, window = inputs
    out, lse = output
    ctx.save_for_backward(q, k, v, out, lse)
    ctx.window = window


torch.library.register_autograd("easydist_amd::flash_attention_swa",
                                _swa_backward, setup_context=_swa_setup_ctx)


def _doc_backward(ctx, grad_out, grad_lse):
    q, k, v, out, lse, lo, hi = ctx.saved_tensors
    dq, dk, dv = torch.ops.easydist_amd.flash_attention_doc_bwd(
        grad_out, q, k, v, out, lse, lo, hi)
    return dq, dk, dv, None, None      # the integer bounds take no gradient


def _doc_setup_ctx(ctx, inputs, output):
    q, k, v, lo, hi = inputs
    out, lse = output
    ctx.save_for_backward(q, k, v, out, lse, lo, hi)


torch.library.register_autograd("easydist_amd::flash_attention_doc",
                                _doc_backward, setup_context=_doc_setup_ctx)


def scaled_dot_product_attention(q, k, v, causal: bool = True,
                                 window: Optional[int] = None,
                                 doc_bounds: Optional[Tuple] = None):
    """window = W: sliding-window causal attention, row i attends keys
    i - W + 1 .. i (flash_attention_swa); it needs causal=True.
    doc_bounds = (lo, hi) from document_bounds: packed sequences, row i
    attends keys lo[b, i] .. i (flash_attention_doc); it needs causal=True
    and no window."""
    if doc_bounds is not None:
        if not causal:
            raise ValueError("scaled_dot_product_attention: doc_bounds needs "
                             "causal=True")
        if window is not None:
            raise ValueError("scaled_dot_product_attention: doc_bounds and a "
                             "window do not combine")
        lo, hi = doc_bounds
        out, _ = torch.ops.easydist_amd.flash_attention_doc(q, k, v, lo, hi)
        return out
    if window is not None:
        if not causal:
            raise ValueError("scaled_dot_product_attention: a window needs "
                             "causal=True")
        if window < 1:
            raise ValueError("scaled_dot_product_attention: window must be "
                             f">= 1, got {window}")
        out, _ = torch.ops.easydist_amd.flash_attention_swa(q, k, v, window)
        return out
    out, _ = torch.ops.easydist_amd.flash_attention(q, k, v, causal)
    return out
