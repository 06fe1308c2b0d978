"""MoE routing as compiler-visible custom ops: EP through the solver.

VERDICT item 3 (the designated beyond-reference capability): the round-1
MoE did its expert all-to-all at MODULE level, invisible to the
auto-SPMD pipeline.  These ops make the capacity-routing scatter and the
weighted combine OPAQUE graph nodes with declared sharding algebra, so
the solver itself chooses between

* DP-experts: bins stay token-sharded (S on the capacity dim), expert
  weights replicate, their gradients all-reduce — zero activation comm,
  heavy weight comm; and
* EP: bins reshard S(cap)->S(expert) — the standard expert-parallel
  all-to-all, emitted by the ordinary S(i)->S(j) reshard machinery
  (passes/sharding.py:_emit_comm -> rt_all_to_all) — expert weights and
  their gradients stay sharded.

The EP preset declares the *parallel* routing semantics (each rank
routes its own tokens into its own capacity slice).  That is the
standard MoE formulation, not an elementwise sharding of the global
trace: slot ORDER inside an expert's capacity, and which tokens drop on
overflow, legitimately differ between world sizes (capacity dropping is
sharding-dependent in every MoE system).  tests/test_moe.py validates
the ws2 execution against the module-level EP reference instead of the
ws1 trace.

Shape plumbing: capacity is computed INSIDE moe_bins from the local
token count (a baked trace-time constant would carry the GLOBAL size
into the shards), and the combine/backward take a `tokens`-shaped
reference tensor instead of an integer row count for the same reason.
Sharding therefore requires cap(N) to divide evenly: cap(N/W)*W ==
cap(N) — true for the benchmark shapes; asserted in the model.

src encoding: src = token_index * K + k  (one field carries both the
token row and which of its top-k slots the bin holds).

On the GPU the four ops run as hand-written gfx950 kernels
(csrc/moe_kernels.hip) inside this envelope: tokens, bins, gbins, gout,
topv, gates and ggates bf16 and contiguous, the row tensors with
C % 8 == 0, C <= 512 (one 16-byte vector per lane of the wave that owns a
row) and 16-byte aligned data; topi and src int64 and contiguous,
valid bool; 1 <= E <= 256, 1 <= K <= 8, N >= 1, N*K and E*cap below 2^31.
Everything else, the CPU, and EASYDIST_MOE_HIP=0 (read at each call, for
A/B timing) run the aten functions below.  The kernels' contract:

* bins, gates, src and valid of moe_bins, gbins of moe_combine_bwd and
  gtopv of moe_bins_bwd are equal (torch.equal) to the aten functions: a
  stable counting sort by expert gives the slot order of aten's stable
  argsort.  The one difference in bits: the gbins row of an invalid slot
  is +0 where aten's gout[0] * 0 * 0 is -0 for a negative gout[0];
* out of moe_combine, gtokens of moe_bins_bwd and ggates of
  moe_combine_bwd are the exact formula summed in fp32 in a fixed order
  (k = 0..K-1; the row dot in a lane's registers, then across the lanes of
  the row's wave) and rounded to bf16 once: tighter than the aten path,
  which rounds every partial sum to bf16, and the same bits on every run,
  where aten's index_add_ adds atomically in whatever order the hardware
  takes.

No atomics, no zero-fill passes, no host synchronisation: the launches go
to the current stream with scratch from the torch allocator and record
into a captured graph.

What does not reach the kernels today.  Rows wider than 512 elements, the
Mixtral bench shape (C = 4096) among them.  And MoEGPT under
moe_train_step's bf16 autocast, eager or compiled: autocast runs the
LayerNorm before the router in fp32, so `tokens`, and `topv` cast to its
dtype, arrive as fp32, `gates` stays fp32 and `gbins` comes back fp32;
all four ops then run the aten functions.  A model held in bf16
(MoELayer(cfg).bfloat16()) with n_embd <= 512 runs the kernels.
"""
from __future__ import annotations

import math
import os

import torch

from . import load_extension

lib = torch.library.Library("easydist_amd", "FRAGMENT")
lib.define("moe_bins(Tensor tokens, Tensor topi, Tensor topv, int n_experts,"
           " float capacity_factor) -> (Tensor, Tensor, Tensor, Tensor)")
lib.define("moe_bins_bwd(Tensor gbins, Tensor ggates, Tensor src, "
           "Tensor valid, Tensor tokens_ref, int top_k) -> (Tensor, Tensor)")
lib.define("moe_combine(Tensor bins, Tensor gates, Tensor src, Tensor valid,"
           " Tensor tokens_ref, int top_k) -> Tensor")
lib.define("moe_combine_bwd(Tensor gout, Tensor bins, Tensor gates, "
           "Tensor src, Tensor valid, int top_k) -> (Tensor, Tensor)")


def capacity(tokens: int, n_experts: int, top_k: int, factor: float) -> int:
    c = int(math.ceil(tokens * top_k / n_experts * factor))
    return max(4, (c + 3) // 4 * 4)   # multiple of 4 for tidy kernels


def _bins_impl(tokens, topi, topv, n_experts, capacity_factor):
    N, C = tokens.shape
    K = topi.shape[1]
    E = n_experts
    cap = capacity(N, E, K, capacity_factor)
    dev = tokens.device
    flat_expert = topi.reshape(-1)
    order = torch.argsort(flat_expert, stable=True)
    sorted_e = flat_expert[order]
    seg_start = torch.searchsorted(sorted_e, torch.arange(E, device=dev))
    pos_in_seg = torch.arange(N * K, device=dev) - seg_start[sorted_e]
    keep = pos_in_seg < cap
    slot = torch.where(keep, pos_in_seg,
                       torch.full_like(pos_in_seg, cap))
    tok_idx = order // K
    k_idx = order % K
    bins_x = tokens.new_zeros(E, cap + 1, C)
    gates_x = topv.new_zeros(E, cap + 1)
    src_x = torch.zeros(E, cap + 1, dtype=torch.long, device=dev)
    valid_x = torch.zeros(E, cap + 1, dtype=torch.bool, device=dev)
    bins_x[sorted_e, slot] = tokens[tok_idx]
    gates_x[sorted_e, slot] = torch.where(
        keep, topv[tok_idx, k_idx],
        torch.zeros_like(pos_in_seg, dtype=topv.dtype))
    src_x[sorted_e, slot] = tok_idx * K + k_idx
    valid_x[sorted_e, slot] = keep
    return (bins_x[:, :cap].contiguous(), gates_x[:, :cap].contiguous(),
            src_x[:, :cap].contiguous(), valid_x[:, :cap].contiguous())


def _bins_bwd_impl(gbins, ggates, src, valid, tokens_ref, top_k):
    E, cap, C = gbins.shape
    n_tokens = tokens_ref.shape[0]
    vm = valid.to(gbins.dtype).unsqueeze(-1)
    gtokens = gbins.new_zeros(n_tokens, C)
    gtokens.index_add_(0, (src // top_k).reshape(-1),
                       (gbins * vm).reshape(-1, C))
    gtopv = ggates.new_zeros(n_tokens * top_k)
    gtopv.index_add_(0, src.reshape(-1),
                     (ggates * valid.to(ggates.dtype)).reshape(-1))
    return gtokens, gtopv.reshape(n_tokens, top_k)


def _combine_impl(bins, gates, src, valid, tokens_ref, top_k):
    E, cap, C = bins.shape
    n_tokens = tokens_ref.shape[0]
    out = bins.new_zeros(n_tokens, C)
    contrib = bins * gates.unsqueeze(-1) \
        * valid.unsqueeze(-1).to(bins.dtype)
    out.index_add_(0, (src // top_k).reshape(-1),
                   contrib.reshape(-1, C).to(out.dtype))
    return out


def _combine_bwd_impl(gout, bins, gates, src, valid, top_k):
    g_rows = gout[(src // top_k).reshape(-1)].reshape(bins.shape)
    vm = valid.to(bins.dtype).unsqueeze(-1)
    gbins = (g_rows * gates.unsqueeze(-1) * vm).to(bins.dtype)
    ggates = (g_rows.float() * bins.float() * vm.float()).sum(-1) \
        .to(gates.dtype)
    return gbins, ggates


MAX_EXPERTS = 256
MAX_TOP_K = 8
MAX_ROW = 512      # elements of a row: 64 lanes of 8


def _rows_ok(t, ndim):
    """A bf16 row tensor the kernels read or write with 16-byte vectors."""
    return (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == ndim
            and t.is_contiguous() and t.size(-1) % 8 == 0
            and t.size(-1) <= MAX_ROW and t.data_ptr() % 16 == 0)


def _flat_ok(t, dtype, shape):
    return (t.is_cuda and t.dtype == dtype and t.is_contiguous()
            and tuple(t.shape) == tuple(shape))


def _sizes_ok(N, K, E, cap):
    return (1 <= E <= MAX_EXPERTS and 1 <= K <= MAX_TOP_K and N >= 1
            and cap >= 1 and N * K < 2 ** 31 and E * cap < 2 ** 31)


def _slots_ok(rows, gates, src, valid, n_tokens, top_k):
    """[E, cap, C] rows with their [E, cap] gates and routing metadata."""
    if not _rows_ok(rows, 3):
        return False
    ec = rows.shape[:2]
    return (_flat_ok(gates, torch.bfloat16, ec)
            and _flat_ok(src, torch.long, ec)
            and _flat_ok(valid, torch.bool, ec)
            and _sizes_ok(n_tokens, top_k, ec[0], ec[1]))


def _bins_kernel_ok(tokens, topi, topv, n_experts, capacity_factor):
    if not _rows_ok(tokens, 2) or topi.dim() != 2:
        return False
    N, K = tokens.shape[0], topi.shape[1]
    return (_flat_ok(topi, torch.long, (N, K))
            and _flat_ok(topv, torch.bfloat16, (N, K))
            and _sizes_ok(N, K, n_experts,
                          capacity(N, n_experts, K, capacity_factor)))


def _bins_bwd_kernel_ok(gbins, ggates, src, valid, tokens_ref, top_k):
    return _slots_ok(gbins, ggates, src, valid, tokens_ref.shape[0], top_k)


def _combine_kernel_ok(bins, gates, src, valid, tokens_ref, top_k):
    return _slots_ok(bins, gates, src, valid, tokens_ref.shape[0], top_k)


def _combine_bwd_kernel_ok(gout, bins, gates, src, valid, top_k):
    return (_rows_ok(gout, 2) and bins.dim() == 3
            and gout.shape[1] == bins.shape[2]
            and _slots_ok(bins, gates, src, valid, gout.shape[0], top_k))


def _kernels(ok):
    """The extension when the call is inside the envelope `ok` and the
    kernels are not switched off; None sends the call to the aten path.
    Inside the envelope on a GPU host a missing extension is an error."""
    if not ok or os.environ.get("EASYDIST_MOE_HIP", "1") == "0":
        return None
    ext = load_extension()
    if ext is None:
        from . import require_hip_ops
        require_hip_ops()   # raises when the extension should exist
    return ext


def _bins_cuda(tokens, topi, topv, n_experts, capacity_factor):
    ext = _kernels(_bins_kernel_ok(tokens, topi, topv, n_experts,
                                   capacity_factor))
    if ext is None:
        return _bins_impl(tokens, topi, topv, n_experts, capacity_factor)
    cap = capacity(tokens.shape[0], n_experts, topi.shape[1],
                   capacity_factor)
    return ext.moe_bins_fwd(tokens, topi, topv, n_experts, cap)


def _bins_bwd_cuda(gbins, ggates, src, valid, tokens_ref, top_k):
    ext = _kernels(_bins_bwd_kernel_ok(gbins, ggates, src, valid,
                                       tokens_ref, top_k))
    if ext is None:
        return _bins_bwd_impl(gbins, ggates, src, valid, tokens_ref, top_k)
    return ext.moe_bins_bwd(gbins, ggates, src, valid, tokens_ref.shape[0],
                            top_k)


def _combine_cuda(bins, gates, src, valid, tokens_ref, top_k):
    ext = _kernels(_combine_kernel_ok(bins, gates, src, valid, tokens_ref,
                                      top_k))
    if ext is None:
        return _combine_impl(bins, gates, src, valid, tokens_ref, top_k)
    return ext.moe_combine_fwd(bins, gates, src, valid, tokens_ref.shape[0],
                               top_k)


def _combine_bwd_cuda(gout, bins, gates, src, valid, top_k):
    ext = _kernels(_combine_bwd_kernel_ok(gout, bins, gates, src, valid,
                                          top_k))
    if ext is None:
        return _combine_bwd_impl(gout, bins, gates, src, valid, top_k)
    return ext.moe_combine_bwd(gout, bins, gates, src, valid, top_k)


for _name, _cpu, _cuda in (
        ("moe_bins", _bins_impl, _bins_cuda),
        ("moe_bins_bwd", _bins_bwd_impl, _bins_bwd_cuda),
        ("moe_combine", _combine_impl, _combine_cuda),
        ("moe_combine_bwd", _combine_bwd_impl, _combine_bwd_cuda)):
    lib.impl(_name, _cpu, "CPU")
    lib.impl(_name, _cuda, "CUDA")


@torch.library.register_fake("easydist_amd::moe_bins")
def _bins_fake(tokens, topi, topv, n_experts, capacity_factor):
    N, C = tokens.shape
    K = topi.shape[1]
    cap = capacity(int(N), n_experts, int(K), capacity_factor)
    E = n_experts
    return (tokens.new_empty(E, cap, C), topv.new_empty(E, cap),
            tokens.new_empty((E, cap), dtype=torch.long),
            tokens.new_empty((E, cap), dtype=torch.bool))


@torch.library.register_fake("easydist_amd::moe_bins_bwd")
def _bins_bwd_fake(gbins, ggates, src, valid, tokens_ref, top_k):
    return (gbins.new_empty(tokens_ref.shape[0], gbins.shape[2]),
            ggates.new_empty(tokens_ref.shape[0], top_k))


@torch.library.register_fake("easydist_amd::moe_combine")
def _combine_fake(bins, gates, src, valid, tokens_ref, top_k):
    return bins.new_empty(tokens_ref.shape[0], bins.shape[2])


@torch.library.register_fake("easydist_amd::moe_combine_bwd")
def _combine_bwd_fake(gout, bins, gates, src, valid, top_k):
    return torch.empty_like(bins), torch.empty_like(gates)


def _bins_backward(ctx, gbins, ggates, gsrc, gvalid):
    src, valid, tokens = ctx.saved_tensors
    gtokens, gtopv = torch.ops.easydist_amd.moe_bins_bwd(
        gbins, ggates, src, valid, tokens, ctx.top_k)
    return gtokens, None, gtopv, None, None


def _bins_setup(ctx, inputs, output):
    tokens, topi, topv, n_experts, capacity_factor = inputs
    bins, gates, src, valid = output
    ctx.save_for_backward(src, valid, tokens)
    ctx.top_k = topi.shape[1]


torch.library.register_autograd("easydist_amd::moe_bins", _bins_backward,
                                setup_context=_bins_setup)


def _combine_backward(ctx, gout):
    bins, gates, src, valid = ctx.saved_tensors
    gbins, ggates = torch.ops.easydist_amd.moe_combine_bwd(
        gout, bins, gates, src, valid, ctx.top_k)
    return gbins, ggates, None, None, None, None


def _combine_setup(ctx, inputs, output):
    bins, gates, src, valid, tokens_ref, top_k = inputs
    ctx.save_for_backward(bins, gates, src, valid)
    ctx.top_k = top_k


torch.library.register_autograd("easydist_amd::moe_combine",
                                _combine_backward,
                                setup_context=_combine_setup)
