"""Mixtral-shape MoE with expert parallelism over xGMI all-to-all.

BASELINE.json names "Mixtral-8x7B-shape MoE auto-SPMD (expert all-to-all
over xGMI) on 8x MI355X" as a headline config; the reference has NO
expert parallelism (SURVEY.md §2 checklist: all_to_all existed only as an
all-gather+slice reshard fallback, easydist/torch/passes/sharding.py:
155-163). This module implements it MI355X-first:

* capacity-based top-k routing with FIXED per-expert capacity so every
  tensor shape is static — traceable, hipGraph-capturable, and the
  all-to-all payloads are equal-sized (RCCL `all_to_all_single` maps to
  pairwise xGMI exchanges with no host-side size negotiation);
* with an expert-parallel process group each rank owns
  n_experts/ep_world experts: tokens are dispatched
  all_to_all(SHARD(rank)->SHARD(expert)), expert FFNs run batched on the
  local experts, and a second all-to-all returns the results;
* without a group the same math runs locally (1-GPU path, CPU tests).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F


@dataclass
class MoEConfig:
    vocab_size: int = 32000
    n_layer: int = 8
    n_head: int = 32
    n_embd: int = 4096
    block_size: int = 2048
    n_experts: int = 8
    top_k: int = 2
    ffn_hidden: int = 14336
    capacity_factor: float = 1.25
    bias: bool = False
    # K/V heads (grouped-query attention); None = n_head, plain MHA
    n_kv_head: Optional[int] = None
    # rotary position embeddings on q and k instead of the learned wpe
    rope: bool = False
    rope_base: float = 10000.0


# Mixtral-8x7B shape (per-layer geometry; n_layer reduced variants below)
MIXTRAL_8X7B = MoEConfig(n_layer=32)
# the same with the real model's 8 K/V heads (G = 4)
MIXTRAL_8X7B_GQA = MoEConfig(n_layer=32, n_kv_head=8)
# ... and its rotary position embeddings (base 1e6)
MIXTRAL_8X7B_ROPE = MoEConfig(n_layer=32, n_kv_head=8, rope=True,
                              rope_base=1e6)
MIXTRAL_SMALL = MoEConfig(vocab_size=1024, n_layer=2, n_head=4, n_embd=256,
                          block_size=128, n_experts=4, top_k=2,
                          ffn_hidden=512)
MIXTRAL_BENCH_4L = MoEConfig(n_layer=4)


def _capacity(tokens: int, n_experts: int, top_k: int,
              factor: float) -> int:
    from ..ops.moe_ops import capacity
    return capacity(tokens, n_experts, top_k, factor)


class ExpertFFN(nn.Module):
    """SwiGLU expert bank stored as 3 batched weights [E, ...] so the
    per-expert GEMMs run as ONE bmm per projection (MFMA-batched on
    hipBLASLt) instead of E small launches."""

    def __init__(self, n_local: int, d: int, h: int):
        super().__init__()
        self.w1 = nn.Parameter(torch.empty(n_local, d, h))
        self.w3 = nn.Parameter(torch.empty(n_local, d, h))
        self.w2 = nn.Parameter(torch.empty(n_local, h, d))
        for w in (self.w1, self.w3):
            nn.init.normal_(w, std=0.02)
        nn.init.normal_(self.w2, std=0.02 / math.sqrt(2.0))

    def forward(self, x):           # x: [E_local, capacity*, d]
        a = torch.bmm(x, self.w1)
        b = torch.bmm(x, self.w3)
        return torch.bmm(F.silu(a) * b, self.w2)


class MoELayer(nn.Module):
    """Top-k routed MoE with optional expert-parallel all-to-all."""

    def __init__(self, cfg: MoEConfig, ep_group=None):
        super().__init__()
        self.cfg = cfg
        self.ep_group = ep_group
        self.ep_world = 1
        self.ep_rank = 0
        if ep_group is not None:
            import torch.distributed as dist
            self.ep_world = dist.get_world_size(ep_group)
            self.ep_rank = dist.get_rank(ep_group)
        assert cfg.n_experts % self.ep_world == 0
        self.n_local = cfg.n_experts // self.ep_world
        self.router = nn.Linear(cfg.n_embd, cfg.n_experts, bias=False)
        self.experts = ExpertFFN(self.n_local, cfg.n_embd, cfg.ffn_hidden)

    def forward(self, x):
        B, T, C = x.shape
        tokens = x.reshape(-1, C)                      # [N, C] local tokens
        N = tokens.shape[0]
        E, K = self.cfg.n_experts, self.cfg.top_k
        logits = self.router(tokens)                   # [N, E]
        probs = F.softmax(logits.float(), dim=-1)
        topv, topi = probs.topk(K, dim=-1)             # [N, K]
        topv = (topv / topv.sum(-1, keepdim=True)).to(x.dtype)

        # STATIC-SHAPE capacity routing through the compiler-visible
        # custom ops (ops/moe_ops.py): the auto-SPMD solver sees their
        # declared sharding algebra and can choose EP — bins resharded
        # S(cap)->S(expert) with ONE rt_all_to_all over xGMI — against
        # DP-experts, priced by its own cost model. capacity is computed
        # inside the op from the LOCAL token count.
        from ..ops import moe_ops  # noqa: F401  (registers the ops)
        bins, gates, src_index, valid = torch.ops.easydist_amd.moe_bins(
            tokens, topi, topv, E, self.cfg.capacity_factor)
        cap = bins.shape[1]

        if self.ep_group is not None and self.ep_world > 1:
            from ..parallel import comm
            W, L = self.ep_world, self.n_local
            # module-level EP (eager reference path; the compiled path
            # reaches the same exchange through the solver)
            recv = comm.all_to_all_ep(bins, self.ep_group)
            expert_in = recv.reshape(W, L, cap, C).transpose(0, 1) \
                .reshape(L, W * cap, C)
            expert_out = self.experts(expert_in)
            send_back = expert_out.reshape(L, W, cap, C).transpose(0, 1) \
                .reshape(W * L, cap, C).contiguous()
            out_bins = comm.all_to_all_ep(send_back, self.ep_group)
            out_bins = out_bins.reshape(E, cap, C)
        else:
            out_bins = self.experts(bins).reshape(E, cap, C)

        # combine: weighted scatter-add back to token positions
        out = torch.ops.easydist_amd.moe_combine(
            out_bins, gates, src_index, valid, tokens, K)
        return out.to(x.dtype).reshape(B, T, C)


class MoEBlock(nn.Module):
    def __init__(self, cfg: MoEConfig, ep_group=None):
        super().__init__()
        self.ln_1 = nn.LayerNorm(cfg.n_embd, bias=cfg.bias)
        from .gpt import CausalSelfAttention, GPTConfig
        acfg = GPTConfig(n_embd=cfg.n_embd, n_head=cfg.n_head,
                         n_kv_head=cfg.n_kv_head,
                         rope=cfg.rope, rope_base=cfg.rope_base,
                         bias=cfg.bias, block_size=cfg.block_size)
        self.attn = CausalSelfAttention(acfg)
        self.ln_2 = nn.LayerNorm(cfg.n_embd, bias=cfg.bias)
        self.moe = MoELayer(cfg, ep_group)

    def forward(self, x, rope=None):
        x = x + self.attn(self.ln_1(x), rope)
        x = x + self.moe(self.ln_2(x))
        return x


class MoEGPT(nn.Module):
    """Mixtral-shape decoder-only LM with MoE FFNs."""

    def __init__(self, cfg: MoEConfig, ep_group=None):
        super().__init__()
        self.cfg = cfg
        self.wte = nn.Embedding(cfg.vocab_size, cfg.n_embd)
        if not cfg.rope:
            self.wpe = nn.Embedding(cfg.block_size, cfg.n_embd)
        self.h = nn.ModuleList(MoEBlock(cfg, ep_group)
                               for _ in range(cfg.n_layer))
        self.ln_f = nn.LayerNorm(cfg.n_embd, bias=cfg.bias)
        self.lm_head = nn.Linear(cfg.n_embd, cfg.vocab_size, bias=False)
        self.register_buffer("pos", torch.arange(cfg.block_size),
                             persistent=False)
        if cfg.rope:
            from .gpt import register_rope_tables
            register_rope_tables(self, cfg.block_size,
                                 cfg.n_embd // cfg.n_head, cfg.rope_base)
        nn.init.normal_(self.wte.weight, std=0.02)
        if not cfg.rope:
            nn.init.normal_(self.wpe.weight, std=0.02)
        nn.init.normal_(self.lm_head.weight, std=0.02)

    def forward(self, idx):
        B, T = idx.shape
        rope = None
        if self.cfg.rope:
            x = self.wte(idx)
            rope = (self.rope_cos[:T], self.rope_sin[:T])
        else:
            x = self.wte(idx) + self.wpe(self.pos[:T])
        if torch.is_autocast_enabled(x.device.type):
            x = x.to(torch.bfloat16)   # keep the residual stream bf16
        for blk in self.h:
            x = blk(x, rope)
        return self.lm_head(self.ln_f(x))

    def loss(self, idx, targets):
        logits = self(idx)
        return F.cross_entropy(logits.float().view(-1, logits.size(-1)),
                               targets.reshape(-1))


def moe_train_step(model, opt, idx, targets):
    dev = "cuda" if idx.is_cuda else "cpu"
    with torch.autocast(device_type=dev, dtype=torch.bfloat16,
                        enabled=idx.is_cuda):
        logits = model(idx)
    loss = F.cross_entropy(logits.float().view(-1, logits.size(-1)),
                           targets.reshape(-1))
    loss.backward()
    opt.step()
    opt.zero_grad(True)
    return loss
