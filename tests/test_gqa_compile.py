"""Grouped-query attention through the compiler, the sharding presets and
ring attention (CPU).

* an `enable_gqa=True` SDPA, traced forward and backward, is rewritten by
  lower_sdpa to the flash attention ops and still computes the eager result;
* a GPT with n_kv_head < n_head compiles, matches eager and has its
  dq/dk/dv repack chain fused into one packed backward per layer;
* the head-dim sharding rule of flash_attention and flash_attention_bwd is
  machine-checked at (H, Hkv) = (4, 2) as tests/test_presets.py does, and
  at Hkv = 1 no rule shards dim 1 of k/v;
* ring attention with (H, Hkv) = (4, 2) equals the single-process op.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

import easydist_amd.ops  # noqa: F401  (registers custom ops + presets)
from easydist_amd.utils.testing import init_single_process, spawn

aten = torch.ops.aten
ed = torch.ops.easydist_amd


# ---------------------------------------------------------------- lowering --
@pytest.mark.parametrize("H,Hkv", [(4, 2), (4, 1)])
def test_lower_sdpa_enable_gqa(H, Hkv):
    from torch.fx.experimental.proxy_tensor import make_fx

    from easydist_amd.compiler.passes.lower_hip import lower_sdpa

    def fwd_bwd(q, k, v, go):
        out = F.scaled_dot_product_attention(q, k, v, is_causal=True,
                                             enable_gqa=True)
        dq, dk, dv = torch.autograd.grad(out, (q, k, v), go)
        return out, dq, dk, dv

    torch.manual_seed(0)
    B, S, D = 2, 16, 8
    q = torch.randn(B, H, S, D, requires_grad=True)
    k = torch.randn(B, Hkv, S, D, requires_grad=True)
    v = torch.randn(B, Hkv, S, D, requires_grad=True)
    go = torch.randn(B, H, S, D)
    want = fwd_bwd(q, k, v, go)
    assert want[2].shape == k.shape and want[3].shape == v.shape

    gm = make_fx(fwd_bwd)(q, k, v, go)
    assert lower_sdpa(gm) == 1
    names = [getattr(n.target, "__name__", "") for n in gm.graph.nodes
             if n.op == "call_function"]
    assert names.count("flash_attention.default") == 1
    assert names.count("flash_attention_bwd.default") == 1
    assert not any("scaled_dot" in s for s in names)
    # the rewritten node still carries K/V of Hkv heads
    fa = next(n for n in gm.graph.nodes
              if n.op == "call_function"
              and n.target is ed.flash_attention.default)
    assert tuple(fa.args[1].meta["val"].shape) == (B, Hkv, S, D)
    got = gm(q, k, v, go)
    for name, a, b in zip(("out", "dq", "dk", "dv"), got, want):
        assert a.shape == b.shape, name
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5), \
            (name, float((a - b).abs().max()))


def test_gqa_gpt_compiled_matches_eager():
    from easydist_amd import easydist_compile, easydist_setup, set_device_mesh
    from easydist_amd.models.gpt import GPT, GPTConfig

    init_single_process()
    easydist_setup(device="cpu")
    set_device_mesh([0], ["spmd0"])
    torch.manual_seed(3)
    cfg = GPTConfig(vocab_size=128, n_layer=2, n_head=4, n_kv_head=2,
                    n_embd=32, block_size=32)
    model = GPT(cfg)
    # c_attn: (H + 2 Hkv) * hd = (4 + 4) * 8 columns
    assert model.h[0].attn.c_attn.weight.shape == (64, 32)
    model_ref = copy.deepcopy(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    opt_ref = torch.optim.Adam(model_ref.parameters(), lr=1e-3, fused=True)

    def train_step(model, opt, idx, targets):
        loss = model.loss(idx, targets)
        loss.backward()
        opt.step()
        opt.zero_grad(True)
        return loss

    compiled = easydist_compile(train_step, cuda_graph=False)
    torch.manual_seed(11)
    for step in range(3):
        idx = torch.randint(0, 128, (4, 32))
        tg = torch.randint(0, 128, (4, 32))
        loss = compiled(model, opt, idx, tg)
        ref = train_step(model_ref, opt_ref, idx, tg)
        assert abs(float(loss) - float(ref)) < 1e-3, (step, float(loss),
                                                      float(ref))
    final = compiled.named_parameters()
    for n, p_ref in model_ref.named_parameters():
        assert torch.allclose(final[n], p_ref.detach(), rtol=1e-3,
                              atol=1e-4), n

    # lower_attn_pack: one fused chain per layer, none left behind
    gm = list(compiled.compiled.values())[0].gm
    names = [getattr(n.target, "__name__", "") for n in gm.graph.nodes
             if n.op == "call_function"]
    assert names.count("flash_attention.default") == 2
    assert names.count("flash_attention_bwd_pack.default") == 2
    assert names.count("flash_attention_bwd.default") == 0


def test_mha_config_is_unchanged():
    """n_kv_head = None is the module of before: same parameter shapes, and
    n_kv_head = n_head the same numbers."""
    from easydist_amd.models.gpt import GPT, GPTConfig
    from easydist_amd.models.moe import MIXTRAL_8X7B, MIXTRAL_8X7B_GQA

    torch.manual_seed(0)
    a = GPT(GPTConfig(vocab_size=64, n_layer=1, n_head=4, n_embd=32,
                      block_size=16))
    torch.manual_seed(0)
    b = GPT(GPTConfig(vocab_size=64, n_layer=1, n_head=4, n_kv_head=4,
                      n_embd=32, block_size=16))
    assert a.h[0].attn.c_attn.weight.shape == (96, 32)
    idx = torch.randint(0, 64, (2, 16))
    assert torch.equal(a(idx), b(idx))
    assert MIXTRAL_8X7B.n_kv_head is None
    assert MIXTRAL_8X7B_GQA.n_kv_head == 8
    assert MIXTRAL_8X7B_GQA.n_head == MIXTRAL_8X7B.n_head == 32


def test_gpt_tp_rejects_gqa():
    from easydist_amd.models.gpt import GPTConfig
    from easydist_amd.models.gpt_tp import TPSelfAttention

    cfg = GPTConfig(vocab_size=64, n_layer=1, n_head=4, n_kv_head=2,
                    n_embd=32, block_size=16)
    with pytest.raises(AssertionError, match="multi-head"):
        TPSelfAttention(cfg, 1, None)


# ----------------------------------------------------------------- presets --
def _head_sid(ann, tensor_idx):
    """Shard ids annotated on dim 1 of one input tensor."""
    return [sid for sid in range(1, 8)
            if (tensor_idx, 1) in ann.positions_of(sid)]


def test_presets_gqa_head_rule_verified():
    import importlib
    presets = importlib.import_module("test_presets")
    from easydist_amd.compiler.preset_propagation import preset_meta_spmd

    torch.manual_seed(0)
    B, H, Hkv, S, D = 4, 4, 2, 8, 16
    q, k, v = torch.randn(B, H, S, D), torch.randn(B, Hkv, S, D), \
        torch.randn(B, Hkv, S, D)
    # forward: the batch and the head rule are executed and compared (the
    # sequence rule is runtime-realized)
    ann, combs = preset_meta_spmd(ed.flash_attention.default,
                                  [tuple(t.shape) for t in (q, k, v)],
                                  (q, k, v, True), {})
    sid = _head_sid(ann, 0)
    assert len(sid) == 1 and _head_sid(ann, 1) == sid \
        and _head_sid(ann, 2) == sid, "head rule must cover q, k and v"
    assert presets._run_case(ed.flash_attention.default, (q, k, v, True),
                             min_rules=2, atol=1e-5) == 2

    out, lse = ed.flash_attention(q, k, v, True)
    go = torch.randn_like(out)
    args = (go, q, k, v, out, lse, True)
    ann, combs = preset_meta_spmd(ed.flash_attention_bwd.default,
                                  [tuple(t.shape) for t in args[:6]],
                                  args, {})
    sid = _head_sid(ann, 1)
    assert len(sid) == 1
    for i in (0, 2, 3, 4, 5):
        assert _head_sid(ann, i) == sid, i
    assert presets._run_case(ed.flash_attention_bwd.default, args,
                             min_rules=2, atol=1e-5) == 2


def test_presets_no_head_shard_at_one_kv_head():
    from easydist_amd.compiler.preset_propagation import preset_meta_spmd

    B, H, S, D = 4, 4, 8, 16
    q, k, v = torch.randn(B, H, S, D), torch.randn(B, 1, S, D), \
        torch.randn(B, 1, S, D)
    out, lse = ed.flash_attention(q, k, v, True)
    go = torch.randn_like(out)
    cases = [
        (ed.flash_attention.default, (q, k, v, True), (1, 2)),
        (ed.flash_attention_bwd.default, (go, q, k, v, out, lse, True),
         (2, 3)),
        (aten._scaled_dot_product_flash_attention_for_cpu.default,
         (q, k, v, 0.0, True), (1, 2)),
        (aten._scaled_dot_product_flash_attention_for_cpu_backward.default,
         (go, q, k, v, out, lse, 0.0, True), (2, 3)),
    ]
    for op, args, kv_idx in cases:
        tensors = [a for a in args if isinstance(a, torch.Tensor)]
        ann, combs = preset_meta_spmd(op, [tuple(t.shape) for t in tensors],
                                      args, {})
        assert ann is not None and combs, op
        for i in range(len(tensors)):
            assert _head_sid(ann, i) == [], (op, i)
        # the batch rule is still there
        assert any((kv_idx[0], 0) in ann.positions_of(sid) for sid in combs)


# ---------------------------------------------------------- ring attention --
def _ring_body(world_size):
    import torch.distributed as dist

    from easydist_amd.ops.attention import scaled_dot_product_attention
    from easydist_amd.ops.ring_attention import ring_attention

    B, H, Hkv, S, D = 2, 4, 2, 16, 8
    r = dist.get_rank()
    torch.manual_seed(0)
    q = torch.randn(B, H, S, D)
    k = torch.randn(B, Hkv, S, D)
    v = torch.randn(B, Hkv, S, D)
    g = torch.randn(B, H, S, D)
    for t in (q, k, v, g):
        dist.broadcast(t, src=0)
    qf, kf, vf = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = scaled_dot_product_attention(qf, kf, vf, causal=True)
    ref.backward(g)
    assert kf.grad.shape == (B, Hkv, S, D)

    Sl = S // world_size
    sl = slice(r * Sl, (r + 1) * Sl)
    ql = q[:, :, sl].clone().requires_grad_(True)
    kl = k[:, :, sl].clone().requires_grad_(True)
    vl = v[:, :, sl].clone().requires_grad_(True)
    out = ring_attention(ql, kl, vl, group=dist.group.WORLD, causal=True)
    assert torch.allclose(out, ref.detach()[:, :, sl], rtol=1e-4, atol=1e-5)
    out.backward(g[:, :, sl])
    for got, want, name in ((ql.grad, qf.grad[:, :, sl], "dq"),
                            (kl.grad, kf.grad[:, :, sl], "dk"),
                            (vl.grad, vf.grad[:, :, sl], "dv")):
        assert got.shape == want.shape, name
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-5), \
            (name, float((got - want).abs().max()))


@pytest.mark.world2
def test_ring_attention_gqa_ws2():
    spawn(_ring_body, args=(2,), world_size=2, port=29711)
