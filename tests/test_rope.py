"""Rotary position embeddings on the CPU: the op's formula, its autograd and
input errors, the tables, the sharding preset, and the rope=True models
through the compiler, the MoE model and sequence parallelism.
"""
import copy
import math

import pytest
import torch

import easydist_amd.ops  # noqa: F401  (registers custom ops + presets)
from easydist_amd.ops.rope import apply_rope, rope_tables
from easydist_amd.utils.testing import init_single_process, spawn

ed = torch.ops.easydist_amd


def _rotate_half(x):
    x1, x2 = x[..., :x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def _hf_reference(qkv, cos, sin, H, Hkv):
    """HuggingFace style: split, view as heads, q*cos + rotate_half(q)*sin
    with the tables repeated over both halves."""
    B, S, W = qkv.shape
    D = W // (H + 2 * Hkv)
    q, k, v = qkv.split([H * D, Hkv * D, Hkv * D], dim=2)
    q = q.view(B, S, H, D)
    k = k.view(B, S, Hkv, D)
    c = torch.cat((cos, cos), dim=-1)[None, :, None, :].to(qkv.dtype)
    s = torch.cat((sin, sin), dim=-1)[None, :, None, :].to(qkv.dtype)
    q = q * c + _rotate_half(q) * s
    k = k * c + _rotate_half(k) * s
    return torch.cat((q.reshape(B, S, H * D), k.reshape(B, S, Hkv * D), v),
                     dim=2)


def _tables64(S, D, p=0, base=10000.0):
    """fp64 tables of positions p .. p+S-1."""
    j = torch.arange(D // 2, dtype=torch.float64)
    ang = torch.arange(p, p + S, dtype=torch.float64)[:, None] \
        * base ** (-2.0 * j / D)
    return ang.cos(), ang.sin()


# ------------------------------------------------------------------ formula --
@pytest.mark.parametrize("B,S,H,Hkv,D", [(2, 5, 4, 2, 16), (1, 3, 2, 2, 32)])
def test_formula_matches_rotate_half(B, S, H, Hkv, D):
    torch.manual_seed(0)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * D)
    cos, sin = rope_tables(S, D)
    out = ed.rope_qkv(qkv, cos, sin, H, Hkv, False)
    ref = _hf_reference(qkv, cos, sin, H, Hkv)
    assert out.shape == qkv.shape and out.dtype == qkv.dtype
    assert out.is_contiguous()
    assert torch.allclose(out, ref, rtol=1e-6, atol=1e-6), \
        float((out - ref).abs().max())
    assert torch.equal(out[..., (H + Hkv) * D:], qkv[..., (H + Hkv) * D:])
    assert torch.equal(apply_rope(qkv, cos, sin, H, Hkv), out)


def test_relative_position_property():
    """q_rot . k_rot depends on the distance of the two positions only."""
    torch.manual_seed(1)
    B, S, H, D = 2, 6, 2, 16
    qkv = torch.randn(B, S, 3 * H * D, dtype=torch.float64)
    scores = []
    for p in (0, 7):
        cos, sin = _tables64(S, D, p)
        out = ed.rope_qkv(qkv, cos, sin, H, H, False)
        q, k, _ = out.split(H * D, dim=2)
        q = q.view(B, S, H, D).transpose(1, 2)
        k = k.view(B, S, H, D).transpose(1, 2)
        scores.append(q @ k.transpose(-1, -2))
    assert torch.allclose(scores[0], scores[1], rtol=0, atol=1e-10), \
        float((scores[0] - scores[1]).abs().max())
    # ... and is not what unrotated q and k give
    q, k, _ = qkv.split(H * D, dim=2)
    plain = q.view(B, S, H, D).transpose(1, 2) \
        @ k.view(B, S, H, D).transpose(1, 2).transpose(-1, -2)
    assert not torch.allclose(scores[0], plain, atol=1e-3)


# ----------------------------------------------------------------- autograd --
def test_gradcheck_fp64():
    torch.manual_seed(2)
    B, S, H, Hkv, D = 1, 3, 2, 1, 16
    cos, sin = rope_tables(S, D)
    x = torch.randn(B, S, (H + 2 * Hkv) * D, dtype=torch.float64,
                    requires_grad=True)
    for inverse in (False, True):
        assert torch.autograd.gradcheck(
            lambda t: ed.rope_qkv(t, cos, sin, H, Hkv, inverse), (x,))


def test_inverse_undoes_forward_fp64():
    torch.manual_seed(3)
    B, S, H, Hkv, D = 2, 5, 4, 2, 16
    cos, sin = _tables64(S, D)
    x = torch.randn(B, S, (H + 2 * Hkv) * D, dtype=torch.float64)
    y = ed.rope_qkv(x, cos, sin, H, Hkv, False)
    back = ed.rope_qkv(y, cos, sin, H, Hkv, True)
    assert not torch.allclose(y, x, atol=1e-3)
    assert torch.allclose(back, x, rtol=0, atol=1e-12), \
        float((back - x).abs().max())


def test_backward_is_inverse_op():
    torch.manual_seed(4)
    B, S, H, Hkv, D = 2, 5, 4, 2, 16
    cos, sin = rope_tables(S, D)
    x = torch.randn(B, S, (H + 2 * Hkv) * D, requires_grad=True)
    g = torch.randn_like(x)
    (dx,) = torch.autograd.grad((apply_rope(x, cos, sin, H, Hkv) * g).sum(),
                                x)
    assert torch.equal(dx, ed.rope_qkv(g, cos, sin, H, Hkv, True))


# ------------------------------------------------------------------- errors --
def test_input_errors():
    B, S, H, Hkv, D = 2, 5, 4, 2, 16
    qkv = torch.randn(B, S, (H + 2 * Hkv) * D)
    cos, sin = rope_tables(S, D)
    with pytest.raises(ValueError, match=r"\(2, 5, 128\)"):
        ed.rope_qkv(qkv, cos, sin, H, Hkv + 1, False)      # W mismatch
    with pytest.raises(ValueError, match=r"\(5, 8\).*\(5, 4\)"):
        ed.rope_qkv(qkv, cos, sin[:, :4], H, Hkv, False)   # cos != sin
    cos4, sin4 = rope_tables(S - 1, D)
    with pytest.raises(ValueError, match=r"\(4, 8\).*\(2, 5, 128\)"):
        ed.rope_qkv(qkv, cos4, sin4, H, Hkv, False)        # rows != S


def test_half_precision_tables_are_rejected():
    qkv = torch.randn(1, 3, 3 * 16)
    cos, sin = rope_tables(3, 16)
    with pytest.raises(AssertionError, match="fp32"):
        ed.rope_qkv(qkv, cos.bfloat16(), sin.bfloat16(), 1, 1, False)


# ------------------------------------------------------------------- tables --
def test_rope_tables():
    S, D = 9, 16
    cos, sin = rope_tables(S, D)
    assert cos.shape == sin.shape == (S, D // 2)
    assert cos.dtype == sin.dtype == torch.float32
    assert torch.equal(cos[0], torch.ones(D // 2))
    assert torch.equal(sin[0], torch.zeros(D // 2))
    for pos, j in ((1, 0), (3, 2), (8, 7), (5, 4)):
        ang = pos * 10000.0 ** (-2.0 * j / D)
        assert abs(float(cos[pos, j]) - math.cos(ang)) < 1e-6
        assert abs(float(sin[pos, j]) - math.sin(ang)) < 1e-6
    cos6, sin6 = rope_tables(S, D, base=1e6)
    ang = 8 * 1e6 ** (-2.0 * 3 / D)
    assert abs(float(cos6[8, 3]) - math.cos(ang)) < 1e-6
    assert abs(float(sin6[8, 3]) - math.sin(ang)) < 1e-6


# ------------------------------------------------------------------- preset --
def test_preset_rule():
    import importlib
    presets = importlib.import_module("test_presets")
    from easydist_amd.compiler.preset_propagation import preset_meta_spmd

    torch.manual_seed(5)
    B, S, H, Hkv, D = 4, 6, 2, 1, 16
    qkv = torch.randn(B, S, (H + 2 * Hkv) * D)
    cos, sin = rope_tables(S, D)
    args = (qkv, cos, sin, H, Hkv, False)
    # both rules are executed shard by shard and compared
    assert presets._run_case(ed.rope_qkv.default, args, min_rules=2) == 2
    ann, combs = preset_meta_spmd(
        ed.rope_qkv.default, [tuple(t.shape) for t in (qkv, cos, sin)],
        args, {})
    groups = sorted(sorted(ann.positions_of(sid)) for sid in combs)
    assert groups == [[(0, 0)], [(0, 1), (1, 0), (2, 0)]], groups
    # nothing on the packed column dim, nothing on the tables' columns
    for sid in range(1, 8):
        pos = ann.positions_of(sid)
        assert (0, 2) not in pos and (1, 1) not in pos and (2, 1) not in pos
    # a dim of size 1 is skipped
    ann1, combs1 = preset_meta_spmd(
        ed.rope_qkv.default, [(1, S, 64), (S, 8), (S, 8)],
        (qkv[:1], cos, sin, H, Hkv, False), {})
    assert [sorted(ann1.positions_of(sid)) for sid in combs1] \
        == [[(0, 1), (1, 0), (2, 0)]]


# ------------------------------------------------------------------ compile --
def _train_step(model, opt, idx, targets):
    loss = model.loss(idx, targets)
    loss.backward()
    opt.step()
    opt.zero_grad(True)
    return loss


def _node_names(compiled):
    gm = list(compiled.compiled.values())[0].gm
    nodes = [n for n in gm.graph.nodes if n.op == "call_function"]
    return nodes, [getattr(n.target, "__name__", "") for n in nodes]


def test_rope_gpt_compiled_matches_eager():
    from easydist_amd import easydist_compile, easydist_setup, set_device_mesh
    from easydist_amd.models.gpt import GPT, GPTConfig

    init_single_process()
    easydist_setup(device="cpu")
    set_device_mesh([0], ["spmd0"])
    torch.manual_seed(3)
    cfg = GPTConfig(vocab_size=128, n_layer=2, n_head=4, n_kv_head=2,
                    n_embd=32, block_size=32, rope=True)
    model = GPT(cfg)
    names = [n for n, _ in model.named_parameters()]
    assert "wpe.weight" not in names
    assert model.rope_cos.shape == model.rope_sin.shape == (32, 4)
    assert model.rope_cos.dtype == torch.float32
    assert "rope_cos" not in model.state_dict()
    model_ref = copy.deepcopy(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    opt_ref = torch.optim.Adam(model_ref.parameters(), lr=1e-3, fused=True)

    compiled = easydist_compile(_train_step, cuda_graph=False)
    torch.manual_seed(11)
    for step in range(3):
        idx = torch.randint(0, 128, (4, 32))
        tg = torch.randint(0, 128, (4, 32))
        loss = compiled(model, opt, idx, tg)
        ref = _train_step(model_ref, opt_ref, idx, tg)
        assert abs(float(loss) - float(ref)) < 1e-3, (step, float(loss),
                                                      float(ref))
    final = compiled.named_parameters()
    for n, p_ref in model_ref.named_parameters():
        assert torch.allclose(final[n], p_ref.detach(), rtol=1e-3,
                              atol=1e-4), n

    nodes, names = _node_names(compiled)
    ropes = [n for n in nodes if n.target is ed.rope_qkv.default]
    assert sorted(bool(n.args[5]) for n in ropes) \
        == [False, False, True, True]
    # the packed attention backward still fuses: its cat now feeds the
    # inverse rotation
    assert names.count("flash_attention_bwd_pack.default") == 2
    assert names.count("flash_attention_bwd.default") == 0


def test_rope_false_is_unchanged():
    from easydist_amd import easydist_compile, easydist_setup, set_device_mesh
    from easydist_amd.models.gpt import GPT, GPTConfig

    init_single_process()
    easydist_setup(device="cpu")
    set_device_mesh([0], ["spmd0"])
    torch.manual_seed(3)
    cfg = GPTConfig(vocab_size=128, n_layer=2, n_head=4, n_kv_head=2,
                    n_embd=32, block_size=32, rope=False)
    model = GPT(cfg)
    assert "wpe.weight" in [n for n, _ in model.named_parameters()]
    assert not hasattr(model, "rope_cos")
    # the same parameters and numbers as a config that never names rope
    torch.manual_seed(3)
    base = GPT(GPTConfig(vocab_size=128, n_layer=2, n_head=4, n_kv_head=2,
                         n_embd=32, block_size=32))
    idx = torch.randint(0, 128, (4, 32))
    assert torch.equal(model(idx), base(idx))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    compiled = easydist_compile(_train_step, cuda_graph=False)
    compiled(model, opt, idx, torch.randint(0, 128, (4, 32)))
    _, names = _node_names(compiled)
    assert names.count("rope_qkv.default") == 0
    assert names.count("flash_attention_bwd_pack.default") == 2


def test_rope_changes_the_model_output():
    """Positions enter: permuting earlier tokens changes the last logits of
    a rope model (it would not without any position information)."""
    from easydist_amd.models.gpt import GPT, GPTConfig

    torch.manual_seed(0)
    model = GPT(GPTConfig(vocab_size=64, n_layer=1, n_head=2, n_embd=32,
                          block_size=16, rope=True))
    idx = torch.randint(0, 64, (1, 16))
    swapped = idx.clone()
    swapped[0, 0], swapped[0, 5] = idx[0, 5], idx[0, 0]
    assert idx[0, 0] != idx[0, 5]
    a, b = model(idx)[0, -1], model(swapped)[0, -1]
    assert not torch.allclose(a, b, atol=1e-6)


# ---------------------------------------------------------------------- MoE --
def test_moe_rope_forward_backward():
    import dataclasses

    from easydist_amd.models.moe import MIXTRAL_SMALL, MoEGPT

    torch.manual_seed(0)
    cfg = dataclasses.replace(MIXTRAL_SMALL, rope=True)
    model = MoEGPT(cfg)
    assert "wpe.weight" not in [n for n, _ in model.named_parameters()]
    assert model.rope_cos.shape == (cfg.block_size,
                                    cfg.n_embd // cfg.n_head // 2)
    idx = torch.randint(0, cfg.vocab_size, (2, 32))
    tg = torch.randint(0, cfg.vocab_size, (2, 32))
    loss = model.loss(idx, tg)
    assert torch.isfinite(loss)
    loss.backward()
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n


def test_mixtral_rope_config():
    from easydist_amd.models.moe import (MIXTRAL_8X7B, MIXTRAL_8X7B_GQA,
                                         MIXTRAL_8X7B_ROPE)

    assert MIXTRAL_8X7B_ROPE.n_kv_head == 8
    assert MIXTRAL_8X7B_ROPE.rope is True
    assert MIXTRAL_8X7B_ROPE.rope_base == 1e6
    assert MIXTRAL_8X7B_ROPE.n_layer == 32
    assert not MIXTRAL_8X7B.rope and not MIXTRAL_8X7B_GQA.rope


# -------------------------------------------------------- sequence parallel --
def _gpt_sp_body(world_size):
    import torch.distributed as dist

    from easydist_amd.models.gpt import GPT, GPTConfig

    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=64, n_layer=1, n_head=2, n_embd=32,
                    block_size=32, rope=True)
    model = GPT(cfg)
    for p in model.parameters():
        dist.broadcast(p.data, src=0)
    model_ref = copy.deepcopy(model)
    model.enable_sequence_parallel(dist.group.WORLD)

    torch.manual_seed(3)
    idx = torch.randint(0, 64, (2, 32))
    dist.broadcast(idx, src=0)
    r = dist.get_rank()
    Sl = 32 // world_size
    sl = slice(r * Sl, (r + 1) * Sl)
    with torch.no_grad():
        logits = model(idx[:, sl])
        ref = model_ref(idx)[:, sl]
    assert logits.shape == ref.shape
    assert torch.allclose(logits, ref, rtol=0, atol=1e-4), \
        (r, float((logits - ref).abs().max()))


@pytest.mark.world2
def test_rope_gpt_sequence_parallel_ws2():
    spawn(_gpt_sp_body, args=(2,), world_size=2, port=29721)
