"""Fused SwiGLU on the CPU: the ops against `F.silu(a) * b` and its autograd,
the shape contract, the fakes, the sharding preset, the lower_swiglu pass on
traced graphs, and the mlp="swiglu" GPT through the compiler.
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.fx.experimental.proxy_tensor import make_fx

import easydist_amd.ops  # noqa: F401  (registers custom ops + presets)
from easydist_amd.ops import swiglu as sw
from easydist_amd.utils.testing import init_single_process, spawn

ed = torch.ops.easydist_amd
aten = torch.ops.aten


# ----------------------------------------------------------------------- op --
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", [(3, 8), (2, 5, 12), (7,)])
def test_op_is_the_aten_chain_bit_for_bit(dtype, shape):
    torch.manual_seed(0)
    a = (3 * torch.randn(shape, dtype=dtype)).requires_grad_(True)
    b = torch.randn(shape, dtype=dtype, requires_grad=True)
    g = torch.randn(shape, dtype=dtype)
    want = F.silu(a) * b
    da, db = torch.autograd.grad(want, (a, b), g)
    got = sw.swiglu(a, b)
    assert got.dtype == dtype and got.shape == want.shape
    assert torch.equal(got, want)
    ga, gb = torch.autograd.grad(got, (a, b), g)
    assert torch.equal(ga, da) and torch.equal(gb, db)
    dgate, dup = ed.swiglu_bwd(g, a.detach(), b.detach())
    assert torch.equal(dgate, da) and torch.equal(dup, db)


def test_gradcheck_fp64():
    torch.manual_seed(1)
    a = (2 * torch.randn(3, 8, dtype=torch.float64)).requires_grad_(True)
    b = torch.randn(3, 8, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(sw.swiglu, (a, b))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_precision_is_the_fp32_formula_rounded_once(dtype):
    torch.manual_seed(2)
    a = (4 * torch.randn(5, 24)).to(dtype)
    b = torch.randn(5, 24).to(dtype)
    g = torch.randn(5, 24).to(dtype)
    a32, b32, g32 = a.float(), b.float(), g.float()
    s = torch.sigmoid(a32)
    out = sw.swiglu(a, b)
    dgate, dup = ed.swiglu_bwd(g, a, b)
    assert out.dtype == dgate.dtype == dup.dtype == dtype
    a64, b64, g64 = a.double(), b.double(), g.double()
    s64 = 1.0 / (1.0 + torch.exp(-a64))
    for got, want32, want64 in (
            (out, a32 * s * b32, a64 * s64 * b64),
            (dup, g32 * a32 * s, g64 * a64 * s64),
            (dgate, g32 * b32 * s * (1.0 + a32 * (1.0 - s)),
             g64 * b64 * s64 * (1.0 + a64 * (1.0 - s64)))):
        assert torch.equal(got, want32.to(dtype))
        # one rounding of the exact value: half an ulp of bf16 is 2^-9 of
        # the next power of two below, so 2^-8 of the value at the most
        assert bool(((got.double() - want64).abs()
                     <= 2.0 ** -8 * want64.abs() + 1e-7).all())
    # the same through autograd
    a2 = a.clone().requires_grad_(True)
    b2 = b.clone().requires_grad_(True)
    ga, gb = torch.autograd.grad(sw.swiglu(a2, b2), (a2, b2), g)
    assert torch.equal(ga, dgate) and torch.equal(gb, dup)


def test_overflowing_gate_gives_zeros():
    a = torch.full((2, 8), -200.0, dtype=torch.bfloat16)
    b = torch.randn(2, 8).to(torch.bfloat16)
    g = torch.randn(2, 8).to(torch.bfloat16)
    for t in (sw.swiglu(a, b),) + tuple(ed.swiglu_bwd(g, a, b)):
        assert torch.isfinite(t).all() and not t.any()


def test_shape_contract():
    a, b = torch.randn(4, 8), torch.randn(4, 8)
    with pytest.raises(ValueError, match=r"\(4, 8\).*\(4, 1\)"):
        sw.swiglu(a, b[:, :1])                       # would broadcast
    with pytest.raises(ValueError, match=r"\(4, 8\).*\(8,\)"):
        sw.swiglu(a, b[0])
    with pytest.raises(ValueError, match="float64"):
        sw.swiglu(a, b.double())
    with pytest.raises(ValueError, match=r"\(1, 8\).*\(4, 8\).*\(4, 8\)"):
        ed.swiglu_bwd(a[:1], a, b)
    with pytest.raises(ValueError, match=r"\(4, 8\).*\(4, 8\).*\(4, 4\)"):
        ed.swiglu_bwd(a, a, b[:, :4])


def test_fakes_match_real_outputs_for_strided_inputs():
    from torch._subclasses.fake_tensor import FakeTensorMode

    torch.manual_seed(3)
    h = torch.randn(6, 32)
    cases = [
        h.chunk(2, -1),                               # halves of one buffer
        (h[1::2, :16], h[::2, 16:]),                  # row slices
        (h[:, :16].t(), h[:, 16:].t()),               # transposed views
        (torch.randn(2, 3, 8).transpose(0, 1), torch.randn(3, 2, 8)),
    ]
    for a, b in cases:
        g = torch.randn(a.shape)
        out = ed.swiglu(a, b)
        dgate, dup = ed.swiglu_bwd(g, a, b)
        with FakeTensorMode() as mode:
            fa, fb, fg = (mode.from_tensor(t) for t in (a, b, g))
            f_out = ed.swiglu(fa, fb)
            f_dgate, f_dup = ed.swiglu_bwd(fg, fa, fb)
        for real, fake in ((out, f_out), (dgate, f_dgate), (dup, f_dup)):
            assert real.shape == fake.shape and real.dtype == fake.dtype
            assert real.stride() == fake.stride()
            assert real.is_contiguous() and fake.is_contiguous()
        assert torch.equal(out, F.silu(a) * b)


def test_kernel_envelope():
    """_kernel_ok on CPU tensors: it reads dtype, shape and strides only."""
    bf = torch.bfloat16
    h = torch.zeros(6, 32, dtype=bf)
    a, b = h.chunk(2, -1)
    assert sw._kernel_ok(a, b)
    assert sw._kernel_ok(h[1::2], h[::2])
    assert sw._kernel_ok(torch.zeros(2, 3, 16, dtype=bf),
                         torch.zeros(2, 3, 32, dtype=bf)[..., :16])
    assert sw._kernel_ok(torch.zeros(1, 8, dtype=bf), torch.zeros(1, 8,
                                                                  dtype=bf))
    assert not sw._kernel_ok(h[:, :12], h[:, 16:28])          # F % 8
    assert not sw._kernel_ok(h[:, 1:9], h[:, 16:24])          # misaligned
    assert not sw._kernel_ok(h.float(), h.float())            # dtype
    assert not sw._kernel_ok(h.t(), h.t())                    # last stride
    assert not sw._kernel_ok(h[:0], h[:0])                    # empty
    # a row stride of 36 is no multiple of 8
    assert not sw._kernel_ok(torch.zeros(6, 36, dtype=bf)[:, :32], h)
    x = torch.zeros(4, 3, 16, dtype=bf)
    assert not sw._kernel_ok(x.transpose(0, 1), x.transpose(0, 1))
    assert sw._kernel_ok(x[:, :2], x[:, 1:]) is False   # rows do not collapse
    assert sw._kernel_ok(x[:, :1], x[:, 2:])             # size-1 dim: they do


# ------------------------------------------------------------------- preset --
def test_preset_rules():
    import importlib
    presets = importlib.import_module("test_presets")
    from easydist_amd.compiler.preset_propagation import preset_meta_spmd

    torch.manual_seed(5)
    a, b, g = (torch.randn(4, 6, 8) for _ in range(3))
    # every dim is offered, executed shard by shard and recombined
    assert presets._run_case(ed.swiglu.default, (a, b), min_rules=3) == 3
    assert presets._run_case(ed.swiglu_bwd.default, (g, a, b),
                             min_rules=3) == 3
    ann, combs = preset_meta_spmd(ed.swiglu_bwd.default, [(4, 6, 8)] * 3,
                                  (g, a, b), {})
    groups = sorted(sorted(ann.positions_of(sid)) for sid in combs)
    assert groups == [[(0, d), (1, d), (2, d)] for d in range(3)], groups
    assert all(isinstance(c, list) and len(c) == 2 for c in combs.values())
    # a dim of size 1 is skipped
    ann1, combs1 = preset_meta_spmd(ed.swiglu.default, [(1, 6, 8)] * 2,
                                    (a[:1], b[:1]), {})
    assert sorted(sorted(ann1.positions_of(sid)) for sid in combs1) \
        == [[(0, 1), (1, 1)], [(0, 2), (1, 2)]]


# --------------------------------------------------------------------- pass --
def _targets(gm):
    return [n.target for n in gm.graph.nodes if n.op == "call_function"]


def _expert_ffn(x, w1, w3, w2, go):
    """ExpertFFN.forward (models/moe.py) and its backward."""
    a = torch.bmm(x, w1)
    b = torch.bmm(x, w3)
    y = torch.bmm(F.silu(a) * b, w2)
    return (y,) + torch.autograd.grad(y, (x, w1, w3, w2), go)


def _dense_mlp(x, w1, w3, w2, go):
    """A Llama-style 2-D MLP, the up projection written first."""
    y = (x @ w3 * F.silu(x @ w1)) @ w2
    return (y,) + torch.autograd.grad(y, (x, w1, w3, w2), go)


def _ffn_inputs(batched, dtype=torch.float32):
    torch.manual_seed(7)
    lead = (2,) if batched else ()
    x = torch.randn(lead + (6, 8), dtype=dtype, requires_grad=True)
    w1 = torch.randn(lead + (8, 16), dtype=dtype, requires_grad=True)
    w3 = torch.randn(lead + (8, 16), dtype=dtype, requires_grad=True)
    w2 = torch.randn(lead + (16, 8), dtype=dtype, requires_grad=True)
    go = torch.randn(lead + (6, 8), dtype=dtype)
    return x, w1, w3, w2, go


@pytest.mark.parametrize("fn,batched", [(_expert_ffn, True),
                                        (_dense_mlp, False)])
def test_lower_swiglu_forward_and_backward(fn, batched):
    from easydist_amd.compiler.passes.lower_hip import lower_swiglu

    args = _ffn_inputs(batched)
    gm = make_fx(fn)(*args)
    before = _targets(gm)
    assert before.count(aten.silu.default) == 1
    assert before.count(aten.silu_backward.default) == 1
    assert before.count(aten.mul.Tensor) == 3
    want = gm(*args)
    assert lower_swiglu(gm) == 2          # one forward, one backward
    after = _targets(gm)
    assert after.count(ed.swiglu.default) == 1
    assert after.count(ed.swiglu_bwd.default) == 1
    assert aten.silu.default not in after
    assert aten.silu_backward.default not in after
    assert aten.mul.Tensor not in after
    # the backward reads the forward's operands, nothing saved in between
    fwd = next(n for n in gm.graph.nodes if n.target is ed.swiglu.default)
    bwd = next(n for n in gm.graph.nodes if n.target is ed.swiglu_bwd.default)
    assert tuple(bwd.args[1:]) == tuple(fwd.args)
    got = gm(*args)
    assert len(got) == len(want) == 5
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert lower_swiglu(gm) == 0          # nothing left to do


def test_lower_swiglu_every_operand_order_swapped():
    """The chain written by hand with each mul the other way round from
    what autograd emits for silu(a) * b."""
    from easydist_amd.compiler.passes.lower_hip import lower_swiglu

    def fn(a, b, g):
        s = aten.silu(a)
        return (aten.mul(b, s), aten.silu_backward(aten.mul(b, g), a),
                aten.mul(s, g))

    torch.manual_seed(6)
    a, b, g = 2 * torch.randn(5, 8), torch.randn(5, 8), torch.randn(5, 8)
    gm = make_fx(fn)(a, b, g)
    want = gm(a, b, g)
    assert lower_swiglu(gm) == 2
    after = _targets(gm)
    assert after.count(ed.swiglu.default) == 1
    assert after.count(ed.swiglu_bwd.default) == 1
    assert aten.silu.default not in after and aten.mul.Tensor not in after
    for x, y in zip(gm(a, b, g), want):
        assert torch.equal(x, y)
    da, db = torch.autograd.grad(
        F.silu(a.requires_grad_(True)) * b.requires_grad_(True), (a, b), g)
    assert torch.equal(want[1], da) and torch.equal(want[2], db)


def test_lower_swiglu_stacked():
    """One activation feeding the next: the second match's operands are
    nodes that the first rewrite created."""
    from easydist_amd.compiler.passes.lower_hip import lower_swiglu

    def fn(a, b, c):
        y = F.silu(F.silu(a) * b) * c
        return (y,) + torch.autograd.grad(y.square().sum(), (a, b, c))

    torch.manual_seed(12)
    a, b, c = (torch.randn(4, 8, requires_grad=True) for _ in range(3))
    gm = make_fx(fn)(a, b, c)
    want = gm(a, b, c)
    assert lower_swiglu(gm) == 4
    after = _targets(gm)
    assert after.count(ed.swiglu.default) == 2
    assert after.count(ed.swiglu_bwd.default) == 2
    assert aten.silu.default not in after
    assert aten.silu_backward.default not in after
    for x, y in zip(gm(a, b, c), want):
        assert torch.equal(x, y)


def test_lower_swiglu_forward_only():
    from easydist_amd.compiler.passes.lower_hip import lower_swiglu

    x, w1, w3, w2, _ = (t.detach() for t in _ffn_inputs(True))

    def fwd(x, w1, w3, w2):
        return torch.bmm(torch.bmm(x, w3) * F.silu(torch.bmm(x, w1)), w2)

    gm = make_fx(fwd)(x, w1, w3, w2)
    want = gm(x, w1, w3, w2)
    assert lower_swiglu(gm) == 1
    after = _targets(gm)
    assert after.count(ed.swiglu.default) == 1
    assert aten.silu.default not in after and aten.mul.Tensor not in after
    assert torch.equal(gm(x, w1, w3, w2), want)


def test_lower_swiglu_leaves_a_broadcast_alone():
    """Nothing fuses: the forward broadcasts, and with it the backward has
    no triple (its gradient comes from the loss, as in a train step)."""
    from easydist_amd.compiler.passes.lower_hip import lower_swiglu

    def fn(a, b):
        y = F.silu(a) * b[..., :1]
        return (y,) + torch.autograd.grad(y.square().sum(), (a, b))

    torch.manual_seed(8)
    a = torch.randn(4, 8, requires_grad=True)
    b = torch.randn(4, 8, requires_grad=True)
    gm = make_fx(fn)(a, b)
    before = _targets(gm)
    assert before.count(aten.silu.default) == 1
    assert before.count(aten.silu_backward.default) == 1
    assert lower_swiglu(gm) == 0
    assert _targets(gm) == before


def test_lower_swiglu_leaves_a_cast_alone():
    """silu in fp32 of a bf16 gate, times a bf16 up: a cast in between."""
    from easydist_amd.compiler.passes.lower_hip import lower_swiglu

    def fn(a, b):
        return F.silu(a.float()) * b

    a = torch.randn(4, 8).bfloat16()
    b = torch.randn(4, 8).bfloat16()
    gm = make_fx(fn)(a, b)
    assert lower_swiglu(gm) == 0
    assert aten.silu.default in _targets(gm)


def test_lower_swiglu_silu_with_an_extra_user():
    """Both halves fuse; the silu stays for its other user."""
    from easydist_amd.compiler.passes.lower_hip import lower_swiglu

    def fn(a, b, go):
        s = F.silu(a)
        y = s * b
        return (y, s.detach() + 1.0) + torch.autograd.grad(y, (a, b), go)

    torch.manual_seed(9)
    a = torch.randn(4, 8, requires_grad=True)
    b = torch.randn(4, 8, requires_grad=True)
    go = torch.randn(4, 8)
    gm = make_fx(fn)(a, b, go)
    want = gm(a, b, go)
    assert lower_swiglu(gm) == 2
    after = _targets(gm)
    assert after.count(ed.swiglu.default) == 1
    assert after.count(ed.swiglu_bwd.default) == 1
    assert after.count(aten.silu.default) == 1
    assert aten.silu_backward.default not in after
    assert aten.mul.Tensor not in after
    for x, y in zip(gm(a, b, go), want):
        assert torch.equal(x, y)


def test_lower_swiglu_partial_backward_is_left_alone():
    """Only d-up is asked for: there is no silu_backward, so the backward's
    mul(g, silu), whose g comes from the loss, stays aten while the forward
    fuses."""
    from easydist_amd.compiler.passes.lower_hip import lower_swiglu

    def fn(a, b):
        y = F.silu(a) * b
        return (y,) + torch.autograd.grad(y.square().sum(), (b,))

    torch.manual_seed(10)
    a = torch.randn(4, 8)
    b = torch.randn(4, 8, requires_grad=True)
    gm = make_fx(fn)(a, b)
    want = gm(a, b)
    n_mul = _targets(gm).count(aten.mul.Tensor)
    assert lower_swiglu(gm) == 1
    after = _targets(gm)
    assert after.count(ed.swiglu.default) == 1
    assert ed.swiglu_bwd.default not in after
    assert after.count(aten.mul.Tensor) == n_mul - 1   # d-up is untouched
    assert after.count(aten.silu.default) == 1
    for x, y in zip(gm(a, b), want):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ compile --
class _LlamaMLP(nn.Module):
    def __init__(self, d=16, h=32):
        super().__init__()
        self.gate_proj = nn.Linear(d, h, bias=False)
        self.up_proj = nn.Linear(d, h, bias=False)
        self.down_proj = nn.Linear(h, d, bias=False)

    def forward(self, x):
        return self.down_proj(F.silu(self.gate_proj(x)) * self.up_proj(x))


def _mlp_step(model, opt, x, y):
    loss = F.mse_loss(model(x), y)
    loss.backward()
    opt.step()
    opt.zero_grad(True)
    return loss


def _names(compiled):
    gm = list(compiled.compiled.values())[0].gm
    return [getattr(n.target, "__name__", "") for n in gm.graph.nodes
            if n.op == "call_function"]


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_compiled_step_fuses_unless_switched_off(monkeypatch, fuse):
    from easydist_amd import easydist_compile, easydist_setup, set_device_mesh

    monkeypatch.setenv("EASYDIST_SWIGLU_FUSE", fuse)
    init_single_process()
    easydist_setup(device="cpu")
    set_device_mesh([0], ["spmd0"])
    torch.manual_seed(0)
    model = _LlamaMLP()
    ref = copy.deepcopy(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3, fused=True)
    x, y = torch.randn(8, 16), torch.randn(8, 16)
    compiled = easydist_compile(_mlp_step, cuda_graph=False)
    loss = compiled(model, opt, x, y)
    want = _mlp_step(ref, opt_ref, x, y)
    assert abs(float(loss) - float(want.detach())) < 1e-6
    names = _names(compiled)
    if fuse == "1":
        assert names.count("swiglu.default") == 1
        assert names.count("swiglu_bwd.default") == 1
        assert "silu.default" not in names
        assert "silu_backward.default" not in names
    else:
        assert names.count("silu.default") == 1
        assert names.count("silu_backward.default") == 1
        assert "swiglu.default" not in names


# ------------------------------------------------------------------- models --
def _gpt_cfg(**kw):
    from easydist_amd.models.gpt import GPTConfig
    return GPTConfig(vocab_size=128, n_layer=2, n_head=4, n_embd=64,
                     block_size=32, **kw)


def _train_step(model, opt, idx, targets):
    loss = model.loss(idx, targets)
    loss.backward()
    opt.step()
    opt.zero_grad(True)
    return loss


def _swiglu_gpt_body(world_size):
    import torch.distributed as dist

    from easydist_amd import easydist_compile, easydist_setup, set_device_mesh
    from easydist_amd.models.gpt import GPT

    easydist_setup(backend="torch", device="cpu")
    set_device_mesh(list(range(world_size)), ["spmd0"])
    torch.manual_seed(3)
    model = GPT(_gpt_cfg(mlp="swiglu"))
    for p in model.parameters():
        dist.broadcast(p.data, src=0)
    model_ref = copy.deepcopy(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    opt_ref = torch.optim.Adam(model_ref.parameters(), lr=1e-3, fused=True)
    compiled = easydist_compile(_train_step, cuda_graph=False)
    torch.manual_seed(11)
    for step in range(2):
        idx = torch.randint(0, 128, (4, 32))
        tg = torch.randint(0, 128, (4, 32))
        dist.broadcast(idx, src=0)
        dist.broadcast(tg, src=0)
        loss = compiled(model, opt, idx, tg)
        ref = _train_step(model_ref, opt_ref, idx, tg)
        assert abs(float(loss) - float(ref)) < 5e-3, (step, float(loss),
                                                      float(ref))
    names = _names(compiled)
    assert names.count("swiglu.default") == 2
    assert names.count("swiglu_bwd.default") == 2
    assert "gelu.default" not in names and "silu.default" not in names


def test_swiglu_gpt_compiled_matches_eager_ws1():
    init_single_process()
    _swiglu_gpt_body(1)


@pytest.mark.world2
def test_swiglu_gpt_compiled_matches_eager_ws2():
    spawn(_swiglu_gpt_body, args=(2,), world_size=2, port=29731)


def test_swiglu_mlp_block():
    from easydist_amd.models.gpt import GPT, GPTConfig, MLPBlock

    torch.manual_seed(0)
    model = GPT(_gpt_cfg(mlp="swiglu"))
    mlp = model.h[0].mlp
    # 8/3 * 64 = 170.67 -> the next multiple of 256
    assert mlp.c_fc.weight.shape == mlp.c_up.weight.shape == (256, 64)
    assert mlp.c_proj.weight.shape == (64, 256)
    assert mlp.c_fc.bias is not None and mlp.c_up.bias is not None
    x = torch.randn(2, 5, 64)
    want = mlp.c_proj(F.silu(mlp.c_fc(x)) * mlp.c_up(x))
    assert torch.equal(mlp(x), want)
    wide = MLPBlock(GPTConfig(n_embd=4096, mlp="swiglu", bias=False))
    assert wide.c_fc.weight.shape == (11008, 4096) and wide.c_up.bias is None
    sized = MLPBlock(_gpt_cfg(mlp="swiglu", ffn_hidden=96))
    assert sized.c_up.weight.shape == (96, 64)


def test_gelu_config_is_unchanged():
    from easydist_amd.models.gpt import GPT

    torch.manual_seed(0)
    base = GPT(_gpt_cfg())
    torch.manual_seed(0)
    named = GPT(_gpt_cfg(mlp="gelu"))
    keys = list(base.state_dict())
    assert keys == list(named.state_dict())
    mlp_keys = [k for k in keys if k.startswith("h.0.mlp.")]
    assert mlp_keys == ["h.0.mlp.c_fc.weight", "h.0.mlp.c_fc.bias",
                        "h.0.mlp.c_proj.weight", "h.0.mlp.c_proj.bias"]
    assert base.h[0].mlp.c_fc.weight.shape == (256, 64)
    idx = torch.randint(0, 128, (2, 32))
    assert torch.equal(base(idx), named(idx))


def test_bad_mlp_string_raises():
    from easydist_amd.models.gpt import GPT

    with pytest.raises(ValueError, match="geglu"):
        GPT(_gpt_cfg(mlp="geglu"))


def test_gpt_tp_refuses_swiglu():
    from easydist_amd.models.gpt_tp import TPMLP

    with pytest.raises(ValueError, match="swiglu"):
        TPMLP(_gpt_cfg(mlp="swiglu"), 1, None)
