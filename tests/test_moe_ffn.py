"""The MoE expert FFN ops (ops/moe_ffn.py) off the GPU: the aten contract
against the fp64 formula, the op registrations, the model option and the
compiler's preset rules (through one compiled step)."""
import copy
import dataclasses

import pytest
import torch
import torch.nn.functional as F

import easydist_amd.ops  # noqa: F401  (registers the ops)
from easydist_amd.models.moe import MIXTRAL_SMALL, ExpertFFN, MoEGPT

ed = torch.ops.easydist_amd
E, R, K, N = 3, 10, 32, 16


def _inputs(dtype):
    g = torch.Generator().manual_seed(1)
    x, w1, w3 = (torch.randn(s, generator=g).to(dtype)
                 for s in ((E, R, K), (E, K, N), (E, K, N)))
    valid = torch.arange(R).expand(E, R) < torch.tensor([[0], [R], [R // 2]])
    return x * valid.unsqueeze(-1), w1 * K ** -0.5, w3 * K ** -0.5, valid


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_aten_path_against_fp64(dtype):
    """|out - ref| <= u |ref| + K u32 mag, u = one rounding to the output
    dtype with twice the half-ulp (2^-8 bf16, 2^-23 fp32), u32 = 2^-23 the
    fp32 accumulation in any order; h as in tests/test_gpu_moe_ffn.py."""
    x, w1, w3, valid = _inputs(dtype)
    h, a, b = ed.moe_expert_up(x, w1, w3, valid)
    c = ed.moe_expert_gemm(x, w1, None)
    assert all(t.dtype == dtype and t.shape == (E, R, N) for t in (h, a, b, c))
    xd, w1d, w3d = x.double(), w1.double(), w3.double()
    ra, rb = torch.bmm(xd, w1d), torch.bmm(xd, w3d)
    ma, mb = torch.bmm(xd.abs(), w1d.abs()), torch.bmm(xd.abs(), w3d.abs())
    u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -23
    acc = K * 2.0 ** -23
    for got, ref, mag in ((a, ra, ma), (b, rb, mb), (c, ra, ma),
                          (h, F.silu(ra) * rb,
                           1.1 * rb.abs() * ma + F.silu(ra).abs() * mb)):
        err = (got.double() - ref).abs()
        assert bool((err <= u * ref.abs() + acc * mag).all())
    assert not h[0].any() and not c[0].any()      # zero rows stay zero


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_opcheck(dtype):
    x, w1, w3, valid = (t.requires_grad_(t.is_floating_point())
                        for t in _inputs(dtype))
    torch.library.opcheck(ed.moe_expert_up.default, (x, w1, w3, valid))
    torch.library.opcheck(ed.moe_expert_up.default, (x, w1, w3, None))
    torch.library.opcheck(ed.moe_expert_gemm.default, (x, w1, valid))


@pytest.mark.parametrize("with_h", [True, False])
def test_up_backward_through_a_and_b(with_h):
    """Gradients arriving through a and b, with and without one through h,
    against autograd of the plain formula in fp32."""
    leaves = [t.requires_grad_(True) for t in _inputs(torch.float32)[:3]]
    g = torch.Generator().manual_seed(3)
    ch, ca, cb = (torch.randn(E, R, N, generator=g) for _ in range(3))

    def loss(h, a, b):
        return (h * ch).sum() * with_h + (a * ca).sum() + (b * cb).sum()

    out = ed.moe_expert_up(*leaves, None)
    got = torch.autograd.grad(loss(*out) if with_h else loss(0, *out[1:]),
                              leaves)
    a, b = torch.bmm(leaves[0], leaves[1]), torch.bmm(leaves[0], leaves[2])
    want = torch.autograd.grad(loss(F.silu(a) * b, a, b), leaves)
    for p, q in zip(got, want):
        torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-6)


def test_expert_ffn_grouped_equals_default_fp32():
    torch.manual_seed(2)
    plain = ExpertFFN(E, K, N)
    grouped = ExpertFFN(E, K, N, grouped=True)
    grouped.load_state_dict(plain.state_dict())
    x, _, _, valid = _inputs(torch.float32)
    xs = [x.clone().requires_grad_(True) for _ in range(2)]
    outs = [plain(xs[0]), grouped(xs[1], valid)]
    assert torch.equal(*outs)          # fp32: literally bmm and silu * mul
    gy = torch.randn_like(outs[0])
    for out in outs:
        out.backward(gy)
    for p, q in zip((xs[0], *plain.parameters()),
                    (xs[1], *grouped.parameters())):
        torch.testing.assert_close(q.grad, p.grad, rtol=1e-5, atol=1e-6)


def test_moe_gpt_grouped_compiles_ws1():
    """MoEGPT with grouped_experts through the compile entry of
    tests/test_moe.py at ws1: the preset rules are exercised, the ops stay
    in the graph, the loss is finite and within that test's 5e-3 of eager."""
    from easydist_amd import easydist_compile, easydist_setup, set_device_mesh
    from easydist_amd.utils.testing import init_single_process

    dev = "cuda" if torch.cuda.is_available() else "cpu"   # the compiler's
    init_single_process()
    easydist_setup(backend="torch", device=dev)
    set_device_mesh([0], ["spmd0"])
    torch.manual_seed(0)
    cfg = dataclasses.replace(MIXTRAL_SMALL, n_layer=1, grouped_experts=True)
    model = MoEGPT(cfg).to(dev)
    model_ref = copy.deepcopy(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    opt_ref = torch.optim.Adam(model_ref.parameters(), lr=1e-3, fused=True)

    def step(model, opt, idx, tg):
        loss = model.loss(idx, tg)
        loss.backward()
        opt.step()
        opt.zero_grad(True)
        return loss

    compiled = easydist_compile(step, cuda_graph=False)
    idx = torch.randint(0, cfg.vocab_size, (4, cfg.block_size), device=dev)
    loss = float(compiled(model, opt, idx, idx).detach())
    ref = float(step(model_ref, opt_ref, idx, idx).detach())
    assert loss == loss and abs(loss - ref) < 5e-3, (loss, ref)
    gm = list(compiled.compiled.values())[0].gm
    targets = [n.target for n in gm.graph.nodes if n.op == "call_function"]
    assert targets.count(ed.moe_expert_up.default) == cfg.n_layer
    assert targets.count(ed.moe_expert_gemm.default) == cfg.n_layer
