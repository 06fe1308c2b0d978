"""The MoE expert FFN backward ops (ops/moe_ffn.py) off the GPU: opcheck,
the aten contract against fp64, and the ops in one compiled training step."""
import dataclasses

import pytest
import torch

import easydist_amd.ops  # noqa: F401  (registers the ops)
from easydist_amd.models.moe import MIXTRAL_SMALL, MoEGPT

ed = torch.ops.easydist_amd
E, R, K, N = 3, 10, 16, 32


def _inputs(dtype):
    gen = torch.Generator().manual_seed(1)
    valid = torch.arange(R).expand(E, R) < torch.tensor([[0], [R], [R // 2]])
    x, g1, g2 = (torch.randn(s, generator=gen).to(dtype) * valid.unsqueeze(-1)
                 for s in ((E, R, K), (E, R, N), (E, R, N)))
    w1, w2 = (torch.randn(E, K, N, generator=gen).to(dtype) * N ** -0.5
              for _ in range(2))
    return x, g1, g2, w1, w2, valid


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_opcheck(dtype):
    x, g1, g2, w1, w2, valid = _inputs(dtype)
    for v in (valid, None):
        for op, args in ((ed.moe_expert_dx, (g1, w1, g2, w2, v)),
                         (ed.moe_expert_dx, (g1, w1, None, None, v)),
                         (ed.moe_expert_dw, (x, g1, v)),
                         (ed.moe_expert_dw2, (x, g1, g2, v))):
            torch.library.opcheck(op.default, args)


def test_aten_bf16_path_against_fp64():
    """|out - ref| <= 2^-8 |ref| + n 2^-23 mag: one rounding to bf16 and the
    fp32 accumulation over n terms, mag the product of absolute values."""
    x, g1, g2, w1, w2, valid = _inputs(torch.bfloat16)
    xd, g1d, g2d, w1t, w2t = (t.double() for t in (
        x.transpose(1, 2), g1, g2, w1.transpose(1, 2), w2.transpose(1, 2)))
    dw1, dw3 = ed.moe_expert_dw2(x, g1, g2, valid)
    for got, n, pairs in (
            (ed.moe_expert_dx(g1, w1, None, None, valid), N, [(g1d, w1t)]),
            (ed.moe_expert_dx(g1, w1, g2, w2, valid), 2 * N,
             [(g1d, w1t), (g2d, w2t)]),
            (ed.moe_expert_dw(x, g2, None), R, [(xd, g2d)]),
            (dw1, R, [(xd, g1d)]), (dw3, R, [(xd, g2d)])):
        ref = sum(torch.bmm(p, q) for p, q in pairs)
        mag = sum(torch.bmm(p.abs(), q.abs()) for p, q in pairs)
        assert got.dtype == torch.bfloat16 and got.shape == ref.shape
        err = (got.double() - ref).abs()
        assert bool((err <= 2.0 ** -8 * ref.abs() + n * 2.0 ** -23 * mag).all())
        assert not got[0].any()           # the expert without a valid row


def test_moe_gpt_grouped_backward_ops_in_the_compiled_step():
    """The compile entry of tests/test_moe_ffn.py at ws1: per layer the step
    holds the up projection's two-product dx and pair dw, the down
    projection's dx and dw, and no baddbmm."""
    from easydist_amd import easydist_compile, easydist_setup, set_device_mesh
    from easydist_amd.utils.testing import init_single_process
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    init_single_process()
    easydist_setup(backend="torch", device=dev)
    set_device_mesh([0], ["spmd0"])
    cfg = dataclasses.replace(MIXTRAL_SMALL, n_layer=1, grouped_experts=True)
    model = MoEGPT(cfg).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)

    def step(model, opt, idx, tg):
        loss = model.loss(idx, tg)
        loss.backward()
        opt.step()
        opt.zero_grad(True)
        return loss

    compiled = easydist_compile(step, cuda_graph=False)
    idx = torch.randint(0, cfg.vocab_size, (4, cfg.block_size), device=dev)
    assert bool(torch.isfinite(compiled(model, opt, idx, idx)))
    gm = list(compiled.compiled.values())[0].gm
    targets = [n.target for n in gm.graph.nodes if n.op == "call_function"]
    assert targets.count(ed.moe_expert_dx.default) == 2 * cfg.n_layer
    assert targets.count(ed.moe_expert_dw2.default) == cfg.n_layer
    assert targets.count(ed.moe_expert_dw.default) == cfg.n_layer
    assert targets.count(torch.ops.aten.baddbmm.default) == 0
