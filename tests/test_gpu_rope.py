"""The gfx950 RoPE kernel (csrc/rope_kernels.hip) against the aten formula.

* exact: integer inputs and tables from {0, +-1, +-0.5} make every product
  and sum exactly representable, so the kernel must be torch.equal to the
  aten formula, forward and inverse: a wrong row, head, half or table index
  shows with no tolerance at all;
* real tables and randn inputs against the fp64 formula, every element
  inside one bf16 rounding plus the fp32 roundings of the formula;
* strided inputs, the aten path outside the envelope, autograd, and a
  rope=True GPT compiled end to end.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

# (B, S, H, Hkv, D)
SHAPES = [
    (1, 1, 1, 1, 64),       # a single row
    (2, 5, 4, 2, 64),       # GQA, odd row count
    (1, 130, 3, 1, 128),    # three q heads on one K/V head, D = 128
    (2, 7, 2, 2, 48),       # three vectors per half
    (1, 5000, 2, 1, 64),    # more rows than one pass of a small grid
    (1, 3, 1, 1, 256),      # the D cap
]


def _ops():
    import easydist_amd.ops as ops
    from easydist_amd.ops import rope
    assert ops.require_hip_ops(), "HIP extension must be loaded on a GPU host"
    return torch.ops.easydist_amd.rope_qkv, rope


def _exact_inputs(B, S, H, Hkv, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    W = (H + 2 * Hkv) * D
    qkv = torch.randint(-8, 9, (B, S, W), generator=g).to(torch.bfloat16)
    vals = torch.tensor([0.0, 1.0, -1.0, 0.5, -0.5])
    cos = vals[torch.randint(0, 5, (S, D // 2), generator=g)]
    sin = vals[torch.randint(0, 5, (S, D // 2), generator=g)]
    return qkv, cos, sin


@requires_gpu
@pytest.mark.parametrize("B,S,H,Hkv,D", SHAPES)
def test_exact(B, S, H, Hkv, D):
    op, rope = _ops()
    qkv, cos, sin = _exact_inputs(B, S, H, Hkv, D)
    assert rope._kernel_ok(qkv.cuda(), cos.cuda(), sin.cuda())
    for inverse in (False, True):
        want = rope._math(qkv, cos, sin, H, Hkv, inverse)
        # the premise: the fp32 formula is exact here
        want64 = rope._math(qkv.double(), cos.double(), sin.double(), H, Hkv,
                            inverse)
        assert torch.equal(want.double(), want64)
        got = op(qkv.cuda(), cos.cuda(), sin.cuda(), H, Hkv, inverse)
        assert got.dtype == torch.bfloat16 and got.is_contiguous()
        assert torch.equal(got.cpu(), want), (inverse, int(
            (got.cpu() != want).sum()))


@requires_gpu
def test_exact_grid_stride(monkeypatch):
    """Three blocks for 313 passes: every block loops, the tail included."""
    op, rope = _ops()
    B, S, H, Hkv, D = 1, 5000, 2, 1, 64
    qkv, cos, sin = _exact_inputs(B, S, H, Hkv, D, seed=1)
    want = rope._math(qkv, cos, sin, H, Hkv, False)
    monkeypatch.setenv("EASYDIST_ROPE_BLOCKS", "3")
    got = op(qkv.cuda(), cos.cuda(), sin.cuda(), H, Hkv, False)
    assert torch.equal(got.cpu(), want)


@requires_gpu
@pytest.mark.parametrize("B,S,H,Hkv,D", SHAPES)
def test_real_tables(B, S, H, Hkv, D):
    """|out - ref| <= 2^-8 |ref| + 2^-18 (|lo| + |hi|) against the fp64
    formula on the same inputs: one rounding to bf16 is the first term; the
    three fp32 roundings of the formula are at most 3 * 2^-24 (|lo| + |hi|),
    which the second covers with room for fused multiply-add."""
    op, rope = _ops()
    torch.manual_seed(B * 1000 + S)
    W = (H + 2 * Hkv) * D
    R = (H + Hkv) * D
    qkv = torch.randn(B, S, W).to(torch.bfloat16)
    cos, sin = rope.rope_tables(S, D)
    x = qkv[..., :R].double().view(B, S, H + Hkv, D)
    mag = x[..., :D // 2].abs() + x[..., D // 2:].abs()
    mag = torch.cat((mag, mag), dim=-1).view(B, S, R)
    for inverse in (False, True):
        ref = rope._math(qkv.double(), cos.double(), sin.double(), H, Hkv,
                         inverse)
        got = op(qkv.cuda(), cos.cuda(), sin.cuda(), H, Hkv, inverse).cpu()
        err = (got.double() - ref)[..., :R].abs()
        bound = 2.0 ** -8 * ref[..., :R].abs() + 2.0 ** -18 * mag
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"rope real tables {(B, S, H, Hkv, D)} inverse={inverse}: "
              f"worst err/bound {worst:.4f}")
        assert bool((err <= bound).all()), worst
        assert torch.equal(got[..., R:], qkv[..., R:])


@requires_gpu
def test_strided_inputs():
    op, rope = _ops()
    B, S, H, Hkv, D = 2, 5, 4, 2, 64
    W = (H + 2 * Hkv) * D
    torch.manual_seed(2)
    qkv = torch.randn(B, S, W).to(torch.bfloat16).cuda()
    cos, sin = rope.rope_tables(S, D, device="cuda")
    want = op(qkv, cos, sin, H, Hkv, False)
    # a column slice of a wider buffer: row stride W + 64
    big = torch.randn(B, S, W + 64, device="cuda").to(torch.bfloat16)
    big[:, :, :W] = qkv
    view = big[:, :, :W]
    assert not view.is_contiguous() and rope._kernel_ok(view, cos, sin)
    got = op(view, cos, sin, H, Hkv, False)
    assert got.is_contiguous() and torch.equal(got, want)
    # every other batch entry
    big2 = torch.randn(2 * B, S, W, device="cuda").to(torch.bfloat16)
    big2[::2] = qkv
    view2 = big2[::2]
    assert not view2.is_contiguous() and rope._kernel_ok(view2, cos, sin)
    got2 = op(view2, cos, sin, H, Hkv, False)
    assert got2.is_contiguous() and torch.equal(got2, want)


@requires_gpu
def test_outside_the_envelope_runs_aten():
    op, rope = _ops()
    torch.manual_seed(3)
    # fp32 input, and a head dim that is no multiple of 16, in both dtypes
    for B, S, H, Hkv, D, dtype in ((2, 5, 4, 2, 64, torch.float32),
                                   (2, 5, 2, 1, 40, torch.float32),
                                   (2, 5, 2, 1, 40, torch.bfloat16)):
        qkv = torch.randn(B, S, (H + 2 * Hkv) * D).to(dtype)
        cos, sin = rope.rope_tables(S, D)
        assert not rope._kernel_ok(qkv.cuda(), cos.cuda(), sin.cuda())
        want = op(qkv, cos, sin, H, Hkv, False)
        got = op(qkv.cuda(), cos.cuda(), sin.cuda(), H, Hkv, False)
        assert got.dtype == dtype and got.is_contiguous()
        if dtype == torch.float32:
            assert torch.allclose(got.cpu(), want, rtol=1e-6, atol=1e-6)
        else:
            # the same fp32 formula on both sides: one bf16 ulp at the most
            assert torch.allclose(got.cpu().float(), want.float(),
                                  rtol=2.0 ** -7, atol=1e-6)


@requires_gpu
def test_autograd_is_the_inverse_kernel():
    op, rope = _ops()
    B, S, H, Hkv, D = 2, 5, 4, 2, 64
    torch.manual_seed(4)
    x = torch.randn(B, S, (H + 2 * Hkv) * D).to(torch.bfloat16).cuda() \
        .requires_grad_(True)
    g = torch.randn(B, S, (H + 2 * Hkv) * D).to(torch.bfloat16).cuda()
    cos, sin = rope.rope_tables(S, D, device="cuda")
    (dx,) = torch.autograd.grad(
        (rope.apply_rope(x, cos, sin, H, Hkv) * g).sum(), x)
    assert torch.equal(dx, op(g, cos, sin, H, Hkv, True))


@requires_gpu
def test_rope_gpt_end_to_end():
    """A rope=True GPT through the compiler on cuda:0, under the benchmarked
    bf16-autocast train step so that the rotations run as the HIP kernel."""
    from easydist_amd import easydist_compile, easydist_setup, set_device_mesh
    from easydist_amd.models.gpt import GPT, GPTConfig, gpt_train_step
    from easydist_amd.utils.testing import init_single_process

    op, _ = _ops()
    init_single_process()
    easydist_setup(backend="torch", device="cuda")
    set_device_mesh([0], ["spmd0"])
    torch.manual_seed(8)
    cfg = GPTConfig(vocab_size=512, n_layer=2, n_head=4, n_kv_head=2,
                    n_embd=256, block_size=128, rope=True)
    model = GPT(cfg).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=True)
    compiled = easydist_compile(gpt_train_step, cuda_graph=False)
    idx = torch.randint(0, 512, (4, 128), device="cuda")
    tg = torch.randint(0, 512, (4, 128), device="cuda")
    loss1 = float(compiled(model, opt, idx, tg))
    loss2 = float(compiled(model, opt, idx, tg))
    assert loss1 == loss1 and loss2 == loss2 and abs(loss1) < 1e4 \
        and abs(loss2) < 1e4, (loss1, loss2)
    assert loss2 <= loss1 + 1.0, (loss1, loss2)

    gm = list(compiled.compiled.values())[0].gm
    nodes = [n for n in gm.graph.nodes if n.op == "call_function"]
    names = [getattr(n.target, "__name__", "") for n in nodes]
    ropes = [n for n in nodes if n.target is op.default]
    assert sorted(bool(n.args[5]) for n in ropes) \
        == [False, False, True, True]
    for n in ropes:
        # bf16 activations, fp32 tables: autocast leaves the tables alone
        assert n.args[0].meta["val"].dtype == torch.bfloat16
        assert n.args[1].meta["val"].dtype == torch.float32
        assert n.args[2].meta["val"].dtype == torch.float32
    assert names.count("flash_attention_bwd_pack.default") == 2
    assert names.count("flash_attention_bwd.default") == 0
