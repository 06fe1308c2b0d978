"""The gfx950 SwiGLU kernels (csrc/swiglu_kernels.hip) against the aten path.

* exact: gates from {32, 64, -128, 0} have the sigmoids 1, 1, 0 and 0.5
  exactly in fp32, and with small integer `up` and power-of-two `grad` every
  product fits bf16, so the kernels must be torch.equal to the aten formula:
  a wrong row, column, stride or operand shows with no tolerance at all;
* randn inputs against the fp64 formula, every element inside one bf16
  rounding plus the fp32 roundings and the fast exponential's error;
* strided inputs, a short grid, an overflowing gate, the aten path outside
  the envelope, autograd, and the mlp="swiglu" GPT and the MoE model
  compiled end to end.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

# (leading dims..., F)
SHAPES = [
    (1, 8),          # one vector
    (3, 8),
    (5, 72),         # nine vectors per row
    (2, 3, 136),     # 3-D
    (313, 1024),     # more than one block
]


def _ops():
    import easydist_amd.ops as ops
    from easydist_amd.ops import swiglu
    assert ops.require_hip_ops(), "HIP extension must be loaded on a GPU host"
    return torch.ops.easydist_amd, swiglu


def _exact_inputs(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    gates = torch.tensor([32.0, 64.0, -128.0, 0.0])
    grads = torch.tensor([1.0, -1.0, 2.0, -2.0, 4.0, -4.0])
    gate = gates[torch.randint(0, 4, shape, generator=g)]
    up = torch.randint(-8, 9, shape, generator=g).float()
    grad = grads[torch.randint(0, 6, shape, generator=g)]
    return tuple(t.to(torch.bfloat16) for t in (gate, up, grad))


def _formula64(gate, up, grad):
    g, u, dy = gate.double(), up.double(), grad.double()
    s = 1.0 / (1.0 + torch.exp(-g))
    return g * s * u, dy * u * s * (1.0 + g * (1.0 - s)), dy * g * s


def _exact_wants(sw, gate, up, grad):
    """The aten path's results, after asserting the premise: the fp32
    formula and the fp64 formula agree once rounded to bf16 (in fp64 the
    sigmoid of 32 is 1 - 1.3e-14, not 1: that rounds away)."""
    out = sw._math(gate, up)
    dgate, dup = sw._math_bwd(grad, gate, up)
    for got, want64 in zip((out, dgate, dup), _formula64(gate, up, grad)):
        assert torch.equal(got, want64.to(torch.bfloat16))
    if out.numel() >= 37 * 72:
        # not degenerate: many distinct values in every output
        assert len(out.unique()) >= 20 and len(dgate.unique()) >= 20 \
            and len(dup.unique()) >= 9
    return out, dgate, dup


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_exact(shape):
    ed, sw = _ops()
    gate, up, grad = _exact_inputs(shape)
    out, dgate, dup = _exact_wants(sw, gate, up, grad)
    cg, cu, cd = gate.cuda(), up.cuda(), grad.cuda()
    assert sw._kernel_ok(cg, cu) and sw._kernel_ok(cd, cg, cu)
    got = ed.swiglu(cg, cu)
    got_dgate, got_dup = ed.swiglu_bwd(cd, cg, cu)
    for name, x, want in (("out", got, out), ("dgate", got_dgate, dgate),
                          ("dup", got_dup, dup)):
        assert x.dtype == torch.bfloat16 and x.is_contiguous()
        assert x.shape == want.shape
        assert torch.equal(x.cpu(), want), (name, int((x.cpu() != want).sum()))


@requires_gpu
def test_exact_grid_stride(monkeypatch):
    """Three blocks for 157 passes: every block loops, the tail included."""
    ed, sw = _ops()
    gate, up, grad = _exact_inputs((313, 1024), seed=1)
    out, dgate, dup = _exact_wants(sw, gate, up, grad)
    monkeypatch.setenv("EASYDIST_SWIGLU_BLOCKS", "3")
    got = ed.swiglu(gate.cuda(), up.cuda())
    got_dgate, got_dup = ed.swiglu_bwd(grad.cuda(), gate.cuda(), up.cuda())
    assert torch.equal(got.cpu(), out)
    assert torch.equal(got_dgate.cpu(), dgate)
    assert torch.equal(got_dup.cpu(), dup)


@requires_gpu
def test_strided_inputs():
    ed, sw = _ops()
    R, Fd = 37, 72
    gate, up, grad = _exact_inputs((R, Fd), seed=2)
    out, dgate, dup = _exact_wants(sw, gate, up, grad)

    def check(cg, cu, cd):
        assert sw._kernel_ok(cg, cu) and sw._kernel_ok(cd, cg, cu)
        got = ed.swiglu(cg, cu)
        got_dgate, got_dup = ed.swiglu_bwd(cd, cg, cu)
        for x, want in ((got, out), (got_dgate, dgate), (got_dup, dup)):
            assert x.is_contiguous() and torch.equal(x.cpu(), want)

    # the two halves of one [R, 2F] projection output
    h = torch.cat((gate, up), dim=-1).cuda()
    cg, cu = h.chunk(2, -1)
    assert not cg.is_contiguous() and not cu.is_contiguous()
    check(cg, cu, grad.cuda())
    # every other row of a taller buffer, the up half at an odd row offset
    tall = torch.full((2 * R, 2 * Fd), 7.0, dtype=torch.bfloat16,
                      device="cuda")
    tall[1::2] = h
    cg, cu = tall[1::2].chunk(2, -1)
    assert cg.stride(0) == 4 * Fd
    check(cg, cu, grad.cuda())
    # grad as a column slice of a wider buffer
    wide = torch.full((R, Fd + 24), 7.0, dtype=torch.bfloat16, device="cuda")
    wide[:, 16:16 + Fd] = grad.cuda()
    cd = wide[:, 16:16 + Fd]
    assert not cd.is_contiguous() and cd.storage_offset() == 16
    check(gate.cuda(), up.cuda(), cd)
    # 3-D operands whose two leading dims collapse to one row stride
    h3 = torch.cat((gate, up), dim=-1)[:36].reshape(4, 9, 2 * Fd).cuda()
    cg, cu = h3.chunk(2, -1)
    assert sw._kernel_ok(cg, cu)
    got = ed.swiglu(cg, cu)
    assert got.shape == (4, 9, Fd)
    assert torch.equal(got.cpu().reshape(36, Fd), out[:36])


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_real_values(shape):
    """Against the fp64 formula on the same bf16 inputs, elementwise:

        |out   - ref| <= 2^-8 |ref| + 2^-18 |g u|
        |dup   - ref| <= 2^-8 |ref| + 2^-18 |dy g|
        |dgate - ref| <= 2^-8 |ref| + 2^-18 |dy u| (1 + |g|)

    The first term is the one rounding to bf16.  The second covers the fp32
    roundings of the formula (each 2^-24) and the error of the fast
    exponential and the hardware reciprocal, a few fp32 ulp, with about 16x
    room; it scales with the operand magnitudes, not with the result,
    because 1 + g (1 - s) cancels near g = -1.28.
    """
    ed, sw = _ops()
    torch.manual_seed(sum(shape))
    gate = (4 * torch.randn(shape)).to(torch.bfloat16)
    up = torch.randn(shape).to(torch.bfloat16)
    grad = torch.randn(shape).to(torch.bfloat16)
    ref_out, ref_dgate, ref_dup = _formula64(gate, up, grad)
    g, u, dy = gate.double().abs(), up.double().abs(), grad.double().abs()
    out = ed.swiglu(gate.cuda(), up.cuda()).cpu()
    dgate, dup = (t.cpu() for t in
                  ed.swiglu_bwd(grad.cuda(), gate.cuda(), up.cuda()))
    for name, got, ref, mag in (("out", out, ref_out, g * u),
                                ("dup", dup, ref_dup, dy * g),
                                ("dgate", dgate, ref_dgate,
                                 dy * u * (1 + g))):
        err = (got.double() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 2.0 ** -18 * mag
        worst = float((err / bound.clamp_min(1e-300)).max())
        # what the fp32 arithmetic alone adds, in units of the second term
        excess = float(((err - 2.0 ** -8 * ref.abs()).clamp_min(0)
                        / (2.0 ** -18 * mag).clamp_min(1e-300)).max())
        print(f"swiglu real values {shape} {name}: worst err/bound "
              f"{worst:.4f}, over one rounding {excess:.4f} of 2^-18 mag")
        assert bool((err <= bound).all()), (name, worst)


@requires_gpu
def test_overflowing_gate():
    """exp(200) is inf in fp32: s = 1/inf = 0, outputs finite and zero."""
    ed, sw = _ops()
    torch.manual_seed(5)
    gate = torch.full((3, 16), -200.0, dtype=torch.bfloat16, device="cuda")
    up = torch.randn(3, 16, device="cuda").to(torch.bfloat16)
    grad = torch.randn(3, 16, device="cuda").to(torch.bfloat16)
    assert sw._kernel_ok(grad, gate, up)
    for t in (ed.swiglu(gate, up),) + tuple(ed.swiglu_bwd(grad, gate, up)):
        assert bool(torch.isfinite(t).all()) and not bool(t.any())


@requires_gpu
def test_outside_the_envelope_runs_aten():
    ed, sw = _ops()
    torch.manual_seed(3)
    bf = torch.bfloat16
    wide = torch.randn(3, 6, 32).to(bf)

    def cases():
        yield "F = 12", tuple(torch.randn(5, 12).to(bf) for _ in range(3))
        yield "fp32", tuple(torch.randn(5, 16) for _ in range(3))
        yield "misaligned slice", tuple(wide[i][:, 1:9] for i in range(3))
        yield "transposed", tuple(wide[i].t() for i in range(3))
        yield "empty", tuple(torch.randn(0, 16).to(bf) for _ in range(3))

    for name, (gate, up, grad) in cases():
        cg, cu, cd = gate.cuda(), up.cuda(), grad.cuda()
        if name == "misaligned slice":      # .cuda() would compact a view
            cw = wide.cuda()
            cg, cu, cd = (cw[i][:, 1:9] for i in range(3))
        elif name == "transposed":
            cw = wide.cuda()
            cg, cu, cd = (cw[i].t() for i in range(3))
        assert not sw._kernel_ok(cg, cu), name
        assert not sw._kernel_ok(cd, cg, cu), name
        got = ed.swiglu(cg, cu)
        got_dgate, got_dup = ed.swiglu_bwd(cd, cg, cu)
        want = sw._math(cg, cu)
        want_dgate, want_dup = sw._math_bwd(cd, cg, cu)
        for x, y in ((got, want), (got_dgate, want_dgate),
                     (got_dup, want_dup)):
            assert x.dtype == gate.dtype and x.shape == gate.shape, name
            assert x.is_contiguous() and torch.equal(x, y), name


@requires_gpu
def test_autograd_runs_the_backward_kernel():
    ed, sw = _ops()
    gate, up, grad = _exact_inputs((37, 72), seed=4)
    _, dgate, dup = _exact_wants(sw, gate, up, grad)
    cg = gate.cuda().requires_grad_(True)
    cu = up.cuda().requires_grad_(True)
    sw.swiglu(cg, cu).backward(grad.cuda())
    assert torch.equal(cg.grad.cpu(), dgate)
    assert torch.equal(cu.grad.cpu(), dup)


def _compile_one_step(model, step_fn, vocab, batch, seq):
    """The first compiled step's loss, eager's under the same autocast on a
    copy of the model, and the compiled graph's call_function names."""
    import copy

    from easydist_amd import easydist_compile, easydist_setup, set_device_mesh
    from easydist_amd.utils.testing import init_single_process

    init_single_process()
    easydist_setup(backend="torch", device="cuda")
    set_device_mesh([0], ["spmd0"])
    model_ref = copy.deepcopy(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=True)
    opt_ref = torch.optim.Adam(model_ref.parameters(), lr=1e-4, fused=True)
    compiled = easydist_compile(step_fn, cuda_graph=False)
    idx = torch.randint(0, vocab, (batch, seq), device="cuda")
    tg = torch.randint(0, vocab, (batch, seq), device="cuda")
    loss = float(compiled(model, opt, idx, tg).detach())
    ref = float(step_fn(model_ref, opt_ref, idx, tg).detach())
    gm = list(compiled.compiled.values())[0].gm
    nodes = [n for n in gm.graph.nodes if n.op == "call_function"]
    return loss, ref, nodes


def _check_graph(ed, nodes, n_layer):
    names = [getattr(n.target, "__name__", "") for n in nodes]
    fwd = [n for n in nodes if n.target is ed.swiglu.default]
    bwd = [n for n in nodes if n.target is ed.swiglu_bwd.default]
    assert len(fwd) == n_layer and len(bwd) == n_layer, names
    assert "silu.default" not in names
    assert "silu_backward.default" not in names
    for n in fwd + bwd:
        # bf16 activations: the kernels' dtype
        for arg in n.args:
            assert arg.meta["val"].dtype == torch.bfloat16


@requires_gpu
def test_swiglu_gpt_end_to_end():
    """The mlp="swiglu" GPT through the compiler on cuda:0 under the
    benchmarked bf16-autocast train step.  The checks of the compiled rope
    GPT (finite, bounded loss), and the loss against eager within 5e-3,
    the bound of the suite's compiled-GPT comparisons on the GPU."""
    from easydist_amd.models.gpt import GPT, GPTConfig, gpt_train_step

    ed, _ = _ops()
    torch.manual_seed(8)
    cfg = GPTConfig(vocab_size=512, n_layer=2, n_head=1, n_embd=64,
                    block_size=128, mlp="swiglu")
    model = GPT(cfg).cuda()
    loss, ref, nodes = _compile_one_step(model, gpt_train_step, 512, 4, 128)
    print(f"swiglu gpt: compiled {loss:.6f} eager {ref:.6f}")
    assert loss == loss and abs(loss) < 1e4, loss
    _check_graph(ed, nodes, cfg.n_layer)
    assert abs(loss - ref) < 5e-3, (loss, ref)


@requires_gpu
def test_moe_end_to_end():
    """MIXTRAL_SMALL through the compiler on cuda:0 in bf16 autocast: the
    experts' silu(a) * b and its backward run as the fused kernels.  Loss
    against eager under the same autocast within 5e-3, as for the GPT."""
    from easydist_amd.models.moe import MIXTRAL_SMALL, MoEGPT, moe_train_step

    ed, _ = _ops()
    torch.manual_seed(9)
    cfg = MIXTRAL_SMALL
    model = MoEGPT(cfg).cuda()
    loss, ref, nodes = _compile_one_step(model, moe_train_step,
                                         cfg.vocab_size, 4, cfg.block_size)
    print(f"swiglu moe: compiled {loss:.6f} eager {ref:.6f}")
    assert loss == loss and abs(loss) < 1e4, loss
    _check_graph(ed, nodes, cfg.n_layer)
    assert abs(loss - ref) < 5e-3, (loss, ref)
