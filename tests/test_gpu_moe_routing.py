"""The gfx950 MoE routing kernels (csrc/moe_kernels.hip) against the aten
functions of ops/moe_ops.py on the CPU and the fp64 formula: exact inputs,
real values, the envelope, autograd and one compiled MoEGPT step."""
import functools
import pytest
import torch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]

# (N, K, E, C, factor, skewed)
CASES = [
    (1, 1, 1, 8, 1.0, False),         # one entry, cap 4, three empty slots
    (5, 2, 3, 72, 1.25, False),       # E not a power of two
    (67, 2, 8, 136, 1.0, False),      # crosses a wave
    (300, 3, 5, 8, 0.5, False),       # drops in every expert
    (1100, 2, 8, 264, 1.25, False),   # more than one 1024-entry chunk
    (600, 8, 256, 16, 2.0, False),    # the E and K limits
    (129, 2, 8, 72, 1.25, True),      # overflow next to empty experts
]
BF = torch.bfloat16
BIT_EQUAL = ("bins", "gates", "src", "valid", "gtopv", "gbins_out")


def _ops():
    import easydist_amd.ops as ops
    from easydist_amd.ops import moe_ops
    assert ops.require_hip_ops(), "HIP extension must be loaded on a GPU host"
    return torch.ops.easydist_amd, moe_ops


@functools.lru_cache(maxsize=None)
def _case(case, exact):
    """Inputs, the CPU functions' results and the fp64 formula; shared."""
    from easydist_amd.ops import moe_ops as mo
    N, K, E, C, factor, skewed = case
    g = torch.Generator().manual_seed(N + 7 * C + exact)
    cap = mo.capacity(N, E, K, factor)

    def rows(*shape):
        if exact:
            return torch.randint(-4, 5, shape, generator=g).to(BF)
        return torch.randn(shape, generator=g).to(BF)

    topi = torch.rand(N, E, generator=g).topk(K).indices
    if skewed:
        topi = torch.tensor([[2, 5]]).repeat(N, 1)
    if exact:
        topv = (0.5 * torch.randint(1, 3, (N, K), generator=g)).to(BF)
    else:
        topv = torch.softmax(torch.randn(N, K, generator=g), -1).to(BF)
    d = dict(tokens=rows(N, C), topi=topi, topv=topv, xbins=rows(E, cap, C),
             gbins=rows(E, cap, C), ggates=rows(E, cap), gout=rows(N, C))
    bins, gates, src, valid = mo._bins_impl(d["tokens"], topi, topv, E, factor)
    d.update(bins=bins, gates=gates, src=src, valid=valid)
    d["out"] = mo._combine_impl(d["xbins"], gates, src, valid, d["tokens"], K)
    d["gtokens"], d["gtopv"] = mo._bins_bwd_impl(
        d["gbins"], d["ggates"], src, valid, d["tokens"], K)
    d["gbins_out"], d["ggates_out"] = mo._combine_bwd_impl(
        d["gout"], d["xbins"], gates, src, valid, K)
    # the fp64 formula, and the sums of magnitudes its bounds scale with
    tok = (src // K).reshape(-1)
    vm = valid.double().unsqueeze(-1)

    def scatter(x):
        return torch.zeros(N, C, dtype=torch.double).index_add_(
            0, tok, (x * vm).reshape(-1, C))

    terms = d["xbins"].double() * gates.double().unsqueeze(-1)
    g_rows = d["gout"].double()[tok].reshape(E, cap, C)
    gb = g_rows * d["xbins"].double() * vm
    d["ref"] = dict(
        bins=d["tokens"].double()[tok].reshape(E, cap, C) * vm,
        out=scatter(terms), out_mag=scatter(terms.abs()),
        gtokens=scatter(d["gbins"].double()),
        gtokens_mag=scatter(d["gbins"].double().abs()),
        gbins_out=g_rows * gates.double().unsqueeze(-1) * vm,
        ggates_out=gb.sum(-1), ggates_mag=gb.abs().sum(-1))
    return d


def _run(ed, mo, case, d):
    """The four ops on the GPU, each inside its envelope."""
    N, K, E, C, factor, _ = case
    c = {k: v.cuda() for k, v in d.items() if isinstance(v, torch.Tensor)}
    assert mo._bins_kernel_ok(c["tokens"], c["topi"], c["topv"], E, factor)
    bins, gates, src, valid = ed.moe_bins(c["tokens"], c["topi"], c["topv"],
                                          E, factor)
    route = (gates, src, valid, c["tokens"], K)
    assert mo._combine_kernel_ok(c["xbins"], *route)
    assert mo._bins_bwd_kernel_ok(c["gbins"], c["ggates"], *route[1:])
    assert mo._combine_bwd_kernel_ok(c["gout"], c["xbins"], *route[:3], K)
    out = ed.moe_combine(c["xbins"], *route)
    gtokens, gtopv = ed.moe_bins_bwd(c["gbins"], c["ggates"], *route[1:])
    gbins_out, ggates_out = ed.moe_combine_bwd(c["gout"], c["xbins"],
                                               *route[:3], K)
    got = dict(bins=bins, gates=gates, src=src, valid=valid, out=out,
               gtokens=gtokens, gtopv=gtopv, gbins_out=gbins_out,
               ggates_out=ggates_out)
    return {k: v.cpu() for k, v in got.items()}


@pytest.mark.parametrize("case", [c for c in CASES if c[1] <= 3])
def test_exact(case):
    ed, mo = _ops()
    d = _case(case, True)
    for name in ("bins", "out", "gtokens", "gbins_out"):   # the premise
        assert torch.equal(d[name], d["ref"][name].to(BF)), name
    got = _run(ed, mo, case, d)
    for name in BIT_EQUAL + ("out", "gtokens"):
        assert torch.equal(got[name], d[name]), name


@pytest.mark.parametrize("case", CASES)
def test_real_values(case):
    """out, gtokens: 2^-8 |ref| + 2^-18 sum|terms| of the fp64 formula, one
    bf16 rounding and K <= 8 fp32 additions (2^-24 each) with room.  ggates:
    2^-8 |ref| + (C + K) 2^-24 sum|g b|, an fp32 sum in any order."""
    ed, mo = _ops()
    N, K, E, C, _, _ = case
    d = _case(case, False)
    got = _run(ed, mo, case, d)
    for name in BIT_EQUAL:
        assert torch.equal(got[name], d[name]), name
    ref = d["ref"]
    for name, mag in (("out", 2.0 ** -18 * ref["out_mag"]),
                      ("gtokens", 2.0 ** -18 * ref["gtokens_mag"]),
                      ("ggates_out", (C + K) * 2.0 ** -24 * ref["ggates_mag"])):
        err = (got[name].double() - ref[name]).abs()
        bound = 2.0 ** -8 * ref[name].abs() + mag
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"moe routing {case} {name}: worst err/bound {worst:.4f}")
        assert bool((err <= bound).all()), (name, worst)


def test_outside_the_envelope_runs_aten(monkeypatch):
    ed, mo = _ops()
    N, K, E, C, factor, _ = case = CASES[2]
    d = _case(case, False)
    c = {k: v.cuda() for k, v in d.items() if isinstance(v, torch.Tensor)}

    def check(tokens, xbins, gout, gbins, inside):
        bins_args = (tokens, c["topi"], c["topv"].to(tokens.dtype), E, factor)
        assert mo._bins_kernel_ok(*bins_args) == inside
        want = mo._bins_impl(*bins_args)
        got = ed.moe_bins(*bins_args)
        gates, src, valid = want[1:]
        route = (gates, src, valid, tokens, K)
        ggates = c["ggates"].to(tokens.dtype)
        assert mo._combine_kernel_ok(xbins, *route) == inside
        assert mo._bins_bwd_kernel_ok(gbins, ggates, *route[1:]) == inside
        assert mo._combine_bwd_kernel_ok(gout, xbins, *route[:3], K) == inside
        want += (mo._combine_impl(xbins, *route),)
        got += (ed.moe_combine(xbins, *route),)
        want += mo._bins_bwd_impl(gbins, ggates, *route[1:])
        got += ed.moe_bins_bwd(gbins, ggates, *route[1:])
        want += mo._combine_bwd_impl(gout, xbins, *route[:3], K)
        got += ed.moe_combine_bwd(gout, xbins, *route[:3], K)
        for x, y in zip(got, want):
            assert x.dtype == y.dtype and torch.equal(x, y)

    rows = (c["tokens"], c["xbins"], c["gout"], c["gbins"])
    check(*(t.float() for t in rows), inside=False)            # fp32
    check(*(t[..., :12].contiguous() for t in rows), inside=False)  # C = 12
    check(*(torch.cat([t] * 4, -1)[..., :520].contiguous() for t in rows),
          inside=False)                                        # C > 512
    args = [c[k] for k in ("xbins", "gates", "src", "valid", "tokens")]
    assert torch.equal(ed.moe_combine(*args, K), ed.moe_combine(*args, K))
    monkeypatch.setenv("EASYDIST_MOE_HIP", "0")   # inside, switched off
    check(*rows, inside=True)


def test_moe_layer_autograd(monkeypatch):
    """A bf16 MoELayer through the kernels against the aten path."""
    from easydist_amd.models.moe import MIXTRAL_SMALL, MoELayer
    _, mo = _ops()
    seen, real = [], mo._kernels    # what each op call dispatched to
    monkeypatch.setattr(mo, "_kernels",
                        lambda ok: seen.append(real(ok)) or seen[-1])
    torch.manual_seed(11)
    layer = MoELayer(MIXTRAL_SMALL).cuda().to(BF)
    x0 = torch.randn(4, 128, MIXTRAL_SMALL.n_embd, device="cuda").to(BF)
    gy = torch.randn_like(x0)

    def run():
        layer.zero_grad(True)
        x = x0.clone().requires_grad_(True)
        y = layer(x)
        y.backward(gy)
        return y.detach(), x.grad, layer.router.weight.grad.clone()

    got = run()
    assert len(seen) == 4 and all(ext is not None for ext in seen), seen
    monkeypatch.setenv("EASYDIST_MOE_HIP", "0")
    want = run()
    assert seen[4:] == [None] * 4, seen
    for name, a, b in zip(("out", "dx", "drouter"), got, want):
        ratio = float((a.float() - b.float()).abs().max()
                      / b.float().abs().max())
        print(f"moe layer {name}: max diff / max magnitude {ratio:.3e}")
        assert ratio <= 2.0 ** -6, (name, ratio)


def test_moe_gpt_end_to_end():
    """The routing ops stay in the compiled graph, and the loss is within
    5e-3 of eager, the suite's bound for compiled models.  Not a test of the
    kernels: autocast hands the ops fp32 tokens, so they run aten here."""
    import copy
    from easydist_amd import easydist_compile, easydist_setup, set_device_mesh
    from easydist_amd.models.moe import MIXTRAL_SMALL as cfg
    from easydist_amd.models.moe import MoEGPT, moe_train_step
    from easydist_amd.utils.testing import init_single_process
    ed, _ = _ops()
    torch.manual_seed(12)
    init_single_process()
    easydist_setup(backend="torch", device="cuda")
    set_device_mesh([0], ["spmd0"])
    model = MoEGPT(cfg).cuda()
    model_ref = copy.deepcopy(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=True)
    opt_ref = torch.optim.Adam(model_ref.parameters(), lr=1e-4, fused=True)
    compiled = easydist_compile(moe_train_step, cuda_graph=False)
    idx = torch.randint(0, cfg.vocab_size, (4, cfg.block_size), device="cuda")
    loss = float(compiled(model, opt, idx, idx).detach())
    ref = float(moe_train_step(model_ref, opt_ref, idx, idx).detach())
    print(f"moe routing gpt: compiled {loss:.6f} eager {ref:.6f}")
    assert loss == loss and abs(loss - ref) < 5e-3, (loss, ref)
    gm = list(compiled.compiled.values())[0].gm
    targets = [n.target for n in gm.graph.nodes if n.op == "call_function"]
    assert targets.count(ed.moe_bins.default) == cfg.n_layer
    assert targets.count(ed.moe_combine.default) == cfg.n_layer
