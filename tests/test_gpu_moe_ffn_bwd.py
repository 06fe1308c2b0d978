"""The gfx950 MoE expert FFN backward kernels (moe_nt, moe_tn) against the
fp64 formula on the CPU from the same bf16 inputs.  Bound, as
tests/test_gpu_moe_ffn.py's: |out - ref| <= 2^-8 |ref| + n 2^-23 mag, n the
reduce length (2N, N for dx with two, one product; R for dw), mag the product
of absolute values.  Exact inputs: sums exact in fp32, outputs equal."""
import functools

import pytest
import torch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]

BF = torch.bfloat16
CASES = [          # (E, R, K, N)
    (1, 4, 32, 32),       # one step each way, partial tiles, R below 32
    (3, 130, 96, 160),    # odd E, row tile + 2, R % 32 == 2, column tails
    (2, 256, 64, 128),    # exact tiles
    (2, 132, 160, 96),    # K over one dx column tile, the pair tile + a tail
]


def _ops():
    import easydist_amd.ops as ops
    from easydist_amd.ops import moe_ffn
    assert ops.require_hip_ops(), "HIP extension must be loaded on a GPU host"
    return torch.ops.easydist_amd, moe_ffn


def _valid(E, R, kind):     # the patterns of test_gpu_moe_ffn.py::_case
    rows = torch.arange(R).expand(E, R)
    if kind == "prefix":      # an empty expert, a full one, a partial one
        counts = [0, R, R // 2 + 1][:E] if E > 1 else [R // 2]
        return rows < torch.tensor(counts).unsqueeze(1)
    if kind == "segments":    # the EP layout: a prefix in each half of R
        S = R // 2
        seg1 = (torch.arange(E) * S // 2).clamp(max=S).unsqueeze(1)
        return torch.where(rows < S, rows < S // 2, rows - S < seg1)
    return None


@functools.lru_cache(maxsize=None)
def _case(case, kind, exact):
    """bf16 inputs, rows that `valid` clears zeroed, and per output (fp64 ref,
    reduce length, mag).  Exact: g, w in {-1, 0, 1}, x in [-2, 2], sums <= 512."""
    E, R, K, N = case
    _nt = functools.partial(torch.einsum, "ern,ekn->erk")   # g @ w^T
    _tn = functools.partial(torch.einsum, "erk,ern->ekn")   # x^T @ g
    gen = torch.Generator().manual_seed(E + R + K + N)
    shapes = ((E, R, K), (E, R, N), (E, R, N), (E, K, N), (E, K, N))
    if exact:
        x, g1, g2, w1, w2 = (
            torch.randint(-2 if i == 0 else -1, 3 if i == 0 else 2, s,
                          generator=gen).double()
            for i, s in enumerate(shapes))
    else:
        x, g1, g2, w1, w2 = (torch.randn(s, generator=gen) for s in shapes)
        w1, w2 = w1 * N ** -0.5, w2 * N ** -0.5
    valid = _valid(E, R, kind)
    if valid is not None:
        x, g1, g2 = (t * valid.unsqueeze(-1) for t in (x, g1, g2))
    d = dict(x=x.to(BF), g1=g1.to(BF), g2=g2.to(BF), w1=w1.to(BF),
             w2=w2.to(BF), valid=valid)
    x, g1, g2, w1, w2 = (d[k].double() for k in ("x", "g1", "g2", "w1", "w2"))
    xa, g1a, g2a, w1a, w2a = (t.abs() for t in (x, g1, g2, w1, w2))
    d["ref"] = {
        "dx1": (_nt(g1, w1), N, _nt(g1a, w1a)),
        "dx2": (_nt(g1, w1) + _nt(g2, w2), 2 * N,
                _nt(g1a, w1a) + _nt(g2a, w2a)),
        "dw1": (_tn(x, g1), R, _tn(xa, g1a)),
        "dw3": (_tn(x, g2), R, _tn(xa, g2a)),
    }
    return d


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("kind", ["none", "prefix", "segments"])
@pytest.mark.parametrize("case", CASES)
def test_backward_ops(case, kind, exact):
    ed, mf = _ops()
    E, R, K, N = case
    d = _case(case, kind, exact)
    x, g1, g2, w1, w2 = (d[k].cuda() for k in ("x", "g1", "g2", "w1", "w2"))
    valid = None if d["valid"] is None else d["valid"].cuda()
    assert mf._dx_kernel_ok(g1, w1, g2, w2, valid)
    assert mf._dw_kernel_ok(x, valid, g1, g2)
    def run(v):    # NaN where the allocator most likely puts the outputs
        nan = [torch.full(s, float("nan"), dtype=BF, device="cuda")
               for s in 2 * [(E, R, K)] + 4 * [(E, K, N)]]
        del nan
        out = dict(dx1=ed.moe_expert_dx(g1, w1, None, None, v),
                   dx2=ed.moe_expert_dx(g1, w1, g2, w2, v))
        out["dw1"], out["dw3"] = ed.moe_expert_dw2(x, g1, g2, v)
        assert torch.equal(out["dw1"], ed.moe_expert_dw(x, g1, v))  # pair
        assert torch.equal(out["dw3"], ed.moe_expert_dw(x, g2, v))
        return {k: t.cpu() for k, t in out.items()}

    got = run(valid)
    if valid is not None:     # skipping changes no output bit
        for name, t in run(None).items():
            assert torch.equal(got[name], t), name
    for name, t in got.items():
        ref, n, mag = d["ref"][name]
        assert t.shape == ref.shape and t.dtype == BF, name
        assert bool(torch.isfinite(t).all()), name
        for e in range(E if valid is not None else 0):
            # dw of an expert, dx of a 128-row tile, without a valid row
            step = R if name.startswith("dw") else 128
            for r0 in range(0, R, step):
                if not d["valid"][e, r0:r0 + step].any():
                    zero = t[e] if step == R else t[e, r0:r0 + step]
                    assert not zero.any(), (name, e, r0)
        if exact:
            assert torch.equal(t, ref.to(BF)), name
        else:
            err = (t.double() - ref).abs()
            bound = 2.0 ** -8 * ref.abs() + n * 2.0 ** -23 * mag
            worst = float((err / bound.clamp_min(1e-300)).max())
            print(f"moe ffn bwd {case} {kind} {name}: err/bound {worst:.4f}")
            assert bool((err <= bound).all()), (name, worst)


def test_outside_the_envelope_runs_aten():
    ed, mf = _ops()
    gen = torch.Generator().manual_seed(5)
    for N, dtype in ((40, BF), (32, torch.float32)):
        g1, g2, w1, w2 = (torch.randn(s, generator=gen).to(dtype).cuda()
                          for s in 2 * [(2, 8, N)] + 2 * [(2, 16, N)])
        assert not mf._dx_kernel_ok(g1, w1, g2, w2, None)
        got = ed.moe_expert_dx(g1, w1, g2, w2, None)
        assert got.dtype == dtype and torch.equal(
            got, mf._dx_impl(g1, w1, g2, w2))


def test_graph_replay():
    """Forward + backward captured and replayed with changed inputs."""
    from easydist_amd.models.moe import ExpertFFN
    _ops()
    E, R, K, N = 3, 130, 96, 160
    torch.manual_seed(8)
    ffn = ExpertFFN(E, K, N, grouped=True).cuda().to(BF)
    valid = _valid(E, R, "prefix").cuda()
    x0 = (torch.randn(E, R, K, device="cuda") * valid.unsqueeze(-1)).to(BF)
    gy0 = (torch.randn(E, R, K, device="cuda") * valid.unsqueeze(-1)).to(BF)

    def grads(x, gy):
        return torch.autograd.grad(ffn(x, valid), (x, *ffn.parameters()), gy)

    static_x = x0.clone().requires_grad_(True)
    static_gy = gy0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        grads(static_x, static_gy)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_grads = grads(static_x, static_gy)
    for scale in (1.0, 0.5, -2.0):
        with torch.no_grad():
            static_x.copy_(x0 * scale)
            static_gy.copy_(gy0 * scale)
        graph.replay()
        eager = grads((x0 * scale).requires_grad_(True), gy0 * scale)
        for i, (p, q) in enumerate(zip(static_grads, eager)):
            assert bool(torch.isfinite(q).all()) and q.any(), i
            assert torch.equal(p, q), (i, scale)     # dx, dw1, dw3, dw2
