"""The gfx950 MoE expert FFN kernels (moe_nn in csrc/gemm_kernels.hip)
against the fp64 bmm / silu formula on the CPU from the same bf16 inputs.

Bounds (K the reduce length, mag the fp64 sum of |x w| over k):

    product:  |out - ref| <= 2^-8 |ref| + K 2^-23 mag
    h:        |h - ref|   <= (2^-8 + 2^-18) |ref|
                             + K 2^-23 (1.1 |b| mag_a + |silu(a)| mag_b)

2^-8 |ref| is the one rounding to bf16 (twice the half-ulp), K 2^-23 mag the
fp32 accumulation in any order (twice the worst case), 1.1 bounds silu's
derivative, 2^-18 |ref| is the allowance for the fast exponential and the
hardware reciprocal.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]

BF = torch.bfloat16
CASES = [          # (E, R, K, N)
    (1, 4, 32, 8),        # one k-step, one partial tile in both directions
    (3, 130, 96, 136),    # odd E, row tile + 2, 3 k-steps, col tile + 8
    (2, 256, 64, 128),    # exact tiles
    (2, 132, 160, 72),    # the SwiGLU column tile (64) plus a tail
]
VALID = ["none", "prefix", "segments"]


def _ops():
    import easydist_amd.ops as ops
    from easydist_amd.ops import moe_ffn
    assert ops.require_hip_ops(), "HIP extension must be loaded on a GPU host"
    return torch.ops.easydist_amd, moe_ffn


def _bound(ref, K, mag, rel=2.0 ** -8):
    return rel * ref.abs() + K * 2.0 ** -23 * mag


@functools.lru_cache(maxsize=None)
def _case(case, kind, exact):
    """bf16 inputs with the rows that `valid` clears zeroed, and the fp64
    references; shared.  Exact inputs: x integers in [-2, 2] (in [-1, 1]
    from k = 64 on), weights in {-1, 0, 1}: every product sum is an integer
    of magnitude <= 128 + (K - 64) <= 224, exact in fp32 and in bf16."""
    E, R, K, N = case
    g = torch.Generator().manual_seed(E + R + K + N)
    if exact:
        x = torch.randint(-2, 3, (E, R, K), generator=g).double()
        x[..., 64:].clamp_(-1, 1)
        w1, w3 = (torch.randint(-1, 2, (E, K, N), generator=g).double()
                  for _ in range(2))
    else:
        x = torch.randn(E, R, K, generator=g)
        w1, w3 = (torch.randn(E, K, N, generator=g) * K ** -0.5
                  for _ in range(2))
    rows = torch.arange(R).expand(E, R)
    valid = None
    if kind == "prefix":      # an empty expert, a full one, a partial one
        counts = [0, R, R // 2 + 1][:E] if E > 1 else [R // 2]
        valid = rows < torch.tensor(counts).unsqueeze(1)
    elif kind == "segments":  # the EP layout: a prefix in each half of R
        S = R // 2
        seg1 = (torch.arange(E) * S // 2).clamp(max=S).unsqueeze(1)
        valid = torch.where(rows < S, rows < S // 2, rows - S < seg1)
    if valid is not None:
        x = x * valid.unsqueeze(-1)
    d = dict(x=x.to(BF), w1=w1.to(BF), w3=w3.to(BF), valid=valid)
    xd, w1d, w3d = (d[k].double() for k in ("x", "w1", "w3"))
    a, b = torch.bmm(xd, w1d), torch.bmm(xd, w3d)
    mag_a = torch.bmm(xd.abs(), w1d.abs())
    mag_b = torch.bmm(xd.abs(), w3d.abs())
    d["ref"] = dict(a=a, b=b, h=F.silu(a) * b)
    d["mag"] = dict(a=mag_a, b=mag_b,
                    h=1.1 * b.abs() * mag_a + F.silu(a).abs() * mag_b)
    return d


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("kind", VALID)
@pytest.mark.parametrize("case", CASES)
def test_forward(case, kind, exact):
    ed, mf = _ops()
    E, R, K, N = case
    d = _case(case, kind, exact)
    x, w1, w3 = (d[k].cuda() for k in ("x", "w1", "w3"))
    valid = None if d["valid"] is None else d["valid"].cuda()
    assert mf._kernel_ok(x, valid, w1, w3)
    nan = torch.full((E, R, N), float("nan"), dtype=BF, device="cuda")
    del nan        # the allocator most likely hands this memory to c
    c = ed.moe_expert_gemm(x, w1, valid)
    nan = [torch.full((E, R, N), float("nan"), dtype=BF, device="cuda")
           for _ in range(3)]
    del nan
    h, a, b = ed.moe_expert_up(x, w1, w3, valid)
    got = {k: v.cpu() for k, v in dict(c=c, a=a, b=b, h=h).items()}
    for name, t in got.items():
        ref = d["ref"]["a" if name == "c" else name]
        mag = d["mag"]["a" if name == "c" else name]
        assert t.shape == (E, R, N) and t.dtype == BF, name
        assert bool(torch.isfinite(t).all()), name
        for e in range(E if valid is not None else 0):
            for r0 in range(0, R, 128):     # skipped tiles are exact zeros
                if not d["valid"][e, r0:r0 + 128].any():
                    assert not t[e, r0:r0 + 128].any(), (name, e, r0)
        if exact and name != "h":
            assert torch.equal(t, ref.to(BF)), name
        else:
            rel = 2.0 ** -8 + (2.0 ** -18 if name == "h" else 0.0)
            err = (t.double() - ref).abs()
            bound = _bound(ref, K, mag, rel)
            worst = float((err / bound.clamp_min(1e-300)).max())
            print(f"moe ffn {case} {kind} {name}: worst err/bound {worst:.4f}")
            assert bool((err <= bound).all()), (name, worst)


def test_outside_the_envelope_runs_aten():
    ed, mf = _ops()
    g = torch.Generator().manual_seed(5)
    for K, dtype in ((40, BF), (32, torch.float32)):
        x, w1, w3 = (torch.randn(s, generator=g).to(dtype).cuda()
                     for s in ((2, 8, K), (2, K, 16), (2, K, 16)))
        assert not mf._kernel_ok(x, None, w1, w3)
        for got, want in zip(ed.moe_expert_up(x, w1, w3, None),
                             mf._up_impl(x, w1, w3)):
            assert got.dtype == dtype and torch.equal(got, want)
        assert torch.equal(ed.moe_expert_gemm(x, w1, None),
                           mf._gemm_impl(x, w1))


def _mm(p, q):
    return torch.bmm(p.abs(), q.abs())


def _acc(p, q):         # fp32 accumulation of p @ q in any order
    return p.shape[2] * 2.0 ** -23 * _mm(p, q)


def test_autograd():
    """ExpertFFN(grouped=True) in bf16 against fp64 autograd of the plain
    formula.  tests/test_gpu_swiglu.py::test_real_values bounds a bf16
    gradient by 2^-8 |ref| + 2^-18 mag (mag = |dy u| (1 + |g|) for dgate,
    |dy g| for dup): that is swiglu_bwd's own da and db from exact inputs.
    Here its inputs a, b and gh = gy w2^T are bf16 roundings already and the
    gradients are GEMMs of da and db, so the bound departs from that test's:
    each rounding enters to first order, u = 2^-8 (twice the half-ulp) of
    the signed fp64 value, with silu' <= 1.1 and silu'' <= 0.5 (egh, eda,
    edb, eh below), and is carried through the gradient's GEMM as a |.|
    product; acc = n 2^-23 mag per GEMM; for dx also u |da w1^T|, the first
    product of the baddbmm being rounded on its own."""
    from easydist_amd.models.moe import ExpertFFN
    _ops()
    case = (3, 130, 96, 136)
    E, R, K, N = case
    d = _case(case, "prefix", False)
    ffn = ExpertFFN(E, K, N, grouped=True).to(BF)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        ffn.w1.copy_(d["w1"])
        ffn.w3.copy_(d["w3"])
        ffn.w2.copy_(torch.randn(E, N, K, generator=g) * N ** -0.5)
    gy = torch.randn(E, R, K, generator=g).to(BF)
    ref = [t.detach().double().requires_grad_(True)
           for t in (d["x"], ffn.w1, ffn.w3, ffn.w2)]
    xd, w1d, w3d, w2d = ref
    a, b = torch.bmm(xd, w1d), torch.bmm(xd, w3d)
    h = F.silu(a) * b
    torch.bmm(h, w2d).backward(gy.double())

    ffn = ffn.cuda()
    x = d["x"].cuda().requires_grad_(True)
    ffn(x, d["valid"].cuda()).backward(gy.cuda())

    with torch.no_grad():
        u, v, gyd = 2.0 ** -8, 2.0 ** -18, gy.double()
        xt, w1t, w3t, w2t = (m.transpose(1, 2) for m in ref)
        s = torch.sigmoid(a)
        gh, f, sa = torch.bmm(gyd, w2t), b * s * (1 + a * (1 - s)), a * s
        da, db = gh * f, gh * sa
        # eda: gh's error; b's and da's rounding; a's; swiglu_bwd's own term
        egh = u * gh.abs() + _acc(gyd, w2t)
        eda = (egh * f.abs() + u * (2 * da.abs() + 0.5 * (gh * a * b).abs())
               + v * (gh * b).abs() * (1 + a.abs()))
        edb = (egh * sa.abs() + u * (db.abs() + 1.1 * (gh * a).abs())
               + v * (gh * a).abs())
        eh = (u + v) * h.abs() + K * 2.0 ** -23 * d["mag"]["h"]
        tails = (_mm(eda, w1t) + _mm(edb, w3t) + u * torch.bmm(da, w1t).abs()
                 + _acc(da, w1t) + _acc(db, w3t),
                 _mm(xt, eda) + _acc(xt, da), _mm(xt, edb) + _acc(xt, db),
                 _mm(eh.transpose(1, 2), gyd) + _acc(h.transpose(1, 2), gyd))
    for name, got, want, tail in zip(("dx", "dw1", "dw3", "dw2"),
                                     (x, ffn.w1, ffn.w3, ffn.w2), ref, tails):
        err = (got.grad.cpu().double() - want.grad).abs()
        bound = u * want.grad.abs() + tail
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"moe ffn autograd {name}: worst err/bound {worst:.4f}")
        assert bool((err <= bound).all()), (name, worst)


def test_moe_layer_and_graph_replay():
    """A bf16 MoELayer with grouped_experts against the same weights
    without.  Per expert the plain path rounds a, b, silu(a) and the product
    where the grouped one rounds h once: with the half-ulp 2^-9 and
    silu' <= 1.1, |dh| <= 2^-9 (1.1 |a b| + 4 |h|) on the signed a, b.  It
    goes through w2 as a |.| product, with both paths' accumulation and the
    rounding of both expert outputs (2^-8 |y_e|), then through the combine
    with its gates; 2^-8 |ref| is the rounding of the two layer outputs.
    dx by test_gpu_moe_routing.py::test_moe_layer_autograd's ratio, 2^-6."""
    import copy
    import dataclasses
    from easydist_amd.models.moe import MIXTRAL_SMALL, MoELayer
    from easydist_amd.ops.moe_ops import _combine_impl
    ed, _ = _ops()
    torch.manual_seed(7)
    cfg = dataclasses.replace(MIXTRAL_SMALL, grouped_experts=True)
    layer = MoELayer(cfg).cuda().to(BF)
    plain = copy.deepcopy(layer)
    plain.experts.grouped = False
    x0 = torch.randn(4, 128, cfg.n_embd, device="cuda").to(BF)
    gy = torch.randn_like(x0)
    outs = []
    for m in (layer, plain):
        x = x0.clone().requires_grad_(True)
        y = m(x)
        y.backward(gy)
        outs.append((y.detach().cpu().double(), x.grad.float()))
    (y, dx), (yp, dxp) = outs

    with torch.no_grad():
        tok = x0.reshape(-1, cfg.n_embd)
        topv, topi = F.softmax(plain.router(tok).float(), -1).topk(cfg.top_k)
        topv = (topv / topv.sum(-1, keepdim=True)).to(BF)
        bins, gates, src, valid = (t.cpu() for t in ed.moe_bins(
            tok, topi, topv, cfg.n_experts, cfg.capacity_factor))
        w1, w3, w2 = (w.detach().cpu().double() for w in
                      (plain.experts.w1, plain.experts.w3, plain.experts.w2))
        a, b = torch.bmm(bins.double(), w1), torch.bmm(bins.double(), w3)
        h = F.silu(a) * b
        eh = 2.0 ** -9 * (1.1 * (a * b).abs() + 4 * h.abs())
        ey = _mm(eh, w2) + 2 * _acc(h, w2) + 2.0 ** -8 * torch.bmm(h, w2).abs()
        tail = _combine_impl(ey, gates.double(), src, valid, tok, cfg.top_k)
    err = (y - yp).abs()
    bound = 2.0 ** -8 * yp.abs() + tail.reshape(y.shape)
    worst = float((err / bound.clamp_min(1e-30)).max())
    ratio = float((dx - dxp).abs().max() / dxp.abs().max())
    print(f"moe ffn layer: worst err/bound {worst:.4f}, dx ratio {ratio:.3e}")
    assert bool((err <= bound).all()), worst
    assert ratio <= 2.0 ** -6, ratio

    # the forward under graph capture, replayed, equals eager
    static_x = x0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        layer(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        static_y = layer(static_x)
    for scale in (1.0, 0.5, 2.0):
        static_x.copy_(x0 * scale)
        graph.replay()
        with torch.no_grad():
            assert torch.equal(static_y, layer(x0 * scale)), scale


