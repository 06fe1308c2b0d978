"""Cross-entropy kernels (ce_fwd_rows, ce_fwd, ce_bwd) against fp64.

References are plain torch in fp64 (on the device) from the rounded logits
the kernel reads. The backward gets lse computed in fp64 and rounded to fp32,
and the reference uses that value upcast, so a forward error cannot hide or
fake a backward one.

Shapes (N, V): (1, 7) tail only; (3, 8) one vector and nothing else; (5, 9)
one vector plus one tail element; (130, 513) idle lanes and a tail element;
(3, 520) a whole wave pass plus one more vector; (130, 1003) a generic odd
size; (5, 50257) the GPT-2 vocabulary, whose rows after the first start at
addresses that are only element-aligned. No N is a multiple of the 4 rows of
a block. Spike cases bring their own rows, one per (position, target) pair.

Inputs: 4 * randn; spike rows, one logit 30 above the row's maximum at column
0, V8 - 1, V8 (first tail element), V - 1, 511 and 512 where V allows
(V8 = V // 8 * 8), the target in turn on the spike, 0 and V - 1: a lost or
doubled element moves lse by O(1); -inf rows, a quarter of the entries -inf,
among them column 0 (the first element of lane 0's first vector), all of
columns 8..15 (a lane with nothing finite, where V <= 520), the whole tail
where a full vector precedes it, the target on a finite entry.

Bounds (u16 = 2^-8, u32 = 2^-24), from the arithmetic: __expf good to about
19 u32 on arguments down to -17, about 100 sequential adds per lane at the
largest V, a handful of rescalings per lane:
  lse, nll   |err| <= 5e-5 + 2 u32 |ref|
  ce_fwd     the scalar within the sum of the per-row bounds of the fp64 sum
  dlogits    |d - ref| <= rnd |ref| + 1e-4 |scale| p_ref, rnd = u16 in bf16
             and 8 u32 in fp32; exactly 0 at -inf logits and on rows whose
             per-row gradient is 0 (the ignore-index path)
Every test prints its worst err / bound.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

U16, U32 = 2.0 ** -8, 2.0 ** -24
SHAPES = ((1, 7), (3, 8), (5, 9), (130, 513), (3, 520), (130, 1003),
          (5, 50257))
KINDS = ("randn", "spike", "neginf")
DTYPES = (torch.bfloat16, torch.float32)
_ids = lambda s: f"{s[0]}x{s[1]}"
_dt = lambda d: "bf16" if d == torch.bfloat16 else "fp32"


@pytest.fixture(scope="module")
def ext():
    import easydist_amd.ops as ops
    e = ops.load_extension()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _spike_pairs(V):
    V8 = V // 8 * 8
    pos = [0, V - 1]
    if V8 > 0:
        pos.append(V8 - 1)
    if V8 < V:
        pos.append(V8)
    pos += [p for p in (511, 512) if p < V]
    pos = sorted(set(pos))
    return [(p, t) for p in pos for t in ("spike", 0, V - 1)]


@functools.lru_cache(maxsize=None)
def _case(kind, dtype, N, V):
    """Logits, targets, gradients and the fp64 references, made once per
    case and shared (read-only)."""
    gen = torch.Generator(device="cuda").manual_seed(
        1009 * V + 13 * N + KINDS.index(kind))
    V8 = V // 8 * 8
    if kind == "spike":
        pairs = _spike_pairs(V)
        N = len(pairs)
    x = 4 * torch.randn(N, V, device="cuda", generator=gen)
    t = torch.randint(0, V, (N,), device="cuda", generator=gen)
    if kind == "spike":
        top = x.amax(-1)
        for r, (p, tg) in enumerate(pairs):
            x[r, p] = top[r] + 30
            t[r] = p if tg == "spike" else tg
    elif kind == "neginf":
        dead = torch.rand(N, V, device="cuda", generator=gen) < 0.25
        dead[:, 0] = True
        if V8 >= 16:
            dead[:, 8:16] = True
        if V8 > 0:
            dead[:, V8:] = True
        if V < 16:
            dead[:, 1] = False    # keep something finite in a tiny row
        x = x.masked_fill(dead, float("-inf"))
        t = torch.multinomial((~dead).float(), 1, generator=gen).squeeze(1)
    x = x.to(dtype).contiguous()
    c = dict(x=x, t=t, N=N, V=V)
    x64 = x.double()
    c["lse"] = torch.logsumexp(x64, -1)
    c["nll"] = c["lse"] - x64.gather(1, t.unsqueeze(1)).squeeze(1)
    # backward: lse rounded to fp32 goes to the kernel and, upcast, here
    c["lse32"] = c["lse"].float()
    p = torch.exp(x64 - c["lse32"].double().unsqueeze(1))
    c["p"] = p
    c["pm"] = p.clone()
    c["pm"][torch.arange(N, device="cuda"), t] -= 1.0
    c["g_scalar"] = torch.tensor(0.37, device="cuda")
    g = torch.randn(N, device="cuda", generator=gen)
    g[1::3] = 0.0                  # rows the ignore-index path switches off
    c["g_rows"] = g
    return c


def _ratio(err, bound):
    """Worst err / bound; a zero bound demands a zero error, and a NaN or
    inf anywhere is a miss (NaN <= bound is False)."""
    r = torch.where(bound > 0, err / bound, torch.zeros_like(err))
    return float(r.max()), bool((~(err <= bound)).any())


def _fwd_bound(ref):
    return 5e-5 + 2 * U32 * ref.abs()


def _check_rows(tag, c, nll, lse):
    N = c["N"]
    for name, t in (("lse", lse), ("nll", nll)):
        assert t.dtype == torch.float32 and tuple(t.shape) == (N,), (tag, name)
        assert bool(torch.isfinite(t).all()), (tag, name, "not finite")
    wl, bl = _ratio((lse.double() - c["lse"]).abs(), _fwd_bound(c["lse"]))
    wn, bn = _ratio((nll.double() - c["nll"]).abs(), _fwd_bound(c["nll"]))
    print(f"{tag} lse worst err/bound {wl:.3f}  nll {wn:.3f}")
    assert not bl and not bn, (tag, wl, wn)


def _check_bwd(tag, c, d, scale):
    x = c["x"]
    assert d.dtype == x.dtype and d.shape == x.shape, tag
    s64 = scale.double().reshape(-1, 1)
    ref = c["pm"] * s64
    rnd = U16 if x.dtype == torch.bfloat16 else 8 * U32
    bound = rnd * ref.abs() + 1e-4 * s64.abs() * c["p"]
    worst, bad = _ratio((d.double() - ref).abs(), bound)
    print(f"{tag} dlogits worst err/bound {worst:.3f}")
    assert not bad, (tag, worst)
    assert bool((d[torch.isinf(x)] == 0).all()), (tag, "-inf entries")
    if scale.numel() > 1:
        assert bool((d[scale == 0] == 0).all()), (tag, "zero-grad rows")


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("kind", KINDS)
def test_ce_fwd(ext, kind, dtype, shape):
    c = _case(kind, dtype, *shape)
    tag = f"ce_fwd {kind} {_dt(dtype)} {_ids(shape)}"
    nll, lse = ext.ce_fwd_rows(c["x"], c["t"])
    _check_rows(tag, c, nll, lse)
    total, lse2 = ext.ce_fwd(c["x"], c["t"])
    assert total.dtype == torch.float32 and total.dim() == 0, tag
    assert torch.equal(lse2, lse), tag
    err = abs(float(total.double() - c["nll"].sum()))
    bound = float(_fwd_bound(c["nll"]).sum())
    print(f"{tag} sum err/bound {err / bound:.3f}")
    assert err <= bound, (tag, err, bound)


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("kind", KINDS)
def test_ce_bwd(ext, kind, dtype, shape):
    c = _case(kind, dtype, *shape)
    tag = f"ce_bwd {kind} {_dt(dtype)} {_ids(shape)}"
    d = ext.ce_bwd(c["g_scalar"], c["x"], c["t"], c["lse32"])
    _check_bwd(tag + " scalar", c, d, c["g_scalar"])
    if c["N"] > 1:     # one row: a [1] gradient is the scalar form
        d = ext.ce_bwd(c["g_rows"], c["x"], c["t"], c["lse32"])
        _check_bwd(tag + " per-row", c, d, c["g_rows"])


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_ce_ops_noncontiguous(ext, dtype):
    """The registered ops on a column slice of a wider buffer."""
    c = _case("randn", dtype, 130, 1003)
    wide = torch.zeros(130, 1003 + 10, device="cuda", dtype=dtype)
    view = wide[:, 3:3 + 1003]
    view.copy_(c["x"])
    assert not view.is_contiguous()
    tag = f"ce ops view {_dt(dtype)}"
    nll, lse = torch.ops.easydist_amd.ce_fwd_rows(view, c["t"])
    _check_rows(tag, c, nll, lse)
    d = torch.ops.easydist_amd.ce_bwd(c["g_rows"], view, c["t"], c["lse32"])
    _check_bwd(tag, c, d, c["g_rows"])


@requires_gpu
def test_rms_norm_module_into_ce(ext):
    """RMSNorm (default fp32 weight) on bf16 activations feeding the loss:
    logits, loss and both gradients against fp64. The dlogits the norm's
    backward receives are within (u16 + 1e-4) of their reference, which
    the linear backward carries through; 2 u16 covers it. That makes the dw
    bound here about one row's share of a column (2 u16 of 130 rows): this
    case checks the chain and its dtypes, and would not see a dropped row.
    tests/test_gpu_norm_exact.py holds rms_norm_bwd's dw to
    (rows + 8) u32, which does."""
    from easydist_amd.ops.ce import cross_entropy
    from easydist_amd.ops.norms import RMSNorm
    N, V, eps = 130, 520, 1e-6
    gen = torch.Generator(device="cuda").manual_seed(77)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    mod = RMSNorm(V, eps=eps).cuda()
    with torch.no_grad():
        mod.weight.copy_(0.5 * rn(V))   # no softmax entry near 1
    x = (2 * rn(N, V)).bfloat16().requires_grad_()
    t = torch.randint(0, V, (N,), device="cuda", generator=gen)
    h = mod(x)
    loss = cross_entropy(h, t)
    loss.backward()
    assert h.dtype == torch.bfloat16 and x.grad.dtype == torch.bfloat16
    assert mod.weight.grad.dtype == torch.float32

    w64 = mod.weight.detach().bfloat16().double()   # what the kernel reads
    x64 = x.detach().double()
    r = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + eps)
    xh = x64 * r
    ref = xh * w64
    worst, bad = _ratio((h.detach().double() - ref).abs(),
                        U16 * ref.abs() + 1e-5 * ref.abs())
    line = f"rms->ce logits {worst:.3f}"
    assert not bad, ("logits", worst)
    # from here on the reference starts at the logits the loss kernel read
    h64 = h.detach().double()
    lse = torch.logsumexp(h64, -1)
    nll = lse - h64.gather(1, t.unsqueeze(1)).squeeze(1)
    err = abs(float(loss.detach().double() * N - nll.sum()))
    bound = float(_fwd_bound(nll).sum())
    line += f" loss {err / bound:.3f}"
    assert err <= bound, ("loss", err, bound)
    g = torch.exp(h64 - lse.unsqueeze(1))
    g[torch.arange(N, device="cuda"), t] -= 1.0
    g = g / N
    gw = g * w64
    c2 = (gw * xh).mean(-1, keepdim=True)
    dx = r * (gw - xh * c2)
    carried = r * (gw.abs() + xh.abs() * (gw * xh).abs().mean(-1,
                                                               keepdim=True))
    worst, bad = _ratio((x.grad.double() - dx).abs(),
                        U16 * dx.abs() + (2 * U16 + 1e-5) * carried)
    line += f" dx {worst:.3f}"
    assert not bad, ("dx", worst)
    tw = g * xh
    worst, bad = _ratio((mod.weight.grad.double() - tw.sum(0)).abs(),
                        (2 * U16 + (N + 8) * U32) * tw.abs().sum(0))
    print(line + f" dw {worst:.3f}")
    assert not bad, ("dw", worst)
