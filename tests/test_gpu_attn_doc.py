"""Document-masked causal attention in the flash kernels against fp32 SDPA
with the dense boolean mask; helpers and tolerances are those of
tests/test_gpu_attn_swa.py (seed per case, NaN poisoning, NaN ragged tail)."""
import math

import pytest
import torch
from test_gpu_attn_swa import ENV, _inputs, _poison, ext  # noqa: F401

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]
# (B, H, Hkv, S, D, document lengths per batch row, strided)
CASES = [
    (1, 2, 2, 128, 64, [[1] * 128], False),   # the diagonal only: out == v
    (1, 2, 2, 256, 64, [[256]], False),       # bounds that mask nothing
    # a boundary on a tile edge (q block 1 starts at tile 1, odd first buffer;
    # the dkv q range ends on a tile edge); row 1 differs, with a boundary
    # mid-wave: a leading tile fully masked for some rows of a wave only
    (2, 2, 2, 256, 64, [[128, 128], [70, 58, 128]], False),
    (1, 2, 1, 384, 64, [[200, 10, 174]], False),  # GQA, 3 blocks, dkv q range
                                                  # ends mid-tile, doc in a wave
    (1, 4, 2, 197, 64, [[50, 100, 47]], True),    # ragged GQA, qkv views
    (1, 2, 2, 300, 128, [[129, 171]], False),     # D = 128 (8-wave dkv), ragged
    (1, 2, 1, 130, 128, [[129, 1]], False),       # two-row last block; the last
                                                  # row is a document of its own
]
IDS = ["B{}H{}K{}S{}D{}n{}{}".format(*c[:5], len(c[5][-1]), "v" * c[6])
       for c in CASES]
STRIDED_CASE = 4


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _run(ext, q, k, v, g, lo, hi):
    (B, H, S, D), Hkv = q.shape, k.shape[1]
    bf, f32 = torch.bfloat16, torch.float32
    _poison(((B, H, S, D), bf), ((B, H, S), f32))
    out, lse = ext.flash_attn_fwd(q, k, v, True, None, lo, hi)
    _poison(((B, H, S, D), bf), ((B, Hkv, S, D), bf), ((B, Hkv, S, D), bf),
            ((B, H, S), f32))
    dq, dk, dv = ext.flash_attn_bwd(g, q, k, v, out, lse, True, None, lo, hi)
    torch.cuda.synchronize()
    return {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


_cache = {}


def _case(ext, idx):
    """Inputs, kernel results and fp32 reference of a case, computed once."""
    if idx in _cache:
        return _cache[idx]
    B, H, Hkv, S, D, lengths, strided = CASES[idx]
    G = H // Hkv
    torch.manual_seed(1600 + idx)
    q, k, v, g = _inputs(B, H, Hkv, S, D, strided)
    n = [torch.tensor(row) for row in lengths]
    assert all(int(r.sum()) == S for r in n)
    lo = torch.stack([(r.cumsum(0) - r).repeat_interleave(r) for r in n])
    hi = torch.stack([r.cumsum(0).repeat_interleave(r) for r in n])
    lo, hi = lo.int().cuda(), hi.int().cuda()
    got = _run(ext, q, k, v, g, lo, hi)
    j = torch.arange(S, device="cuda")
    mask = ((j >= lo[:, :, None]) & (j <= j[:, None]))[:, None]
    qf, kf, vf = (t.float().contiguous().requires_grad_(True)
                  for t in (q, k, v))
    ke = kf.repeat_interleave(G, dim=1)
    ref = torch.nn.functional.scaled_dot_product_attention(
        qf, ke, vf.repeat_interleave(G, dim=1), attn_mask=mask)
    ref.backward(g.float())
    s = (qf @ ke.transpose(-1, -2)).detach() / math.sqrt(D)
    want = {"out": ref.detach(), "dq": qf.grad, "dk": kf.grad, "dv": vf.grad,
            "lse": torch.logsumexp(s.masked_fill(~mask, -math.inf), -1)}
    _cache[idx] = ((q, k, v, g, lo, hi), got, want)
    return _cache[idx]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_doc_against_fp32_reference(ext, idx):
    (B, H, Hkv, S, D, lengths, _), tag = CASES[idx], IDS[idx]
    G = H // Hkv
    (q, k, v, g, lo, hi), got, want = _case(ext, idx)
    err = {n: float((got[n].float() - want[n]).abs().max()) for n in got}
    print(tag, err)
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), (tag, name, "not finite")
        assert t.shape == want[name].shape, (tag, name)
    assert torch.allclose(got["out"].float(), want["out"],
                          atol=3e-2, rtol=3e-2), (tag, err)
    if max(map(max, lengths)) == 1:   # softmax over the one visible key is 1.0
        assert torch.equal(got["out"], v), (tag, "out != v")
    assert torch.allclose(got["lse"], want["lse"], atol=1e-2, rtol=1e-3), \
        (tag, err)
    # dk and dv sum G per-head gradients: G times the per-head bound
    assert err["dq"] < 8e-2 and err["dk"] < G * 8e-2 \
        and err["dv"] < G * 8e-2, (tag, err)


@pytest.mark.parametrize("idx", [3, 5], ids=[IDS[3], IDS[5]])
def test_other_dkv_geometry_is_bit_identical(ext, monkeypatch, idx):
    """8 waves at D = 64, 4 at D = 128: the geometry that is not the
    default; the extra q tiles its blocks walk add exact zeros."""
    args, got, _ = _case(ext, idx)
    monkeypatch.setenv("EASYDIST_DKV_GEOM", "0" if CASES[idx][4] == 64 else "1")
    other = _run(ext, *args)
    for name in got:
        assert torch.equal(other[name], got[name]), (IDS[idx], name)


def test_public_op_runs_the_document_kernels(ext, monkeypatch):
    """The op with the aten math path taken away, on the strided ragged GQA
    case: the tensors of the direct kernel calls."""
    from easydist_amd.ops import attention

    def _no_math(*a, **kw):
        raise AssertionError("aten math path taken at a kernel shape")

    monkeypatch.setattr(attention, "_math_fwd", _no_math)
    monkeypatch.setattr(attention, "_math_bwd", _no_math)
    (q, k, v, g, lo, hi), ker, _ = _case(ext, STRIDED_CASE)
    assert not q.is_contiguous() and k.shape[1] < q.shape[1]
    ql, kl, vl = (t.detach().requires_grad_(True) for t in (q, k, v))
    out = attention.scaled_dot_product_attention(ql, kl, vl, causal=True,
                                                 doc_bounds=(lo, hi))
    out.backward(g)
    torch.cuda.synchronize()
    got = {"out": out.detach(), "dq": ql.grad, "dk": kl.grad, "dv": vl.grad}
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), (name, "not finite")
        assert torch.equal(t, ker[name]), name
