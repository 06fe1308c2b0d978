"""Flash attention under the two workgroup maps (EASYDIST_ATTN_MAP).

The map only moves blocks between workgroup ids; per-block arithmetic is
the same, so legacy (0) and balanced (1) outputs must be bit-identical,
and balanced must meet the fp32 SDPA reference within the bounds of
tests/test_gpu_kernels.py.  Shapes are the smallest at which a wrong map
goes wrong: fewer workgroups than XCDs, a swizzle remainder, nblk = 8 with
heads straddling XCD groups, odd nblk, and the D = 128 variants.

A block the map never reaches leaves at::empty memory unwritten, and the
caching allocator may hand back a buffer that still holds a previous
call's right answer.  So every case has its own seed, output-sized
NaN-filled tensors are allocated and freed right before each call under
test, and the outputs must be finite.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

# (B, H, S, D, causal)
CASES = [
    (1, 3, 128, 64, True),     # nblk 1, nbh 3: fewer workgroups than XCDs
    (2, 3, 384, 64, True),     # nblk 3, nbh 6: 18 workgroups, remainder 2
    (2, 3, 384, 64, False),    # same, no mask
    (1, 5, 1024, 64, True),    # nblk 8: heads straddle XCD groups
    (1, 3, 1152, 64, True),    # odd nblk 9, 27 workgroups
    (1, 2, 256, 128, True),    # D = 128 variants
]


@pytest.fixture(scope="module")
def ext():
    import easydist_amd.ops as ops
    e = ops.load_extension()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _poison(*shapes_dtypes):
    """Allocate, NaN-fill and free tensors of the output sizes so the
    outputs of the next call most likely reuse poisoned memory."""
    ts = [torch.full(s, float("nan"), device="cuda", dtype=dt)
          for s, dt in shapes_dtypes]
    torch.cuda.synchronize()
    del ts


def _run(ext, q, k, v, g, causal):
    B, H, S, D = q.shape
    bf, f32 = torch.bfloat16, torch.float32
    _poison(((B, H, S, D), bf), ((B, H, S), f32))
    out, lse = ext.flash_attn_fwd(q, k, v, causal)
    _poison(((B, H, S, D), bf), ((B, H, S, D), bf), ((B, H, S, D), bf),
            ((B, H, S), f32))
    dq, dk, dv = ext.flash_attn_bwd(g, q, k, v, out, lse, causal)
    _poison(((B, S, 3 * H * D), bf), ((B, H, S), f32))
    packed = ext.flash_attn_bwd_pack(g, q, k, v, out, lse, causal)
    torch.cuda.synchronize()
    return {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv,
            "packed": packed}


@requires_gpu
@pytest.mark.parametrize("case", list(enumerate(CASES)),
                         ids=lambda c: "B{}H{}S{}D{}{}".format(
                             *c[1][:4], "c" if c[1][4] else "n"))
def test_attn_block_map_modes(ext, monkeypatch, case):
    idx, (B, H, S, D, causal) = case
    torch.manual_seed(100 + idx)
    q, k, v, g = (torch.randn(B, H, S, D, device="cuda",
                              dtype=torch.bfloat16) for _ in range(4))

    monkeypatch.setenv("EASYDIST_ATTN_MAP", "0")
    legacy = _run(ext, q, k, v, g, causal)
    monkeypatch.setenv("EASYDIST_ATTN_MAP", "1")
    bal = _run(ext, q, k, v, g, causal)

    for name, t in bal.items():
        assert bool(torch.isfinite(t).all()), ("balanced", name)
        assert bool(torch.isfinite(legacy[name]).all()), ("legacy", name)
        # 1. bit equality between the two maps
        assert torch.equal(t, legacy[name]), \
            (name, float((t.float() - legacy[name].float()).abs().max()))

    # the packed buffer holds the same dq/dk/dv
    ref_packed = torch.cat([bal[n].transpose(1, 2).reshape(B, S, H * D)
                            for n in ("dq", "dk", "dv")], -1)
    assert torch.equal(bal["packed"], ref_packed)

    # 2. balanced mode against the fp32 reference
    qf = q.float().requires_grad_(True)
    kf = k.float().requires_grad_(True)
    vf = v.float().requires_grad_(True)
    ref = torch.nn.functional.scaled_dot_product_attention(
        qf, kf, vf, is_causal=causal)
    ref.backward(g.float())
    ref = ref.detach()
    err = float((bal["out"].float() - ref).abs().max())
    assert torch.allclose(bal["out"].float(), ref, atol=3e-2, rtol=3e-2), \
        ("out", err)
    s = q.float() @ k.float().transpose(-1, -2) / math.sqrt(D)
    if causal:
        mask = torch.ones(S, S, device="cuda", dtype=torch.bool).tril()
        s = s.masked_fill(~mask, float("-inf"))
    lref = torch.logsumexp(s, -1)
    assert torch.allclose(bal["lse"], lref, atol=1e-2, rtol=1e-3), \
        ("lse", float((bal["lse"] - lref).abs().max()))
    for name, want in (("dq", qf.grad), ("dk", kf.grad), ("dv", vf.grad)):
        e = float((bal[name].float() - want).abs().max())
        assert e < 8e-2, (name, e, B, H, S, D)
