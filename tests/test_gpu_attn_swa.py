"""Sliding-window causal attention in the flash kernels: row i attends keys
i - W < j <= i.  Reference: fp32 SDPA with a boolean band mask, logsumexp
for lse, K/V repeat_interleave'd.  Helpers and tolerances as in
tests/test_gpu_attn_gqa.py (seed per case, NaN poisoning, NaN ragged tail).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
# (B, H, Hkv, S, D, W, strided)
CASES = [
    (1, 2, 2, 128, 64, 1, False),     # the diagonal only: out == v exactly
    (2, 2, 2, 256, 64, 64, False),    # q block 1 starts at tile 1 (odd first
                                      # buffer); the left edge cuts every tile
    (1, 2, 2, 256, 64, 16, False),    # a leading tile fully masked for some
                                      # rows of a wave only
    (1, 2, 1, 384, 64, 100, False),   # GQA, 3 blocks, dkv q range ends mid-tile
    (1, 4, 2, 197, 64, 70, True),     # ragged GQA, views of a qkv buffer
    (1, 2, 2, 300, 128, 129, False),  # D = 128 (8-wave dkv), ragged
    (1, 2, 1, 130, 128, 3, False),    # last block has two rows; the window
                                      # reaches back across the block edge
]
IDS = ["B{}H{}K{}S{}D{}W{}{}".format(*c[:6], "v" if c[6] else "")
       for c in CASES]
STRIDED_CASE = 4
ENV = ("EASYDIST_ATTN_MAP", "EASYDIST_ATTN_TR", "EASYDIST_DKV_SWAP",
       "EASYDIST_DKV_GEOM")


@pytest.fixture(scope="module")
def ext():
    import easydist_amd.ops as ops
    e = ops.load_extension()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _poison(*shapes_dtypes):
    """NaN-filled tensors of the output sizes, freed for the next call."""
    ts = [torch.full(s, float("nan"), device="cuda", dtype=dt)
          for s, dt in shapes_dtypes]
    torch.cuda.synchronize()
    del ts


def _run(ext, q, k, v, g, *window):
    """fwd + bwd through the extension; no window = the causal calls as
    every earlier caller spells them."""
    (B, H, S, D), Hkv = q.shape, k.shape[1]
    bf, f32 = torch.bfloat16, torch.float32
    _poison(((B, H, S, D), bf), ((B, H, S), f32))
    out, lse = ext.flash_attn_fwd(q, k, v, True, *window)
    _poison(((B, H, S, D), bf), ((B, Hkv, S, D), bf), ((B, Hkv, S, D), bf),
            ((B, H, S), f32))
    dq, dk, dv = ext.flash_attn_bwd(g, q, k, v, out, lse, True, *window)
    torch.cuda.synchronize()
    return {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def _inputs(B, H, Hkv, S, D, strided):
    """q, g [B, H, S, D], k, v [B, Hkv, S, D]: [:S] views whose rows up to
    the next multiple of 128 are NaN; strided: views of one qkv buffer."""
    Sp, bf = (S + 127) // 128 * 128, torch.bfloat16
    if strided:
        qkv = torch.randn(B, Sp, (H + 2 * Hkv) * D, device="cuda", dtype=bf)
        full = list(qkv.split([H * D, Hkv * D, Hkv * D], dim=2))
        full.append(torch.randn(B, Sp, H * D, device="cuda", dtype=bf))
        full = [t.view(B, Sp, -1, D).transpose(1, 2) for t in full]
    else:
        full = [torch.randn(B, h, Sp, D, device="cuda", dtype=bf)
                for h in (H, Hkv, Hkv, H)]
    for t in full:
        t[:, :, S:] = float("nan")
    return tuple(t[:, :, :S] for t in full)


_cache = {}


def _case(ext, idx):
    """Inputs, kernel results and fp32 reference of a case, computed once."""
    if idx in _cache:
        return _cache[idx]
    B, H, Hkv, S, D, W, strided = CASES[idx]
    G = H // Hkv
    torch.manual_seed(1200 + idx)
    q, k, v, g = _inputs(B, H, Hkv, S, D, strided)
    got = _run(ext, q, k, v, g, W)
    i = torch.arange(S, device="cuda")
    band = (i[None, :] <= i[:, None]) & (i[None, :] > i[:, None] - W)
    qf, kf, vf = (t.float().contiguous().requires_grad_(True)
                  for t in (q, k, v))
    ke = kf.repeat_interleave(G, dim=1)
    ref = torch.nn.functional.scaled_dot_product_attention(
        qf, ke, vf.repeat_interleave(G, dim=1), attn_mask=band)
    ref.backward(g.float())
    s = (qf @ ke.transpose(-1, -2)).detach() / math.sqrt(D)
    want = {"out": ref.detach(), "dq": qf.grad, "dk": kf.grad, "dv": vf.grad,
            "lse": torch.logsumexp(s.masked_fill(~band, -math.inf), -1)}
    _cache[idx] = ((q, k, v, g), got, want)
    return _cache[idx]


@requires_gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_swa_against_fp32_reference(ext, monkeypatch, idx):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    B, H, Hkv, S, D, W, strided = CASES[idx]
    G, tag = H // Hkv, IDS[idx]
    (q, k, v, g), got, want = _case(ext, idx)
    err = {n: float((got[n].float() - want[n]).abs().max()) for n in got}
    print(tag, err)
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), (tag, name, "not finite")
        assert t.shape == want[name].shape, (tag, name)
    assert torch.allclose(got["out"].float(), want["out"],
                          atol=3e-2, rtol=3e-2), (tag, err)
    if W == 1 and G == 1:      # softmax over the one visible key is 1.0
        assert torch.equal(got["out"], v), (tag, "out != v")
    assert torch.allclose(got["lse"], want["lse"], atol=1e-2, rtol=1e-3), \
        (tag, err)
    # dk and dv sum G per-head gradients: G times the per-head bound
    assert err["dq"] < 8e-2 and err["dk"] < G * 8e-2 \
        and err["dv"] < G * 8e-2, (tag, err)


@requires_gpu
@pytest.mark.parametrize("W", [192, 10 ** 6])
def test_window_of_s_or_more_is_plain_causal(ext, monkeypatch, W):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    torch.manual_seed(1300)
    q, k, v, g = _inputs(1, 2, 2, 192, 64, False)
    got, causal = _run(ext, q, k, v, g, W), _run(ext, q, k, v, g)
    for name in ("out", "lse", "dq", "dk", "dv"):
        assert bool(torch.isfinite(got[name]).all()), (name, "not finite")
        assert torch.equal(got[name], causal[name]), (W, name)


@requires_gpu
def test_public_op_runs_the_window_kernels(ext, monkeypatch):
    """The op with the aten math path taken away, on the strided ragged GQA
    case: the tensors of the direct kernel calls."""
    from easydist_amd.ops import attention

    def _no_math(*a, **kw):
        raise AssertionError("aten math path taken at a kernel shape")

    monkeypatch.setattr(attention, "_math_fwd", _no_math)
    monkeypatch.setattr(attention, "_math_bwd", _no_math)
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    B, H, Hkv, S, D, W, strided = CASES[STRIDED_CASE]
    assert strided and Hkv < H and S % 128 != 0
    (q, k, v, g), ker, _ = _case(ext, STRIDED_CASE)
    ql, kl, vl = (t.detach().requires_grad_(True) for t in (q, k, v))
    out = attention.scaled_dot_product_attention(ql, kl, vl, causal=True,
                                                 window=W)
    out.backward(g)
    torch.cuda.synchronize()
    got = {"out": out.detach(), "dq": ql.grad, "dk": kl.grad, "dv": vl.grad}
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), (name, "not finite")
        assert torch.equal(t, ker[name]), name
