"""Grouped-query attention (Hkv < H) in the flash attention op, on the CPU.

q is [B, H, S, D], k and v are [B, Hkv, S, D] with H = G * Hkv, and query
head h attends K/V head h // G (torch's repeat_interleave convention).
dk and dv have K/V's shape: the group sum is taken in fp32 and rounded once.

The reference is autograd through fp32 SDPA on repeat_interleave'd K/V.
Inputs are bf16 values, so the reference sees exactly what the op sees;
the op's own arithmetic on the CPU is fp32 with P rounded to the value
dtype before P @ V (as in the kernels), which bounds the error below.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import easydist_amd.ops  # noqa: F401  (registers the custom ops)
from easydist_amd.ops import attention

ed = torch.ops.easydist_amd

HEADS = [(4, 2), (4, 1), (6, 3)]
B, S, D = 2, 24, 16


def _inputs(H, Hkv, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, S, D, generator=g).to(torch.bfloat16)
    k = torch.randn(B, Hkv, S, D, generator=g).to(torch.bfloat16)
    v = torch.randn(B, Hkv, S, D, generator=g).to(torch.bfloat16)
    go = torch.randn(B, H, S, D, generator=g).to(torch.bfloat16)
    return tuple(t.to(dtype) for t in (q, k, v, go))


def _reference(q, k, v, go, causal):
    G = q.shape[1] // k.shape[1]
    qf, kf, vf = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    out = F.scaled_dot_product_attention(
        qf, kf.repeat_interleave(G, dim=1), vf.repeat_interleave(G, dim=1),
        is_causal=causal)
    out.backward(go.float())
    s = qf.detach() @ kf.detach().repeat_interleave(G, dim=1).transpose(
        -1, -2) / math.sqrt(D)
    if causal:
        s = s.masked_fill(~torch.ones(S, S, dtype=torch.bool).tril(),
                          float("-inf"))
    return out.detach(), torch.logsumexp(s, -1), qf.grad, kf.grad, vf.grad


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_op_numerics_fp32(H, Hkv, causal):
    # bf16-representable values held in fp32: the op's math is fp32 end to
    # end, so only summation order separates it from the reference
    q, k, v, go = _inputs(H, Hkv, torch.float32, 10 * H + Hkv)
    want = _reference(q, k, v, go, causal)
    out, lse = ed.flash_attention(q, k, v, causal)
    assert out.shape == (B, H, S, D) and lse.shape == (B, H, S)
    dq, dk, dv = ed.flash_attention_bwd(go, q, k, v, out, lse, causal)
    assert dq.shape == q.shape
    assert dk.shape == k.shape == (B, Hkv, S, D)
    assert dv.shape == v.shape
    for name, got, ref in zip(("out", "lse", "dq", "dk", "dv"),
                              (out, lse, dq, dk, dv), want):
        assert torch.allclose(got, ref, rtol=1e-4, atol=1e-5), \
            (name, float((got - ref).abs().max()))
    packed = ed.flash_attention_bwd_pack(go, q, k, v, out, lse, causal)
    assert packed.shape == (B, S, (H + 2 * Hkv) * D)
    cat = torch.cat([t.transpose(1, 2).reshape(B, S, -1)
                     for t in (dq, dk, dv)], dim=-1)
    assert torch.equal(packed, cat)


@pytest.mark.parametrize("H,Hkv", HEADS)
def test_op_numerics_bf16_and_autograd(H, Hkv):
    # bf16 tensors through the public entry: gradients land in leaves of
    # K/V's shape.  Bounds: out is rounded to bf16 once (2^-8 relative) on
    # top of the bf16 P (2^-8 per weight, weights sum to 1, |v| < 5); each
    # gradient is one bf16 rounding of an fp32 sum of magnitude <= ~16.
    q, k, v, go = _inputs(H, Hkv, torch.bfloat16, 20 * H + Hkv)
    want = _reference(q, k, v, go, True)
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = attention.scaled_dot_product_attention(ql, kl, vl, causal=True)
    out.backward(go)
    assert kl.grad.shape == k.shape and vl.grad.shape == v.shape
    assert kl.grad.dtype == torch.bfloat16
    assert torch.allclose(out.float(), want[0], rtol=2 ** -7, atol=4e-2)
    for name, got, ref in (("dq", ql.grad, want[2]), ("dk", kl.grad, want[3]),
                           ("dv", vl.grad, want[4])):
        assert torch.allclose(got.float(), ref, rtol=2 ** -7, atol=2e-2), \
            (name, float((got.float() - ref).abs().max()))


def test_group_sum_is_rounded_once():
    # dv of a single key: S = 1 makes P = 1 exactly, so dv = sum_g grad_g.
    # The two heads of the group carry 1 + 2^-9 and -1: the fp32 sum 2^-9
    # is a bf16 value, while each head rounded to bf16 first (1 and -1)
    # would sum to 0.  grad rides in fp32 to carry the 2^-9.
    go = torch.empty(1, 2, 1, 16, dtype=torch.float32)
    go[:, 0] = 1.0 + 2.0 ** -9
    go[:, 1] = -1.0
    assert float(go.to(torch.bfloat16)[0, 0, 0, 0]) == 1.0
    q = torch.zeros(1, 2, 1, 16)
    k = torch.zeros(1, 1, 1, 16, dtype=torch.bfloat16)
    v = torch.zeros(1, 1, 1, 16, dtype=torch.bfloat16)
    out, lse = attention._math_fwd(q, k, v, True)
    _, _, dv = attention._math_bwd(go, q, k, v, out, lse, True)
    assert dv.dtype == torch.bfloat16 and dv.shape == (1, 1, 1, 16)
    assert float(dv[0, 0, 0, 0]) == 2.0 ** -9


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_non_dividing_head_count_raises(dtype):
    q, _, _, go = _inputs(4, 2, dtype, 1)
    _, k, v, _ = _inputs(3, 3, dtype, 2)
    with pytest.raises((ValueError, RuntimeError), match="heads"):
        ed.flash_attention(q, k, v, True)
    out = torch.zeros_like(q)
    lse = torch.zeros(B, 4, S)
    with pytest.raises((ValueError, RuntimeError), match="heads"):
        ed.flash_attention_bwd(go, q, k, v, out, lse, True)
    with pytest.raises((ValueError, RuntimeError), match="heads"):
        ed.flash_attention_bwd_pack(go, q, k, v, out, lse, True)
    # k and v of different head counts never broadcast either
    with pytest.raises((ValueError, RuntimeError), match="heads"):
        ed.flash_attention(q, k[:, :2], k[:, :1], True)


@pytest.mark.parametrize("H,Hkv", HEADS)
def test_fake_shapes(H, Hkv):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        q = torch.empty(B, H, S, 64, dtype=torch.bfloat16)
        k = torch.empty(B, Hkv, S, 64, dtype=torch.bfloat16)
        v = torch.empty(B, Hkv, S, 64, dtype=torch.bfloat16)
        out, lse = ed.flash_attention(q, k, v, True)
        assert out.shape == (B, H, S, 64) and lse.shape == (B, H, S)
        assert lse.dtype == torch.float32
        dq, dk, dv = ed.flash_attention_bwd(out, q, k, v, out, lse, True)
        assert dq.shape == (B, H, S, 64)
        assert dk.shape == (B, Hkv, S, 64) and dv.shape == (B, Hkv, S, 64)
        packed = ed.flash_attention_bwd_pack(out, q, k, v, out, lse, True)
        assert packed.shape == (B, S, (H + 2 * Hkv) * 64)


def _z(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16)


@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_envelope_inside(H, Hkv, Dh):
    assert attention._kernel_ok(_z(2, H, 33, Dh), _z(2, Hkv, 33, Dh),
                                _z(2, Hkv, 33, Dh))


def test_envelope_outside():
    q = _z(2, 4, 33, 64)
    # head count that does not divide
    assert not attention._kernel_ok(q, _z(2, 3, 33, 64), _z(2, 3, 33, 64))
    assert not attention._kernel_ok(_z(2, 2, 33, 64), _z(2, 4, 33, 64),
                                    _z(2, 4, 33, 64))
    # k and v of different shapes
    assert not attention._kernel_ok(q, _z(2, 2, 33, 64), _z(2, 1, 33, 64))
    assert not attention._kernel_ok(q, _z(2, 2, 33, 64), _z(2, 4, 33, 64))
    # batch, sequence or head dim mismatch
    assert not attention._kernel_ok(q, _z(1, 2, 33, 64), _z(1, 2, 33, 64))
    assert not attention._kernel_ok(q, _z(2, 2, 32, 64), _z(2, 2, 32, 64))
    assert not attention._kernel_ok(q, _z(2, 2, 33, 128), _z(2, 2, 33, 128))
    # dtype of k/v
    assert not attention._kernel_ok(q, _z(2, 2, 33, 64).float(),
                                    _z(2, 2, 33, 64).float())
    # no K/V head at all
    assert not attention._kernel_ok(q, _z(2, 0, 33, 64), _z(2, 0, 33, 64))
