"""Sliding-window causal attention off the GPU: the ops, their presets and
the model option (kernels: tests/test_gpu_attn_swa.py)."""
import math

import pytest
import torch
import torch.fx.experimental.proxy_tensor

import easydist_amd.ops  # noqa: F401  (registers the custom ops)
from easydist_amd.ops import attention

ed = torch.ops.easydist_amd
B, H, HKV, S, D, W = 2, 4, 2, 12, 8, 5


def _band(S, W):
    i = torch.arange(S)
    return (i[None, :] <= i[:, None]) & (i[None, :] > i[:, None] - W)


def _qkv(dtype, grad=False):
    torch.manual_seed(7)
    return tuple(torch.randn(B, h, S, D, dtype=dtype, requires_grad=grad)
                 for h in (H, HKV, HKV))


def test_math_path_against_dense_masked_softmax():
    q, k, v = _qkv(torch.float64, grad=True)
    g = torch.randn(B, H, S, D, dtype=torch.float64)
    out = attention.scaled_dot_product_attention(q, k, v, window=W)
    out.backward(g)
    _, lse = ed.flash_attention_swa(q, k, v, W)

    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    G = H // HKV
    s = qr @ kr.repeat_interleave(G, 1).transpose(-1, -2) / math.sqrt(D)
    s = s.masked_fill(~_band(S, W), float("-inf"))
    ref = torch.softmax(s, -1) @ vr.repeat_interleave(G, 1)
    ref.backward(g)
    assert (s[0, 0] > float("-inf")).sum(-1).tolist() == \
        [min(i + 1, W) for i in range(S)]
    # fp64 on both sides; the op's math path computes the scores in fp32
    for got, want in ((out, ref), (lse, torch.logsumexp(s, -1)),
                      (q.grad, qr.grad), (k.grad, kr.grad),
                      (v.grad, vr.grad)):
        assert got.shape == want.shape
        assert torch.allclose(got.double(), want, atol=1e-5, rtol=1e-5)


def test_opcheck():
    q, k, v = _qkv(torch.float32, grad=True)
    torch.library.opcheck(ed.flash_attention_swa.default, (q, k, v, W))
    out, lse = ed.flash_attention_swa(q, k, v, W)
    torch.library.opcheck(
        ed.flash_attention_swa_bwd.default,
        (torch.randn_like(out), q.detach(), k.detach(), v.detach(),
         out.detach(), lse.detach(), W))


def test_errors():
    q, k, v = _qkv(torch.float32)
    for w in (0, -3):
        with pytest.raises(ValueError, match="window"):
            attention.scaled_dot_product_attention(q, k, v, window=w)
        with pytest.raises(ValueError, match="window"):
            ed.flash_attention_swa(q, k, v, w)
        with pytest.raises(ValueError, match="window"):
            ed.flash_attention_swa_bwd(q, q, k, v, q, q[..., 0], w)
    with pytest.raises(ValueError, match="causal"):
        attention.scaled_dot_product_attention(q, k, v, causal=False,
                                               window=W)


@pytest.mark.parametrize("bwd", [False, True])
def test_presets_shard_batch_and_heads_only(bwd):
    from easydist_amd.compiler.preset_propagation import (RUNTIME_REALIZED,
                                                          preset_meta_spmd)
    q, k, v = _qkv(torch.float32)
    out, lse = ed.flash_attention_swa(q, k, v, W)
    op = ed.flash_attention_swa_bwd.default if bwd \
        else ed.flash_attention_swa.default
    args = (torch.randn_like(out), q, k, v, out, lse, W) if bwd \
        else (q, k, v, W)
    assert op not in RUNTIME_REALIZED
    shapes = [tuple(t.shape) for t in args[:-1]]
    ann, combs = preset_meta_spmd(op, shapes, args, {})
    whole = op(*args)
    dims = []
    for sid, comb in combs.items():
        pos = ann.positions_of(sid)
        assert len(pos) == len(shapes)          # every operand shards
        (d,) = {d for _, d in pos}
        dims.append(d)
        halves = [op(*[t.chunk(2, d)[r] for t in args[:-1]], W)
                  for r in range(2)]
        for j, c in enumerate(comb):
            assert torch.allclose(c([h[j] for h in halves]), whole[j],
                                  atol=1e-6)
    assert sorted(dims) == [0, 1]               # never the sequence


def test_gpt_sliding_window_option(monkeypatch):
    from easydist_amd.models.gpt import GPT, GPTConfig
    kw = dict(vocab_size=64, n_layer=2, n_head=2, n_kv_head=1, n_embd=16,
              block_size=16, rope=True)
    torch.manual_seed(3)
    model = GPT(GPTConfig(sliding_window=W, **kw))
    plain = GPT(GPTConfig(**kw))
    plain.load_state_dict(model.state_dict())
    idx = torch.randint(0, 64, (2, 16))
    got = model(idx)
    # sliding_window=None traces to the op it always did, W to the new one
    ops_of = lambda m: [n.target for n in torch.fx.experimental.proxy_tensor
                        .make_fx(m)(idx).graph.nodes if "flash" in str(n.target)]
    assert ops_of(plain) == [ed.flash_attention.default] * 2
    assert ops_of(model) == [ed.flash_attention_swa.default] * 2

    # the same weights with a dense band mask in place of the op
    def dense(q, k, v, causal=True, window=None):
        G = q.shape[1] // k.shape[1]
        return torch.nn.functional.scaled_dot_product_attention(
            q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1),
            attn_mask=_band(q.shape[2], W))
    monkeypatch.setattr(attention, "scaled_dot_product_attention", dense)
    assert torch.allclose(got, plain(idx), atol=1e-5, rtol=1e-5)
    with pytest.raises(NotImplementedError, match="sliding_window"):
        model.enable_sequence_parallel(None)
    with pytest.raises(ValueError, match="sliding_window"):
        GPT(GPTConfig(sliding_window=0, **kw))
