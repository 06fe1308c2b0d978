"""Document-masked causal attention off the GPU: the bounds, the ops, their
presets and the model option (kernels: tests/test_gpu_attn_doc.py)."""
import pytest
import torch
from torch.fx.experimental.proxy_tensor import make_fx

import easydist_amd.ops  # noqa: F401  (registers the custom ops)
from easydist_amd.models.gpt import GPT, GPTConfig
from easydist_amd.ops import attention

ed = torch.ops.easydist_amd
B, H, HKV, S, D = 2, 4, 2, 12, 8
# row 1 repeats id 0 at both ends: two documents, not one
IDS = torch.tensor([[7, 7, 7, 7, 7, 2, 2, 9, 9, 9, 9, 9],
                    [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0]])
LO, HI = attention.document_bounds(IDS)


def _qkv(grad=False):
    torch.manual_seed(7)
    return tuple(torch.randn(B, h, S, D, requires_grad=grad)
                 for h in (H, HKV, HKV))


def test_document_bounds():
    assert LO.dtype == HI.dtype == torch.int32
    assert LO.tolist() == [[0] * 5 + [5] * 2 + [7] * 5, [0] + [1] * 10 + [11]]
    assert HI.tolist() == [[5] * 5 + [7] * 2 + [12] * 5,
                           [1] + [11] * 10 + [12]]


def test_math_path_against_dense_mask_sdpa():
    q, k, v = _qkv(grad=True)
    g = torch.randn(B, H, S, D)
    attention.scaled_dot_product_attention(
        q, k, v, doc_bounds=(LO, HI)).backward(g)
    out, lse = ed.flash_attention_doc(q, k, v, LO, HI)
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ke, ve = (t.repeat_interleave(H // HKV, 1) for t in (kr, vr))
    mask = (IDS[:, :, None] == IDS[:, None, :]).tril()[:, None].clone()
    mask[1, :, 11, 0] = False
    ref = torch.nn.functional.scaled_dot_product_attention(
        qr, ke, ve, attn_mask=mask)
    ref.backward(g)
    s = (qr @ ke.transpose(-1, -2) / D ** 0.5).masked_fill(~mask, -1e30)
    for got, want in ((out, ref), (lse, torch.logsumexp(s, -1)),
                      (q.grad, qr.grad), (k.grad, kr.grad), (v.grad, vr.grad)):
        assert got.shape == want.shape
        assert torch.allclose(got, want, atol=1e-5, rtol=1e-5)


def test_opcheck():
    q, k, v = _qkv(grad=True)
    torch.library.opcheck(ed.flash_attention_doc.default, (q, k, v, LO, HI))
    out, lse = ed.flash_attention_doc(q, k, v, LO, HI)
    torch.library.opcheck(
        ed.flash_attention_doc_bwd.default,
        (torch.randn_like(out), q.detach(), k.detach(), v.detach(),
         out.detach(), lse.detach(), LO, HI))


def test_errors():
    q, k, v = _qkv()
    sdpa = attention.scaled_dot_product_attention
    with pytest.raises(ValueError, match="causal"):
        sdpa(q, k, v, causal=False, doc_bounds=(LO, HI))
    with pytest.raises(ValueError, match="window"):
        sdpa(q, k, v, window=4, doc_bounds=(LO, HI))
    for lo, hi in ((LO.long(), HI), (LO, HI[:, :-1])):
        with pytest.raises(ValueError, match="int32"):
            ed.flash_attention_doc(q, k, v, lo, hi)
    kw = dict(vocab_size=64, n_layer=1, n_head=2, n_embd=16, block_size=S)
    with pytest.raises(NotImplementedError, match="sliding_window"):
        GPT(GPTConfig(sliding_window=4, **kw))(IDS, doc_ids=IDS)
    sp = GPT(GPTConfig(**kw))
    sp._sp_group, sp._sp_rank = object(), 0
    with pytest.raises(NotImplementedError, match="sequence parallelism"):
        sp(IDS, doc_ids=IDS)


@pytest.mark.parametrize("bwd", [False, True])
def test_presets_shard_batch_and_heads_only(bwd):
    from easydist_amd.compiler.preset_propagation import (RUNTIME_REALIZED,
                                                          preset_meta_spmd)
    q, k, v = _qkv()
    out, lse = ed.flash_attention_doc(q, k, v, LO, HI)
    op = ed.flash_attention_doc_bwd.default if bwd \
        else ed.flash_attention_doc.default
    args = (torch.randn_like(out), q, k, v, out, lse, LO, HI) if bwd \
        else (q, k, v, LO, HI)
    assert op not in RUNTIME_REALIZED
    ann, combs = preset_meta_spmd(op, [tuple(t.shape) for t in args], args,
                                  {})
    whole = op(*args)
    dims = []
    for sid, comb in combs.items():
        pos = dict(ann.positions_of(sid))
        (d,) = set(pos.values())
        dims.append(d)
        # the bounds shard with the batch only; everything else always
        assert sorted(pos) == list(range(len(args) - (0 if d == 0 else 2)))
        halves = [op(*[t.chunk(2, d)[r] if i in pos else t
                       for i, t in enumerate(args)]) for r in range(2)]
        for j, c in enumerate(comb):
            assert torch.allclose(c([h[j] for h in halves]), whole[j],
                                  atol=1e-6)
    assert sorted(dims) == [0, 1]               # never the sequence


@pytest.mark.parametrize("rope", [False, True])
def test_gpt_packed_row_equals_documents_alone(rope):
    torch.manual_seed(3)
    model = GPT(GPTConfig(vocab_size=64, n_layer=2, n_head=2, n_kv_head=1,
                          n_embd=16, block_size=16, rope=rope))
    idx = torch.randint(0, 64, (1, 16))
    doc_ids = torch.tensor([[4] * 7 + [5] * 9])
    packed = model(idx, doc_ids=doc_ids)
    alone = torch.cat([model(idx[:, :7]), model(idx[:, 7:])], dim=1)
    # wpe positions restart per document; rope's do not and need not, its
    # scores depend on i - j only.  atol: fp32 matmul reordering
    assert torch.allclose(packed, alone, atol=1e-5)
    assert not torch.allclose(packed, model(idx), atol=1e-5)
    flash = lambda *a: [n.target for n in make_fx(model)(*a).graph.nodes
                        if "flash" in str(n.target)]
    assert flash(idx) == [ed.flash_attention.default] * 2
    assert flash(idx, doc_ids) == [ed.flash_attention_doc.default] * 2
