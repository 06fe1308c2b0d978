"""Grouped-query attention (Hkv < H) in the flash attention kernels.

q is [B, H, S, D], k and v are [B, Hkv, S, D], G = H // Hkv, and query head
h attends K/V head h // G.  The GQA instantiations of the forward and dq
kernels differ from the MHA ones in the head of their K/V base pointer
only; the dkv kernel walks the Q/dO tiles of the G query heads of its K/V
head in one loop and sums into the same fp32 accumulators.

Reference for exactness: the MHA kernels on repeat_interleave'd contiguous
K/V.  Per query head the arithmetic is the same instruction sequence, so
out, lse and dq must be bit-identical; dk and dv must equal the sum of the
G per-head bf16 gradients of that run up to bf16 rounding (see
test_gqa_dkv_is_the_group_sum).

Shapes are the smallest that reach each path (see CASES).  As in
tests/test_gpu_attn_ragged.py: a seed per case, output-sized NaN-filled
tensors allocated and freed right before each call under test, all outputs
finite, and ragged inputs as [:, :, :S] views of tensors whose rows
S .. S_pad-1 are NaN.
"""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

# (B, H, Hkv, S, D, causal, strided)
CASES = [
    (2, 2, 1, 128, 64, True, False),   # MQA, one block; b/h split by Hkv
    (2, 4, 2, 256, 64, True, False),   # two key blocks; causal skip across
                                       # a head switch
    (1, 6, 3, 128, 64, False, False),  # G = 2, head count no power of two
    (1, 4, 1, 192, 64, True, False),   # ragged, 3 (then 1) tiles per head:
                                       # buffer parity flips at a switch
    (2, 4, 2, 197, 64, False, True),   # ragged, views of the qkv buffer
    (1, 4, 2, 129, 128, True, False),  # D = 128, second block: one row
]
IDS = ["B{}H{}K{}S{}D{}{}{}".format(*c[:5], "c" if c[5] else "n",
                                    "v" if c[6] else "") for c in CASES]
STRIDED_CASE = 4


@pytest.fixture(scope="module")
def ext():
    import easydist_amd.ops as ops
    e = ops.load_extension()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _pad128(S):
    return (S + 127) // 128 * 128


def _poison(*shapes_dtypes):
    """Allocate, NaN-fill and free tensors of the output sizes so the
    outputs of the next call most likely reuse poisoned memory."""
    ts = [torch.full(s, float("nan"), device="cuda", dtype=dt)
          for s, dt in shapes_dtypes]
    torch.cuda.synchronize()
    del ts


def _run(ext, q, k, v, g, causal):
    B, H, S, D = q.shape
    Hkv = k.shape[1]
    bf, f32 = torch.bfloat16, torch.float32
    _poison(((B, H, S, D), bf), ((B, H, S), f32))
    out, lse = ext.flash_attn_fwd(q, k, v, causal)
    _poison(((B, H, S, D), bf), ((B, Hkv, S, D), bf), ((B, Hkv, S, D), bf),
            ((B, H, S), f32))
    dq, dk, dv = ext.flash_attn_bwd(g, q, k, v, out, lse, causal)
    _poison(((B, S, (H + 2 * Hkv) * D), bf), ((B, H, S), f32))
    packed = ext.flash_attn_bwd_pack(g, q, k, v, out, lse, causal)
    torch.cuda.synchronize()
    return {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv,
            "packed": packed}


def _inputs(B, H, Hkv, S, D, strided):
    """q, g [B, H, S, D] and k, v [B, Hkv, S, D]; where S % 128 != 0 they
    are views whose rows S .. S_pad-1 are NaN."""
    Sp = _pad128(S)
    nan = float("nan")
    bf = torch.bfloat16
    if not strided:
        full = [torch.randn(B, h, Sp, D, device="cuda", dtype=bf)
                for h in (H, Hkv, Hkv, H)]
        for t in full:
            t[:, :, S:] = nan
        views = tuple(t[:, :, :S] for t in full)
    else:
        qkv = torch.randn(B, Sp, (H + 2 * Hkv) * D, device="cuda", dtype=bf)
        gb = torch.randn(B, Sp, H * D, device="cuda", dtype=bf)
        qkv[:, S:] = nan
        gb[:, S:] = nan
        q, k, v = qkv[:, :S].split([H * D, Hkv * D, Hkv * D], dim=2)
        views = (q.view(B, S, H, D).transpose(1, 2),
                 k.view(B, S, Hkv, D).transpose(1, 2),
                 v.view(B, S, Hkv, D).transpose(1, 2),
                 gb[:, :S].view(B, S, H, D).transpose(1, 2))
    for t, h in zip(views, (H, Hkv, Hkv, H)):
        assert t.shape == (B, h, S, D) and t.stride(3) == 1
        assert bool(torch.isfinite(t).all())
    return views


_cache = {}


def _case(ext, idx):
    """Inputs, the GQA results, the MHA results on expanded K/V and the
    fp32 reference of one case, computed once and shared (nothing below
    writes to them)."""
    if idx in _cache:
        return _cache[idx]
    B, H, Hkv, S, D, causal, strided = CASES[idx]
    G = H // Hkv
    torch.manual_seed(900 + idx)
    q, k, v, g = _inputs(B, H, Hkv, S, D, strided)
    got = _run(ext, q, k, v, g, causal)

    ke = k.repeat_interleave(G, dim=1).contiguous()
    ve = v.repeat_interleave(G, dim=1).contiguous()
    assert ke.shape == (B, H, S, D)
    mha = _run(ext, q, ke, ve, g, causal)

    qf = q.float().contiguous().requires_grad_(True)
    kf = k.float().contiguous().requires_grad_(True)
    vf = v.float().contiguous().requires_grad_(True)
    ref = torch.nn.functional.scaled_dot_product_attention(
        qf, kf.repeat_interleave(G, dim=1), vf.repeat_interleave(G, dim=1),
        is_causal=causal)
    ref.backward(g.float())
    s = q.float() @ ke.float().transpose(-1, -2) / math.sqrt(D)
    if causal:
        mask = torch.ones(S, S, device="cuda", dtype=torch.bool).tril()
        s = s.masked_fill(~mask, float("-inf"))
    want = {"out": ref.detach(), "lse": torch.logsumexp(s, -1),
            "dq": qf.grad, "dk": kf.grad, "dv": vf.grad}
    _cache[idx] = ((q, k, v, g), got, mha, want)
    return _cache[idx]


def _clean_env(monkeypatch):
    for name in ("EASYDIST_ATTN_MAP", "EASYDIST_ATTN_TR",
                 "EASYDIST_DKV_SWAP"):
        monkeypatch.delenv(name, raising=False)


@requires_gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_gqa_equals_mha_on_expanded_kv(ext, monkeypatch, idx):
    """out, lse and dq bit for bit; the packed buffer is the cat."""
    _clean_env(monkeypatch)
    B, H, Hkv, S, D, causal, strided = CASES[idx]
    _, got, mha, _ = _case(ext, idx)
    for name, t in list(got.items()) + list(mha.items()):
        assert bool(torch.isfinite(t).all()), (IDS[idx], name, "not finite")
    assert got["out"].shape == (B, H, S, D) and got["out"].is_contiguous()
    assert got["dq"].shape == (B, H, S, D) and got["dq"].is_contiguous()
    assert got["lse"].shape == (B, H, S)
    for name in ("dk", "dv"):
        assert got[name].shape == (B, Hkv, S, D)
        assert got[name].is_contiguous()
    for name in ("out", "lse", "dq"):
        a, b = got[name], mha[name]
        assert torch.equal(a, b), \
            (IDS[idx], name, float((a.float() - b.float()).abs().max()))
    # the packed buffer: dq at column 0, dk at H*D, dv at (H + Hkv)*D
    ref_packed = torch.cat([got[n].transpose(1, 2).reshape(B, S, -1)
                            for n in ("dq", "dk", "dv")], -1)
    assert got["packed"].shape == (B, S, (H + 2 * Hkv) * D)
    assert torch.equal(got["packed"], ref_packed)


@requires_gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_gqa_dkv_is_the_group_sum(ext, monkeypatch, idx):
    """dk and dv against the G per-head bf16 gradients x_g of the MHA run:

        |got - sum_g float(x_g)| <= 2^-7 sum_g |x_g| + 2^-16 max|sum_g x_g|

    elementwise.  First term: bf16 unit roundoff 2^-8, once for rounding
    the fp32 group sum (|sum| <= sum of |.|) and once for the rounding each
    x_g already carries.  Second term: a floor for the fp32 summation
    order (one accumulator over G heads against G accumulators), 256 times
    below a bf16 ulp at the tensor's maximum.  A missing, duplicated or
    mis-indexed head is orders of magnitude outside."""
    _clean_env(monkeypatch)
    B, H, Hkv, S, D, causal, strided = CASES[idx]
    G = H // Hkv
    _, got, mha, _ = _case(ext, idx)
    for name in ("dk", "dv"):
        x = mha[name].float().view(B, Hkv, G, S, D)
        total = x.sum(2)
        bound = 2.0 ** -7 * x.abs().sum(2) + 2.0 ** -16 * total.abs().max()
        err = (got[name].float() - total).abs()
        worst = float((err - bound).max())
        print(IDS[idx], name, "max err", float(err.max()),
              "max (err - bound)", worst,
              "max err / bound", float((err / bound).max()))
        assert bool((err <= bound).all()), (IDS[idx], name, worst)


@requires_gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_gqa_against_fp32_reference(ext, monkeypatch, idx):
    _clean_env(monkeypatch)
    B, H, Hkv, S, D, causal, strided = CASES[idx]
    G = H // Hkv
    tag = IDS[idx]
    _, got, _, want = _case(ext, idx)
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), (tag, name, "not finite")
    err = float((got["out"].float() - want["out"]).abs().max())
    print(tag, "out max-abs err", err)
    assert torch.allclose(got["out"].float(), want["out"],
                          atol=3e-2, rtol=3e-2), (tag, "out", err)
    err = float((got["lse"] - want["lse"]).abs().max())
    print(tag, "lse max-abs err", err)
    assert torch.allclose(got["lse"], want["lse"], atol=1e-2, rtol=1e-3), \
        (tag, "lse", err)
    # dk and dv sum G per-head gradients: G times the per-head bound
    for name, bound in (("dq", 8e-2), ("dk", G * 8e-2), ("dv", G * 8e-2)):
        e = float((got[name].float() - want[name]).abs().max())
        print(tag, name, "max-abs err", e, "bound", bound)
        assert e < bound, (tag, name, e)


@requires_gpu
def test_public_op_runs_the_gqa_kernels(ext, monkeypatch):
    """The custom op on the strided ragged case with the aten math path
    taken away: gradients land in leaves of K/V's shape."""
    from easydist_amd.ops import attention

    def _no_math(*a, **kw):
        raise AssertionError("aten math path taken at a kernel shape")

    monkeypatch.setattr(attention, "_math_fwd", _no_math)
    monkeypatch.setattr(attention, "_math_bwd", _no_math)
    _clean_env(monkeypatch)
    B, H, Hkv, S, D, causal, strided = CASES[STRIDED_CASE]
    assert strided and Hkv < H
    (q, k, v, g), ker, _, want = _case(ext, STRIDED_CASE)
    ql, kl, vl = (t.detach().requires_grad_(True) for t in (q, k, v))
    assert not kl.is_contiguous()
    out = attention.scaled_dot_product_attention(ql, kl, vl, causal=causal)
    out.backward(g)
    torch.cuda.synchronize()
    assert kl.grad.shape == (B, Hkv, S, D) and vl.grad.shape == (B, Hkv, S, D)
    got = {"out": out.detach(), "dq": ql.grad, "dk": kl.grad, "dv": vl.grad}
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), (name, "not finite")
        # the op runs the kernels the direct calls ran
        assert torch.equal(t, ker[name]), name
    assert torch.allclose(got["out"].float(), want["out"],
                          atol=3e-2, rtol=3e-2)


@requires_gpu
def test_gqa_gpt_compiled_runs_flash_kernel():
    """A GPT with 2 query heads on 1 K/V head (D = 64) through the
    auto-SPMD compiler on one GPU: loss as the eager step, and a flash
    kernel in the compiled step."""
    from easydist_amd import easydist_compile, easydist_setup, set_device_mesh
    from easydist_amd.models.gpt import GPT, GPTConfig, gpt_train_step
    from easydist_amd.utils.stream_tracer import trace_kernel_streams
    from easydist_amd.utils.testing import init_single_process

    init_single_process()
    easydist_setup(device="cuda")
    set_device_mesh([0], ["spmd0"])
    torch.manual_seed(21)
    cfg = GPTConfig(vocab_size=256, n_layer=1, n_head=2, n_kv_head=1,
                    n_embd=128, block_size=64)
    model = GPT(cfg).cuda()
    assert model.h[0].attn.c_attn.weight.shape == (256, 128)
    model_ref = copy.deepcopy(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    opt_ref = torch.optim.Adam(model_ref.parameters(), lr=1e-3, fused=True)

    compiled = easydist_compile(gpt_train_step, cuda_graph=False)
    torch.manual_seed(22)
    for _ in range(3):
        idx = torch.randint(0, 256, (4, 64), device="cuda")
        tg = torch.randint(0, 256, (4, 64), device="cuda")
        loss = compiled(model, opt, idx, tg).detach()
        ref = gpt_train_step(model_ref, opt_ref, idx, tg).detach()
        assert abs(float(loss) - float(ref)) < 5e-3, (float(loss), float(ref))

    kernels = trace_kernel_streams(compiled, model, opt, idx, tg)
    assert any("flash" in name for name in kernels), sorted(kernels)
