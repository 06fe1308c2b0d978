"""Flash attention at sequence lengths that are no multiple of 128.

S % 128 != 0 runs the RAGGED instantiations of the forward, dq and dkv
kernels: the same tile walk and per-element arithmetic as the aligned
kernels, with the row index of every global load clamped to S - 1 and
ceiling grids.

Over-read detection: every input is a [:, :, :S, :] view of a tensor that
holds S rounded up to 128 rows, the padding rows NaN.  The row stride is
that of the padded tensor, so a kernel that reads and uses a row >= S
yields NaN and fails the finiteness check without leaving allocated
memory.  The strided cases do the same on the [B, S_pad, 3*H*D] qkv buffer
of the models.

Shapes are the smallest that reach each tail path (see CASES).  Bounds are
those of tests/test_gpu_attn_tr.py.  As there: a seed per case,
output-sized NaN-filled tensors allocated and freed right before each call
under test, and all outputs finite.

Pad equivalence (causal cases): the aligned kernels on the inputs padded
to the next multiple of 128 (random finite q/k/v rows, zero grad rows)
must give bit-identical rows < S.  Under the causal mask rows < S never
see keys >= S, and zero grad rows add exact zeros to dk and dv.
"""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

# (B, H, S, D, causal, strided)
CASES = [
    (1, 1, 1, 64, True, False),      # one row, one key
    (1, 2, 63, 64, False, False),    # one partial tile; S % 4, S % 8 != 0
    (2, 2, 65, 64, True, False),     # second tile: one key; wave 4: one row
    (2, 3, 197, 64, False, True),    # ViT: 69-row block, 5-key tile, odd lse
    (1, 2, 129, 128, True, False),   # 256-byte rows; second block: one row
    (1, 2, 200, 128, False, False),  # D = 128 partial tile, full mask
    (2, 3, 320, 64, True, True),     # S % 64 == 0: waves 4-7 of block 2 empty
]
IDS = ["B{}H{}S{}D{}{}{}".format(*c[:4], "c" if c[4] else "n",
                                 "v" if c[5] else "") for c in CASES]
CAUSAL = [i for i, c in enumerate(CASES) if c[4]]
VIT_CASE = 3


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


def _inputs(B, H, S, D, strided):
    """q, k, v, g as [B, H, S, D] views whose rows S .. S_pad-1 are NaN."""
    Sp = _pad128(S)
    nan = float("nan")
    if not strided:
        full = [torch.randn(B, H, Sp, D, device="cuda", dtype=torch.bfloat16)
                for _ in range(4)]
        for t in full:
            t[:, :, S:] = nan
        views = tuple(t[:, :, :S] for t in full)
    else:
        qkv = torch.randn(B, Sp, 3 * H * D, device="cuda",
                          dtype=torch.bfloat16)
        gb = torch.randn(B, Sp, H * D, device="cuda", dtype=torch.bfloat16)
        qkv[:, S:] = nan
        gb[:, S:] = nan
        q, k, v = (t.view(B, S, H, D).transpose(1, 2)
                   for t in qkv[:, :S].split(H * D, dim=2))
        views = (q, k, v, gb[:, :S].view(B, S, H, D).transpose(1, 2))
    for t in views:
        assert t.shape == (B, H, S, D) and t.stride(3) == 1
        # a view: the padded tensor's NaN rows lie behind row S - 1
        assert t.untyped_storage().nbytes() >= 2 * B * H * Sp * D
        assert bool(torch.isfinite(t).all())
    return views


_cache = {}


def _case(ext, idx):
    """Inputs, kernel results and the fp32 reference of one case, computed
    once and shared (nothing below writes to them)."""
    if idx in _cache:
        return _cache[idx]
    B, H, S, D, causal, strided = CASES[idx]
    torch.manual_seed(700 + idx)
    q, k, v, g = _inputs(B, H, S, D, strided)
    got = _run(ext, q, k, v, g, causal)

    qf = q.float().contiguous().requires_grad_(True)
    kf = k.float().contiguous().requires_grad_(True)
    vf = v.float().contiguous().requires_grad_(True)
    ref = torch.nn.functional.scaled_dot_product_attention(
        qf, kf, vf, is_causal=causal)
    ref.backward(g.float())
    s = q.float() @ k.float().transpose(-1, -2) / math.sqrt(D)
    if causal:
        mask = torch.ones(S, S, device="cuda", dtype=torch.bool).tril()
        s = s.masked_fill(~mask, float("-inf"))
    want = {"out": ref.detach(), "lse": torch.logsumexp(s, -1),
            "dq": qf.grad, "dk": kf.grad, "dv": vf.grad}
    _cache[idx] = ((q, k, v, g), got, want)
    return _cache[idx]


def _check_against_reference(got, want, tag):
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
    for name in ("dq", "dk", "dv"):
        e = float((got[name].float() - want[name]).abs().max())
        print(tag, name, "max-abs err", e)
        assert e < 8e-2, (tag, name, e)


@requires_gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_ragged_against_reference(ext, monkeypatch, idx):
    monkeypatch.delenv("EASYDIST_ATTN_MAP", raising=False)
    monkeypatch.delenv("EASYDIST_ATTN_TR", raising=False)
    B, H, S, D, causal, strided = CASES[idx]
    _, got, want = _case(ext, idx)
    for name in ("out", "dq", "dk", "dv"):
        assert got[name].shape == (B, H, S, D) and got[name].is_contiguous()
    assert got["lse"].shape == (B, H, S)
    _check_against_reference(got, want, IDS[idx])
    # the packed buffer holds the same three gradients, bit for bit
    ref_packed = torch.cat([got[n].transpose(1, 2).reshape(B, S, H * D)
                            for n in ("dq", "dk", "dv")], -1)
    assert got["packed"].shape == (B, S, 3 * H * D)
    assert torch.equal(got["packed"], ref_packed)


@requires_gpu
@pytest.mark.parametrize("idx", CAUSAL, ids=[IDS[i] for i in CAUSAL])
def test_ragged_equals_padded_aligned(ext, monkeypatch, idx):
    monkeypatch.delenv("EASYDIST_ATTN_MAP", raising=False)
    monkeypatch.delenv("EASYDIST_ATTN_TR", raising=False)
    B, H, S, D, causal, strided = CASES[idx]
    assert causal
    (q, k, v, g), got, _ = _case(ext, idx)
    Sp = _pad128(S)
    gen = torch.Generator(device="cuda").manual_seed(800 + idx)
    padded = []
    for t in (q, k, v):
        p = torch.randn(B, H, Sp, D, device="cuda", dtype=torch.bfloat16,
                        generator=gen)
        p[:, :, :S] = t
        padded.append(p)
    gp = torch.zeros(B, H, Sp, D, device="cuda", dtype=torch.bfloat16)
    gp[:, :, :S] = g
    pad = _run(ext, *padded, gp, True)
    for name in ("out", "lse", "dq", "dk", "dv"):
        a, b = got[name], pad[name][:, :, :S]
        assert bool(torch.isfinite(pad[name]).all()), (name, "padded run")
        assert torch.equal(a, b), \
            (name, float((a.float() - b.float()).abs().max()))


@requires_gpu
def test_public_op_runs_the_kernels_at_vit_length(ext, monkeypatch):
    """The custom op at S = 197 with the aten math path taken away."""
    from easydist_amd.ops import attention

    def _no_math(*a, **kw):
        raise AssertionError("aten math path taken at a kernel shape")

    monkeypatch.setattr(attention, "_math_fwd", _no_math)
    monkeypatch.setattr(attention, "_math_bwd", _no_math)
    monkeypatch.delenv("EASYDIST_ATTN_MAP", raising=False)
    monkeypatch.delenv("EASYDIST_ATTN_TR", raising=False)
    B, H, S, D, causal, strided = CASES[VIT_CASE]
    assert S == 197 and strided and not causal
    (q, k, v, g), _, want = _case(ext, VIT_CASE)
    # leaves that keep the strided views' layout and storage
    ql, kl, vl = (t.detach().requires_grad_(True) for t in (q, k, v))
    assert not ql.is_contiguous()
    out = attention.scaled_dot_product_attention(ql, kl, vl, causal=False)
    out.backward(g)
    torch.cuda.synchronize()
    got = {"out": out.detach(), "dq": ql.grad, "dk": kl.grad, "dv": vl.grad}
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), (name, "not finite")
    assert torch.allclose(got["out"].float(), want["out"],
                          atol=3e-2, rtol=3e-2)
    for name in ("dq", "dk", "dv"):
        e = float((got[name].float() - want[name]).abs().max())
        assert e < 8e-2, (name, e)


@requires_gpu
def test_vit_compiled_runs_flash_kernel():
    """ViT at S = 17, D = 64 through the auto-SPMD compiler on one GPU:
    loss as the eager step, and a flash kernel in the compiled step."""
    from easydist_amd import easydist_compile, easydist_setup, set_device_mesh
    from easydist_amd.models.vit import ViT, ViTConfig, vit_train_step
    from easydist_amd.utils.stream_tracer import trace_kernel_streams
    from easydist_amd.utils.testing import init_single_process

    init_single_process()
    easydist_setup(device="cuda")
    set_device_mesh([0], ["spmd0"])
    torch.manual_seed(11)
    cfg = ViTConfig(image_size=32, patch_size=8, n_layer=1, n_head=1,
                    n_embd=64, n_classes=10)
    model = ViT(cfg).cuda()
    model_ref = copy.deepcopy(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    opt_ref = torch.optim.Adam(model_ref.parameters(), lr=1e-3, fused=True)

    compiled = easydist_compile(vit_train_step, cuda_graph=False)
    torch.manual_seed(12)
    for _ in range(3):
        x = torch.randn(4, 3, 32, 32, device="cuda")
        y = torch.randint(0, 10, (4,), device="cuda")
        loss = compiled(model, opt, x, y).detach()
        ref = vit_train_step(model_ref, opt_ref, x, y).detach()
        assert abs(float(loss) - float(ref)) < 5e-3, (float(loss), float(ref))

    kernels = trace_kernel_streams(compiled, model, opt, x, y)
    assert any("flash" in name for name in kernels), sorted(kernels)
