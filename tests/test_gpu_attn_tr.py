"""Flash attention under the two LDS forms (EASYDIST_ATTN_TR).

TR = 1 keeps one row-major image per staged tile and takes the B operand
of PV, dS K, P^T dO and dS^T Q from it with the hardware transposed read;
TR = 0 builds the second, transposed copy.  Every MFMA sees the same
fragments in the same order, so the two forms must be bit-identical, and
TR = 1 must meet the fp32 SDPA reference within the bounds of
tests/test_gpu_attn_block_map.py.  Shapes are the smallest that reach a
distinct path: one block of two tiles (both LDS buffers, the diagonal
mask), four tiles (buffer 0 reused), causal blocks whose upper waves skip
whole tiles before a transposed read, the 256-byte-row image (D = 128),
and the [B,S,H,D]-layout views of the model.

As in the block-map test: a seed per case, output-sized NaN-filled
tensors allocated and freed right before each call under test, and the
outputs must be finite.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, S, D, causal, strided)
CASES = [
    (1, 2, 128, 64, True, False),    # one block, two tiles, diagonal mask
    (2, 3, 256, 64, False, False),   # four tiles: third reuses buffer 0
    (2, 3, 384, 64, True, False),    # waves skip whole tiles
    (1, 2, 256, 128, True, False),   # 256-byte-row image
    (1, 2, 256, 128, False, False),
    (2, 3, 256, 64, True, True),     # q/k/v split from one qkv, grad view
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


def _inputs(B, H, S, D, strided):
    if not strided:
        return tuple(torch.randn(B, H, S, D, device="cuda",
                                 dtype=torch.bfloat16) for _ in range(4))
    qkv = torch.randn(B, S, 3 * H * D, device="cuda", dtype=torch.bfloat16)
    q, k, v = (t.view(B, S, H, D).transpose(1, 2)
               for t in qkv.split(H * D, dim=2))
    g = torch.randn(B, S, H * D, device="cuda", dtype=torch.bfloat16) \
        .view(B, S, H, D).transpose(1, 2)
    assert not q.is_contiguous() and not g.is_contiguous()
    return q, k, v, g


@requires_gpu
@pytest.mark.parametrize("case", list(enumerate(CASES)),
                         ids=lambda c: "B{}H{}S{}D{}{}{}".format(
                             *c[1][:4], "c" if c[1][4] else "n",
                             "v" if c[1][5] else ""))
def test_attn_tr_forms(ext, monkeypatch, case):
    idx, (B, H, S, D, causal, strided) = case
    torch.manual_seed(600 + idx)
    q, k, v, g = _inputs(B, H, S, D, strided)
    monkeypatch.delenv("EASYDIST_ATTN_MAP", raising=False)

    monkeypatch.setenv("EASYDIST_ATTN_TR", "0")
    two = _run(ext, q, k, v, g, causal)
    monkeypatch.setenv("EASYDIST_ATTN_TR", "1")
    one = _run(ext, q, k, v, g, causal)

    for name, t in one.items():
        assert bool(torch.isfinite(t).all()), ("tr1", name)
        assert bool(torch.isfinite(two[name]).all()), ("tr0", name)
        # 1. bit equality between the two forms
        assert torch.equal(t, two[name]), \
            (name, float((t.float() - two[name].float()).abs().max()))

    # the packed buffer holds the same dq/dk/dv
    ref_packed = torch.cat([one[n].transpose(1, 2).reshape(B, S, H * D)
                            for n in ("dq", "dk", "dv")], -1)
    assert torch.equal(one["packed"], ref_packed)

    # 2. TR = 1 against the fp32 reference
    qf = q.float().contiguous().requires_grad_(True)
    kf = k.float().contiguous().requires_grad_(True)
    vf = v.float().contiguous().requires_grad_(True)
    ref = torch.nn.functional.scaled_dot_product_attention(
        qf, kf, vf, is_causal=causal)
    ref.backward(g.float())
    ref = ref.detach()
    err = float((one["out"].float() - ref).abs().max())
    assert torch.allclose(one["out"].float(), ref, atol=3e-2, rtol=3e-2), \
        ("out", err)
    s = q.float() @ k.float().transpose(-1, -2) / math.sqrt(D)
    if causal:
        mask = torch.ones(S, S, device="cuda", dtype=torch.bool).tril()
        s = s.masked_fill(~mask, float("-inf"))
    lref = torch.logsumexp(s, -1)
    assert torch.allclose(one["lse"], lref, atol=1e-2, rtol=1e-3), \
        ("lse", float((one["lse"] - lref).abs().max()))
    for name, want in (("dq", qf.grad), ("dk", kf.grad), ("dv", vf.grad)):
        e = float((one[name].float() - want).abs().max())
        assert e < 8e-2, (name, e, B, H, S, D)


# EASYDIST_DKV_SWAP is read once per process, so the swapped dkv kernel
# gets a process of its own: dk and dv bit-equal between the TR values.
_SWAP_CHILD = r"""
import os, torch
import easydist_amd.ops as ops
ext = ops.load_extension()
assert ext is not None
B, H, S, D = 2, 3, 256, 64
torch.manual_seed(650)
q, k, v, g = (torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
              for _ in range(4))
res = {}
for tr in ("0", "1"):
    os.environ["EASYDIST_ATTN_TR"] = tr
    out, lse = ext.flash_attn_fwd(q, k, v, True)
    ts = [torch.full((B, H, S, D), float("nan"), device="cuda",
                     dtype=torch.bfloat16) for _ in range(3)]
    torch.cuda.synchronize()
    del ts
    res[tr] = ext.flash_attn_bwd(g, q, k, v, out, lse, True)
    torch.cuda.synchronize()
for i, name in ((1, "dk"), (2, "dv")):
    a, b = res["0"][i], res["1"][i]
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), name
    assert torch.equal(a, b), (name, float((a.float() - b.float()).abs().max()))
qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
torch.nn.functional.scaled_dot_product_attention(
    qf, kf, vf, is_causal=True).backward(g.float())
for i, w in ((1, kf.grad), (2, vf.grad)):
    e = float((res["1"][i].float() - w).abs().max())
    assert e < 8e-2, (i, e)
print("SWAP_TR_OK")
"""


@requires_gpu
def test_attn_tr_dkv_swap():
    env = dict(os.environ)
    env["EASYDIST_DKV_SWAP"] = "1"
    env.pop("EASYDIST_ATTN_MAP", None)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _SWAP_CHILD], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SWAP_TR_OK" in r.stdout, \
        (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
