"""Flash attention dkv under its two workgroup geometries (EASYDIST_DKV_GEOM).

Geometry 0 is 8 waves on a 128-key block with the full-tile loop; geometry
1 is 4 waves on a 64-key block that walks each 64-column q tile as two
32-column halves.  Every wave meets the same q tiles in the same order and
every accumulator the same operands in the same order, so dk, dv and the
packed buffer must be bit-identical between the two, dq (another kernel)
must not move, and geometry 1 must meet the fp32 SDPA reference within the
bounds of tests/test_gpu_attn_tr.py.  Each case runs with the shipped TR
value of each geometry and with EASYDIST_ATTN_TR=1 forced.

Shapes are the smallest that reach a distinct path of a 64-key block; see
the comment on each case.  As in the TR test: a seed per case, output-sized
NaN-filled tensors allocated and freed right before each call under test,
and the outputs must be finite.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, Hkv, S, D, causal, strided, map)
CASES = [
    # two blocks; block 1 runs a single q tile and uses only buffer 0
    (1, 2, 2, 128, 64, True, False, None),
    # four tiles: buffer 0 is reused
    (2, 3, 3, 256, 64, False, False, None),
    # blocks with different trip counts in one launch
    (2, 3, 3, 384, 64, True, False, None),
    # last block holds one key: three of its four waves wholly out of range
    (1, 2, 2, 65, 64, True, False, None),
    (1, 2, 2, 65, 64, False, False, None),
    # partial last block and partial last q tile
    (1, 2, 2, 200, 64, True, False, None),
    # q, k, v views of one [B,S,3HD] buffer; grad a [B,S,H,D] view
    (2, 3, 3, 256, 64, True, True, None),
    # GQA head switch inside the flat loop
    (1, 4, 2, 192, 64, True, False, None),
    # GQA and ragged together
    (1, 4, 2, 200, 64, True, False, None),
    # B*H not a multiple of 8, under both maps
    (3, 3, 3, 256, 64, True, False, "0"),
    (3, 3, 3, 256, 64, True, False, "1"),
    # D = 128 still correct under the knob
    (1, 2, 2, 256, 128, True, False, None),
]


def _case_id(c):
    B, H, Hkv, S, D, causal, strided, amap = c[1]
    return "B{}H{}k{}S{}D{}{}{}{}".format(
        B, H, Hkv, S, D, "c" if causal else "n", "v" if strided else "",
        "" if amap is None else "m" + amap)


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


def _bwd(ext, q, k, v, g, out, lse, causal):
    B, H, S, D = q.shape
    Hkv = k.shape[1]
    bf, f32 = torch.bfloat16, torch.float32
    _poison(((B, H, S, D), bf), ((B, Hkv, S, D), bf), ((B, Hkv, S, D), bf),
            ((B, H, S), f32))
    dq, dk, dv = ext.flash_attn_bwd(g, q, k, v, out, lse, causal)
    _poison(((B, S, (H + 2 * Hkv) * D), bf), ((B, H, S), f32))
    packed = ext.flash_attn_bwd_pack(g, q, k, v, out, lse, causal)
    torch.cuda.synchronize()
    return {"dq": dq, "dk": dk, "dv": dv, "packed": packed}


def _inputs(B, H, Hkv, S, D, strided):
    bf = torch.bfloat16
    if not strided:
        q = torch.randn(B, H, S, D, device="cuda", dtype=bf)
        k = torch.randn(B, Hkv, S, D, device="cuda", dtype=bf)
        v = torch.randn(B, Hkv, S, D, device="cuda", dtype=bf)
        g = torch.randn(B, H, S, D, device="cuda", dtype=bf)
        return q, k, v, g
    assert H == Hkv
    qkv = torch.randn(B, S, 3 * H * D, device="cuda", dtype=bf)
    q, k, v = (t.view(B, S, H, D).transpose(1, 2)
               for t in qkv.split(H * D, dim=2))
    g = torch.randn(B, S, H * D, device="cuda", dtype=bf) \
        .view(B, S, H, D).transpose(1, 2)
    assert not q.is_contiguous() and not g.is_contiguous()
    return q, k, v, g


@requires_gpu
@pytest.mark.parametrize("case", list(enumerate(CASES)), ids=_case_id)
def test_attn_dkv_geometries(ext, monkeypatch, case):
    idx, (B, H, Hkv, S, D, causal, strided, amap) = case
    torch.manual_seed(900 + idx)
    q, k, v, g = _inputs(B, H, Hkv, S, D, strided)
    if amap is None:
        monkeypatch.delenv("EASYDIST_ATTN_MAP", raising=False)
    else:
        monkeypatch.setenv("EASYDIST_ATTN_MAP", amap)
    monkeypatch.delenv("EASYDIST_ATTN_TR", raising=False)
    monkeypatch.delenv("EASYDIST_DKV_GEOM", raising=False)
    out, lse = ext.flash_attn_fwd(q, k, v, causal)

    # fp32 reference, once per case
    G = H // Hkv
    qf = q.float().contiguous().requires_grad_(True)
    kf = k.float().contiguous().requires_grad_(True)
    vf = v.float().contiguous().requires_grad_(True)
    torch.nn.functional.scaled_dot_product_attention(
        qf, kf.repeat_interleave(G, dim=1), vf.repeat_interleave(G, dim=1),
        is_causal=causal).backward(g.float())
    want = {"dq": qf.grad, "dk": kf.grad, "dv": vf.grad}

    for tr in (None, "1"):          # shipped TR of each geometry, then TR = 1
        if tr is not None:
            monkeypatch.setenv("EASYDIST_ATTN_TR", tr)
        res = {}
        for geom in ("0", "1"):
            monkeypatch.setenv("EASYDIST_DKV_GEOM", geom)
            res[geom] = _bwd(ext, q, k, v, g, out, lse, causal)
        old, new = res["0"], res["1"]
        for name in ("dq", "dk", "dv", "packed"):
            assert bool(torch.isfinite(old[name]).all()), ("geom0", tr, name)
            assert bool(torch.isfinite(new[name]).all()), ("geom1", tr, name)
            # 1. dk, dv and the packed buffer bit-equal; 2. dq unchanged
            diff = float((new[name].float() - old[name].float()).abs().max())
            assert torch.equal(new[name], old[name]), (tr, name, diff)
        ref_packed = torch.cat(
            [new[n].transpose(1, 2).reshape(B, S, -1)
             for n in ("dq", "dk", "dv")], -1)
        assert torch.equal(new["packed"], ref_packed), tr
        # 3. geometry 1 against the fp32 reference
        for name in ("dq", "dk", "dv"):
            e = float((new[name].float() - want[name]).abs().max())
            print(f"tr={tr} {name} max abs err vs fp32: {e:.4g}")
            assert e < 8e-2, (tr, name, e, B, H, Hkv, S, D)


# EASYDIST_DKV_SWAP is read once per process, so the swapped dkv kernel
# gets a process of its own: dk and dv bit-equal between the geometries.
_SWAP_CHILD = r"""
import os, torch
import easydist_amd.ops as ops
ext = ops.load_extension()
assert ext is not None
B, H, S, D = 2, 3, 256, 64
torch.manual_seed(950)
q, k, v, g = (torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
              for _ in range(4))
out, lse = ext.flash_attn_fwd(q, k, v, True)
res = {}
for tr in ("0", "1"):
    for geom in ("0", "1"):
        os.environ["EASYDIST_ATTN_TR"] = tr
        os.environ["EASYDIST_DKV_GEOM"] = geom
        ts = [torch.full((B, H, S, D), float("nan"), device="cuda",
                         dtype=torch.bfloat16) for _ in range(3)]
        torch.cuda.synchronize()
        del ts
        res[tr, geom] = ext.flash_attn_bwd(g, q, k, v, out, lse, True)
        torch.cuda.synchronize()
for tr in ("0", "1"):
    for i, name in ((0, "dq"), (1, "dk"), (2, "dv")):
        a, b = res[tr, "0"][i], res[tr, "1"][i]
        assert bool(torch.isfinite(a).all()), (tr, name)
        assert bool(torch.isfinite(b).all()), (tr, name)
        assert torch.equal(a, b), \
            (tr, name, float((a.float() - b.float()).abs().max()))
qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
torch.nn.functional.scaled_dot_product_attention(
    qf, kf, vf, is_causal=True).backward(g.float())
for i, w in ((1, kf.grad), (2, vf.grad)):
    e = float((res["1", "1"][i].float() - w).abs().max())
    assert e < 8e-2, (i, e)
print("SWAP_GEOM_OK")
"""


@requires_gpu
def test_attn_dkv_geom_swap():
    env = dict(os.environ)
    env["EASYDIST_DKV_SWAP"] = "1"
    env.pop("EASYDIST_ATTN_MAP", None)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _SWAP_CHILD], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SWAP_GEOM_OK" in r.stdout, \
        (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
