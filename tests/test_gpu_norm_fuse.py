"""Residual-fused LayerNorm kernels against the kernels they replace.

add_layer_norm_fwd must be bit-equal to aten's bf16 add followed by
layer_norm_fwd; layer_norm_bwd_res must give the dx of the
EASYDIST_NORM_FUSE=0 pair (norm_bwd + param_grads) followed by aten's add,
bit for bit. dw/db are the same fp32 terms summed in another order: they
are held to the bounds of test_layer_norm_bwd and to twice the old
kernel's error against an fp64 sum.

Shapes: D 64 (8 active lanes), 768 (second vector step half filled), 776
(97 vectors), 1024 (exactly two steps), 2048 (the register cap), 2056
(first D on the unfused fall-back); rows 1, 7, 1027 (no multiple of the 4
waves of a block) and 5000 (more rows than waves in the grid).
"""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

DIMS = (64, 768, 776, 1024, 2048, 2056)
ROWS = (1, 7, 1027, 5000)
MAX_FUSED_D = 2048
EPS = 1e-5


@pytest.fixture(scope="module")
def ext():
    import easydist_amd.ops as ops
    e = ops.load_extension()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _case(rows, D):
    """Seeded inputs, the unfused results and the references, made once
    per shape and shared (read-only) by the tests below."""
    import easydist_amd.ops as ops
    e = ops.load_extension()
    gen = torch.Generator(device="cuda").manual_seed(1000 * D + rows)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=gen).bfloat16()
    c = dict(a=rnd(rows, D), b=rnd(rows, D), grad=rnd(rows, D),
             res=rnd(rows, D), w=rnd(D), bias=rnd(D))
    c["x"] = c["a"] + c["b"]
    c["fwd"] = e.layer_norm_fwd(c["x"], c["w"], c["bias"], EPS)
    c["fwd_plain"] = e.layer_norm_fwd(c["x"], None, None, EPS)
    _, mean, rstd = c["fwd"]
    with _env(EASYDIST_NORM_FUSE="0"):
        c["old"] = e.layer_norm_bwd(c["grad"], c["x"], mean, rstd, c["w"],
                                    [True, True, True])
        c["old_plain"] = e.layer_norm_bwd(c["grad"], c["x"], mean, rstd,
                                          None, [True, True, True])
    # fp32 autograd reference, as in test_layer_norm_bwd
    x32 = c["x"].float().requires_grad_()
    w32 = c["w"].float().requires_grad_()
    b32 = c["bias"].float().requires_grad_()
    torch.nn.functional.layer_norm(x32, (D,), w32, b32, EPS).backward(
        c["grad"].float())
    c["dw32"], c["db32"] = w32.grad, b32.grad
    # fp64 sums of the terms the kernels add, from the same inputs
    g64 = c["grad"].double().cpu()
    xh64 = (c["x"].double().cpu() - mean.double().cpu()) * rstd.double().cpu()
    c["dw64"], c["db64"] = (g64 * xh64).sum(0), g64.sum(0)
    return c


def _err(t, ref64):
    return float((t.double().cpu() - ref64).abs().max())


@requires_gpu
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("rows", ROWS)
def test_add_layer_norm_fwd_bit_equal(ext, rows, D):
    c = _case(rows, D)
    for key, w, bias in (("fwd", c["w"], c["bias"]),
                         ("fwd_plain", None, None)):
        s, out, mean, rstd = ext.add_layer_norm_fwd(c["a"], c["b"], w, bias,
                                                    EPS)
        ref_out, ref_mean, ref_rstd = c[key]
        assert torch.equal(s, c["x"])
        assert torch.equal(out, ref_out)
        assert torch.equal(mean, ref_mean)
        assert torch.equal(rstd, ref_rstd)


@requires_gpu
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("rows", ROWS)
def test_layer_norm_bwd_res(ext, rows, D):
    c = _case(rows, D)
    _, mean, rstd = c["fwd"]
    old_dx, old_dw, old_db = c["old"]
    args = (c["grad"], c["x"], mean, rstd, c["w"])

    dx, dw, db = ext.layer_norm_bwd(*args, [True, True, True])
    assert torch.equal(dx, old_dx)
    dxr, dwr, dbr = ext.layer_norm_bwd_res(*args, c["res"],
                                           [True, True, True])
    assert torch.equal(dxr, old_dx + c["res"])

    # no weight; mask entries false (the kernels compute all three anyway)
    dxp, _, _ = ext.layer_norm_bwd_res(*args[:4], None, c["res"],
                                       [True, True, True])
    assert torch.equal(dxp, c["old_plain"][0] + c["res"])
    for mask in ([True, False, False], [False, True, True]):
        with _env(EASYDIST_NORM_FUSE="0"):
            mo = ext.layer_norm_bwd(*args, mask)
        mn = ext.layer_norm_bwd_res(*args, c["res"], mask)
        assert torch.equal(mn[0], mo[0] + c["res"])
        if D <= MAX_FUSED_D:    # the old atomic sums vary from call to call
            assert torch.equal(mn[1], dwr) and torch.equal(mn[2], dbr)

    # the residual changes nothing about dw/db
    assert dw.dtype == torch.float32 and db.dtype == torch.float32
    if D <= MAX_FUSED_D:
        # fixed-order partials: identical from call to call (above
        # MAX_FUSED_D the wrapper runs the old atomic kernels)
        assert torch.equal(dw, dwr) and torch.equal(db, dbr)
        dw2, db2 = ext.layer_norm_bwd(*args, [True, True, True])[1:]
        assert torch.equal(dw, dw2) and torch.equal(db, db2)

    assert torch.allclose(dw, c["dw32"], atol=1.0, rtol=5e-2)
    assert torch.allclose(db, c["db32"], atol=1.0, rtol=5e-2)
    errs = dict(dw_old=_err(old_dw, c["dw64"]), dw_new=_err(dw, c["dw64"]),
                db_old=_err(old_db, c["db64"]), db_new=_err(db, c["db64"]))
    print(f"rows {rows} D {D}: " + " ".join(f"{k} {v:.3e}"
                                             for k, v in errs.items()))
    assert errs["dw_new"] <= 2 * errs["dw_old"], errs
    assert errs["db_new"] <= 2 * errs["db_old"], errs


@requires_gpu
def test_layer_norm_bwd_res_few_blocks(ext):
    """Two blocks for 1027 rows: every wave walks ~128 rows."""
    c = _case(1027, 768)
    _, mean, rstd = c["fwd"]
    with _env(EASYDIST_NORM_BWD_BLOCKS="2"):
        dx, dw, db = ext.layer_norm_bwd_res(c["grad"], c["x"], mean, rstd,
                                            c["w"], c["res"],
                                            [True, True, True])
    assert torch.equal(dx, c["old"][0] + c["res"])
    assert torch.allclose(dw, c["dw32"], atol=1.0, rtol=5e-2)
    assert torch.allclose(db, c["db32"], atol=1.0, rtol=5e-2)
    assert _err(dw, c["dw64"]) <= 2 * _err(c["old"][1], c["dw64"])
    assert _err(db, c["db64"]) <= 2 * _err(c["old"][2], c["db64"])
