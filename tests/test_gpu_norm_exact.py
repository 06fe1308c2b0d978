"""LayerNorm / RMSNorm kernels against fp64 references of the same operation.

The references are plain torch in fp64 (on the device), from the rounded
inputs the kernel sees. The backward tests compute mean/rstd in fp64 from x,
round them to fp32, hand those to the kernel and use them, upcast, in the
reference: a forward error can neither hide nor fake a backward one.

Grid. Every D of {8, 64, 512, 520, 776, 1024, 2048, 2056, 4096} (one lane; a
partial wave; each NV boundary of the register kernels and the value just
past it; the last fused D and the first unfused one; several trips of the
strided loop) and every row count appear for every kernel:
  forward  (7, 8) (1027, 64) (1, 512) (7, 520) (1027, 776) (1, 1024)
           (7, 2048) (1027, 2048) (7, 2056) (1, 4096) (1027, 4096)
  backward (5000, 8) (1027, 64) (7, 512) (1, 520) (5000, 776) (1027, 1024)
           (1, 2048) (5000, 2048) (7, 2056) (5000, 2056) (1027, 4096)
5000 rows are more than the waves of the fused backward's capped grid.

Input families (forward): randn; offset rows off_r + s * randn, off_r cycling
through (0, 16, 64), s = 0.5 in bf16 and (0, 100, 1000), s = 1 in fp32;
constant rows (variance exactly 0; the constants 3.25, -0.5 and 100 and all
their partial sums are exact in fp32, so out must be the bias itself);
1e-3 * randn (eps = 1e-5 dominates the variance); one-hot rows, a single
1000 at column 0, D - 1 or the last column of the first vector step (511 in
bf16, 255 in fp32), cycling by row. Backward: x from randn and offset, grad
randn or a single nonzero in the last row's last column.

Bounds (u16 = 2^-8, one bf16 ulp relative; u32 = 2^-24; all terms fp64):
  mean, rstd   relative error <= max(4 * err_aten, 4e-6), err_aten being the
      error of aten's fp32 native_layer_norm (for RMS: of _rms_fwd_aten in
      fp32) on the same inputs, measured in the test. 4 covers another,
      equally sound summation order over at most 4096 terms, the floor the
      cases where aten is exact. On zero-mean rows the error of the mean is
      taken relative to the row's max|x|.
  out bf16     |out - ref| <= u16 |ref| + 1e-5 (|xhat w| + |b|)
  out fp32     the same with 16 u32 for u16, plus the mean/rstd bound
      propagated through xhat: |w| (rstd dmean + |xhat| drstd/rstd)
  dx           |dx - ref| <= k u16 |ref| + 1e-5 r (|gw| + |mean(gw)| +
      |xhat mean(gw xhat)|); with a residual the result is rounded twice,
      at |dx_ref| and at |dx_ref + res|
  dw, db       within (rows + 8) u32 sum_r |g xhat| (resp. sum_r |g|) of the
      fp64 column sum: any fp32 summation order plus the rounding of each
      term, about rows/8 times less than one dropped row.

The bf16 `out` bound has no term for the statistics' error: without weight
and bias it is purely relative to |xhat|, and small-bf16-1027x4096 has an
element within 1e-7 sigma of its row's mean. An fp32 row sum leaves 1e-9 of
error in xhat there (err / bound 2.1); the bf16 kernels therefore take the
row sum in fp64 and subtract the mean as an fp32 pair.
"""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

U16, U32 = 2.0 ** -8, 2.0 ** -24
EPS = 1e-5
STAT_FACTOR, STAT_FLOOR = 4.0, 4e-6
FWD_SHAPES = ((7, 8), (1027, 64), (1, 512), (7, 520), (1027, 776), (1, 1024),
              (7, 2048), (1027, 2048), (7, 2056), (1, 4096), (1027, 4096))
BWD_SHAPES = ((5000, 8), (1027, 64), (7, 512), (1, 520), (5000, 776),
              (1027, 1024), (1, 2048), (5000, 2048), (7, 2056), (5000, 2056),
              (1027, 4096))
FAMILIES = ("randn", "offset", "const", "small", "onehot")
DTYPES = (torch.bfloat16, torch.float32)
_ids = lambda s: f"{s[0]}x{s[1]}"
_dt = lambda d: "bf16" if d == torch.bfloat16 else "fp32"


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


def _rows(family, dtype, rows, D, gen):
    """x [rows, D] in dtype and zero_mean [rows, 1] (rows whose mean error
    is measured against max|x|)."""
    bf = dtype == torch.bfloat16
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    r = torch.arange(rows, device="cuda")
    zero_mean = torch.zeros(rows, 1, dtype=torch.bool, device="cuda")
    if family == "randn":
        x, zero_mean = rn(rows, D), ~zero_mean
    elif family == "offset":
        offs = torch.tensor((0., 16., 64.) if bf else (0., 100., 1000.),
                            device="cuda")[r % 3].unsqueeze(1)
        x = offs + (0.5 if bf else 1.0) * rn(rows, D)
        zero_mean = offs == 0
    elif family == "const":
        c = torch.tensor((3.25, -0.5, 100.), device="cuda")[r % 3]
        x = c.unsqueeze(1).expand(rows, D).clone()
    elif family == "small":
        x, zero_mean = 1e-3 * rn(rows, D), ~zero_mean
    else:
        step_last = min(511 if bf else 255, D - 1)
        col = torch.tensor((0, D - 1, step_last), device="cuda")[r % 3]
        x = torch.zeros(rows, D, device="cuda")
        x[r, col] = 1000.
    return x.to(dtype).contiguous(), zero_mean


@functools.lru_cache(maxsize=None)
def _fwd_case(family, dtype, rows, D):
    """Inputs, fp64 statistics and the aten comparator's error, made once
    per case and shared (read-only) by the forward tests."""
    gen = torch.Generator(device="cuda").manual_seed(
        7919 * D + 31 * rows + FAMILIES.index(family))
    x, zero_mean = _rows(family, dtype, rows, D, gen)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen).to(dtype)
    c = dict(x=x, w=rn(D), b=rn(D), zero_mean=zero_mean)
    x64 = x.double()
    c["mean"] = x64.mean(-1, keepdim=True)
    c["var"] = (x64 - c["mean"]).pow(2).mean(-1, keepdim=True)
    c["rstd"] = torch.rsqrt(c["var"] + EPS)
    c["xhat"] = (x64 - c["mean"]) * c["rstd"]
    c["mean_scale"] = torch.where(zero_mean,
                                  x64.abs().amax(-1, keepdim=True),
                                  c["mean"].abs())
    c["ms"] = x64.pow(2).mean(-1, keepdim=True)
    c["rrms"] = torch.rsqrt(c["ms"] + EPS)
    # the comparators: aten in fp32 on the same (upcast) inputs
    _, am, ar = torch.native_layer_norm(x.float(), [D], None, None, EPS)
    c["tol_mean"] = max(STAT_FACTOR * _rel(am, c["mean"], c["mean_scale"]),
                        STAT_FLOOR)
    c["tol_rstd"] = max(STAT_FACTOR * _rel(ar, c["rstd"], c["rstd"]),
                        STAT_FLOOR)
    from easydist_amd.ops.norms import _rms_fwd_aten
    _, rr = _rms_fwd_aten(x.float(), None, EPS)
    c["tol_rrms"] = max(STAT_FACTOR * _rel(rr, c["rrms"], c["rrms"]),
                        STAT_FLOOR)
    return c


def _rel(t, ref64, scale64):
    return float(((t.double().reshape(ref64.shape) - ref64).abs()
                  / scale64).max())


def _ratio(err, bound):
    """Worst err / bound; a zero bound demands a zero error, and a NaN or
    inf anywhere is a miss (NaN <= bound is False)."""
    bad = ~(err <= bound)
    r = torch.where(bound > 0, err / bound, torch.zeros_like(err))
    return float(r.max()), bool(bad.any())


def _check_stats(tag, c, mean, rstd, rms):
    rows = c["x"].shape[0]
    assert rstd.dtype == torch.float32 and tuple(rstd.shape) == (rows, 1)
    if rms:
        e = _rel(rstd, c["rrms"], c["rrms"])
        print(f"{tag} rstd rel {e:.3e} / tol {c['tol_rrms']:.3e}")
        assert e <= c["tol_rrms"], (tag, e, c["tol_rrms"])
        return
    assert mean.dtype == torch.float32 and tuple(mean.shape) == (rows, 1)
    em = _rel(mean, c["mean"], c["mean_scale"])
    er = _rel(rstd, c["rstd"], c["rstd"])
    print(f"{tag} mean rel {em:.3e} / tol {c['tol_mean']:.3e}  "
          f"rstd rel {er:.3e} / tol {c['tol_rstd']:.3e}")
    assert em <= c["tol_mean"], (tag, "mean", em, c["tol_mean"])
    assert er <= c["tol_rstd"], (tag, "rstd", er, c["tol_rstd"])


def _check_out(tag, c, out, w, b, rms):
    dtype = c["x"].dtype
    assert out.dtype == dtype and out.shape == c["x"].shape
    xhat = c["x"].double() * c["rrms"] if rms else c["xhat"]
    xw = xhat * w.double() if w is not None else xhat
    bb = b.double().expand_as(xw) if b is not None else torch.zeros_like(xw)
    ref = xw + bb
    slack = 1e-5 * (xw.abs() + bb.abs())
    if dtype == torch.bfloat16:
        bound = U16 * ref.abs() + slack
    else:
        wa = w.double().abs() if w is not None else 1.0
        if rms:
            prop = wa * xhat.abs() * c["tol_rrms"]
        else:
            prop = wa * (c["rstd"] * c["tol_mean"] * c["mean_scale"]
                         + xhat.abs() * c["tol_rstd"])
        bound = 16 * U32 * ref.abs() + slack + prop
    worst, bad = _ratio((out.double() - ref).abs(), bound)
    print(f"{tag} out worst err/bound {worst:.3f}")
    assert not bad, (tag, worst)


def _affine_variants(c, rms):
    if rms:
        return ((c["w"], None), (None, None))
    return ((c["w"], c["b"]), (None, None), (c["w"], None), (None, c["b"]))


@requires_gpu
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=_ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("family", FAMILIES)
def test_layer_norm_fwd(ext, family, dtype, shape):
    c = _fwd_case(family, dtype, *shape)
    for w, b in _affine_variants(c, False):
        tag = f"ln {family} {_dt(dtype)} {_ids(shape)} w{int(w is not None)}" \
              f"b{int(b is not None)}"
        out, mean, rstd = ext.layer_norm_fwd(c["x"], w, b, EPS)
        _check_stats(tag, c, mean, rstd, False)
        _check_out(tag, c, out, w, b, False)
        if family == "const":
            # variance exactly 0: rstd = 1/sqrt(eps), out = the bias
            want = (b if b is not None else torch.zeros_like(c["w"]))
            assert torch.equal(out, want.expand_as(out)), tag
            assert _rel(rstd, c["rstd"], c["rstd"]) <= STAT_FLOOR
            assert float((c["rstd"] - EPS ** -0.5).abs().max()) < 1e-9


@requires_gpu
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=_ids)
@pytest.mark.parametrize("family", FAMILIES)
def test_add_layer_norm_fwd(ext, family, shape):
    """a + b is the family's row exactly: a is x with its three lowest
    mantissa bits cleared, b the (exactly representable) rest."""
    c = _fwd_case(family, torch.bfloat16, *shape)
    x = c["x"]
    a = (x.view(torch.int16) & -8).view(torch.bfloat16)
    b2 = (x.float() - a.float()).bfloat16()
    assert torch.equal((a.float() + b2.float()).bfloat16(), x)
    for w, b in _affine_variants(c, False):
        tag = f"add_ln {family} {_ids(shape)} w{int(w is not None)}" \
              f"b{int(b is not None)}"
        s, out, mean, rstd = ext.add_layer_norm_fwd(a, b2, w, b, EPS)
        assert s.dtype == torch.bfloat16 and torch.equal(s, x), tag
        _check_stats(tag, c, mean, rstd, False)
        _check_out(tag, c, out, w, b, False)
        # and bit-equal to the unfused pair, on every family
        o2, m2, r2 = ext.layer_norm_fwd(x, w, b, EPS)
        assert torch.equal(out, o2), tag
        assert torch.equal(mean, m2) and torch.equal(rstd, r2), tag


@requires_gpu
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=_ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("family", FAMILIES)
def test_rms_norm_fwd(ext, family, dtype, shape):
    c = _fwd_case(family, dtype, *shape)
    for w, _ in _affine_variants(c, True):
        tag = f"rms {family} {_dt(dtype)} {_ids(shape)} w{int(w is not None)}"
        out, rstd = ext.rms_norm_fwd(c["x"], w, EPS)
        _check_stats(tag, c, None, rstd, True)
        _check_out(tag, c, out, w, None, True)


# ------------------------------------------------------------- backward ----
@functools.lru_cache(maxsize=None)
def _bwd_case(family, rows, D, onehot_grad):
    gen = torch.Generator(device="cuda").manual_seed(
        104729 * D + 17 * rows + FAMILIES.index(family) + 5 * onehot_grad)
    x, _ = _rows(family, torch.bfloat16, rows, D, gen)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen).bfloat16()
    c = dict(x=x, w=rn(D), res=rn(rows, D))
    if onehot_grad:
        g = torch.zeros(rows, D, device="cuda", dtype=torch.bfloat16)
        g[rows - 1, D - 1] = 3.0
    else:
        g = rn(rows, D)
    c["g"] = g
    x64 = x.double()
    m64 = x64.mean(-1, keepdim=True)
    r64 = torch.rsqrt((x64 - m64).pow(2).mean(-1, keepdim=True) + EPS)
    # the fp32 statistics the kernels get; the reference uses these values
    c["mean"], c["rstd"] = m64.float(), r64.float()
    c["rrms"] = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + EPS).float()
    return c


def _bwd_ref(c, w, rms):
    x64, g64 = c["x"].double(), c["g"].double()
    m = torch.zeros_like(c["mean"]).double() if rms else c["mean"].double()
    r = (c["rrms"] if rms else c["rstd"]).double()
    xh = (x64 - m) * r
    gw = g64 * w.double() if w is not None else g64
    c1 = torch.zeros_like(m) if rms else gw.mean(-1, keepdim=True)
    c2 = (gw * xh).mean(-1, keepdim=True)
    dx = r * (gw - c1 - xh * c2)
    slack = 1e-5 * r * (gw.abs() + c1.abs() + (xh * c2).abs())
    t = g64 * xh
    rows = x64.shape[0]
    return dict(dx=dx, slack=slack, dw=t.sum(0), db=g64.sum(0),
                dw_bound=(rows + 8) * U32 * t.abs().sum(0),
                db_bound=(rows + 8) * U32 * g64.abs().sum(0))


def _check_bwd(tag, c, ref, dx, dw, db, res, has_db=True):
    """dx, dw and (LayerNorm) db; RMSNorm has no bias and passes
    has_db=False with db=None."""
    rows, D = c["x"].shape
    assert isinstance(dx, torch.Tensor) and isinstance(dw, torch.Tensor), tag
    assert isinstance(db, torch.Tensor) if has_db else db is None, tag
    assert dx.dtype == torch.bfloat16 and dx.shape == c["x"].shape, tag
    want = ref["dx"]
    bound = U16 * want.abs() + ref["slack"]
    if res is not None:
        want = want + res.double()
        bound = bound + U16 * want.abs()
    worst, bad = _ratio((dx.double() - want).abs(), bound)
    line = f"{tag} dx worst err/bound {worst:.3f}"
    assert not bad, (tag, "dx", worst)
    for name, t in (("dw", dw), ("db", db))[:2 if has_db else 1]:
        assert t.dtype == torch.float32 and tuple(t.shape) == (D,), (tag, name)
        wst, bad = _ratio((t.double() - ref[name]).abs(),
                          ref[name + "_bound"])
        line += f"  {name} {wst:.3f}"
        assert not bad, (tag, name, wst)
    print(line)


def _run_ln_bwd(ext, family, shape, onehot_grad, fuse):
    c = _bwd_case(family, *shape, onehot_grad)
    mask = [True, True, True]
    env = {} if fuse else {"EASYDIST_NORM_FUSE": "0"}
    for w in (c["w"], None):
        ref = _bwd_ref(c, w, False)
        tag = f"ln_bwd fuse{int(fuse)} {family} {_ids(shape)} " \
              f"w{int(w is not None)}"
        with _env(**env):
            dx, dw, db = ext.layer_norm_bwd(c["g"], c["x"], c["mean"],
                                            c["rstd"], w, mask)
            _check_bwd(tag, c, ref, dx, dw, db, None)
            for res in (c["res"], None):
                dx, dw, db = ext.layer_norm_bwd_res(
                    c["g"], c["x"], c["mean"], c["rstd"], w, res, mask)
                _check_bwd(tag + f" res{int(res is not None)}", c, ref, dx,
                           dw, db, res)


@requires_gpu
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=_ids)
@pytest.mark.parametrize("family", ("randn", "offset"))
@pytest.mark.parametrize("fuse", (True, False), ids=("fused", "unfused"))
def test_layer_norm_bwd(ext, fuse, family, shape):
    _run_ln_bwd(ext, family, shape, False, fuse)


@requires_gpu
@pytest.mark.parametrize("shape", ((5000, 776), (1027, 4096)), ids=_ids)
@pytest.mark.parametrize("fuse", (True, False), ids=("fused", "unfused"))
def test_layer_norm_bwd_onehot_grad(ext, fuse, shape):
    _run_ln_bwd(ext, "randn", shape, True, fuse)


def _run_rms_bwd(ext, family, shape, onehot_grad):
    c = _bwd_case(family, *shape, onehot_grad)
    for w in (c["w"], None):
        ref = _bwd_ref(c, w, True)
        tag = f"rms_bwd {family} {_ids(shape)} w{int(w is not None)}"
        out = ext.rms_norm_bwd(c["g"], c["x"], c["rrms"], w)
        assert len(out) == 2
        _check_bwd(tag, c, ref, out[0], out[1], None, None, has_db=False)


@requires_gpu
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=_ids)
@pytest.mark.parametrize("family", ("randn", "offset"))
def test_rms_norm_bwd(ext, family, shape):
    _run_rms_bwd(ext, family, shape, False)


@requires_gpu
def test_rms_norm_bwd_onehot_grad(ext):
    _run_rms_bwd(ext, "randn", (5000, 776), True)


# --------------------------------------------------------------- module ----
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_rms_norm_module(ext, dtype):
    """RMSNorm with its default fp32 weight on bf16 and fp32 activations:
    forward and both gradients against fp64."""
    from easydist_amd.ops.norms import RMSNorm
    rows, D, eps = 1027, 776, 1e-6
    gen = torch.Generator(device="cuda").manual_seed(4242)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    mod = RMSNorm(D, eps=eps).cuda()
    with torch.no_grad():
        mod.weight.copy_(rn(D))
    assert mod.weight.dtype == torch.float32
    x = (1.5 * rn(rows, D) + 0.25).to(dtype).requires_grad_()
    g = rn(rows, D).to(dtype)
    out = mod(x)
    out.backward(g)
    assert out.dtype == dtype and x.grad.dtype == dtype
    assert mod.weight.grad.dtype == torch.float32
    assert mod.weight.grad.shape == mod.weight.shape

    # the kernels read the weight in the activation's dtype
    w64 = mod.weight.detach().to(dtype).double()
    x64, g64 = x.detach().double(), g.double()
    r = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + eps)
    xh = x64 * r
    rnd = U16 if dtype == torch.bfloat16 else 16 * U32
    ref = xh * w64
    worst, bad = _ratio((out.detach().double() - ref).abs(),
                        rnd * ref.abs() + 1e-5 * ref.abs())
    line = f"rms module {_dt(dtype)} out {worst:.3f}"
    assert not bad, ("out", worst)
    gw = g64 * w64
    c2 = (gw * xh).mean(-1, keepdim=True)
    dx = r * (gw - xh * c2)
    bound = rnd * dx.abs() + 1e-5 * r * (gw.abs() + (xh * c2).abs())
    worst, bad = _ratio((x.grad.double() - dx).abs(), bound)
    line += f" dx {worst:.3f}"
    assert not bad, ("dx", worst)
    t = g64 * xh
    worst, bad = _ratio((mod.weight.grad.double() - t.sum(0)).abs(),
                        (rows + 8) * U32 * t.abs().sum(0))
    print(line + f" dw {worst:.3f}")
    assert not bad, ("dw", worst)
