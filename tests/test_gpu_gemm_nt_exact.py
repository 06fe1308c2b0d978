"""The NT GEMM kernels, their fused epilogues and the ops that wrap them.

1. Plain GEMM, exact.  a and bt are integers in [-2, 2] stored as bf16,
bias integers in [-8, 8]: every product and every partial sum is an integer
far below 2^24, so fp32 accumulation is exact in any order and
ext.gemm_nt must equal (a @ bt^T + bias) rounded to bf16 element for
element.  One dropped, duplicated or stale k element moves an output by at
least one integer step.  Every 128x128 tile of every reference holds a
non-zero entry (asserted on the CPU), so an unvisited tile cannot pass as
zeros, and the outputs are allocated over NaN-poisoned memory.

Shapes (M, N, K) and the path each reaches.  gemm_nt_256 (K % 64 == 0,
M >= 256, N >= 128; NT = K / 64 k-tiles):
  (256, 128, 64)   one workgroup, NT 1, half-wide N: clamped source columns
  (256, 256, 128)  NT 2, a full tile
  (257, 264, 192)  NT 3, one-row M tail, 8-column N tail, 4 workgroups
  (512, 384, 320)  NT 5: odd, buffer parity wraps
  (768, 768, 256)  9 workgroups (xcd_swizzle remainder 1), NT 4
  (1280, 768, 64)  15 workgroups (remainder 7), prologue + dummy-stage tail
  (256, 256, 768)  NT 12, the workload's K
gemm_nt_128 (everything else the dispatcher admits):
  (16, 8, 32)      the minimum: one k-tile
  (100, 136, 96)   3 k-tiles, M and N tails
  (255, 512, 64)   just under the M threshold with K % 64 == 0
  (512, 120, 128)  N < 128
  (512, 512, 96)   K % 64 != 0, 16 workgroups

2. Epilogue modes 1 to 6 against fp64.  a is integers in [-1, 1], bt and
bias integers/16 with |bt| <= 4/16 and |bias| <= 1, so the pre-activation
is still exact in fp32 and pre_ref = bf16(a @ bt^T + bias) is exactly the
value the epilogue reads back from its bf16 bounce.  aux for the backward
modes is bf16(2 * randn).  At least half of pre_ref has |pre| < 3
(asserted), so the data sit in gelu's curved range.  The forward modes 1
and 3 are called without aux.  Modes 5 and 6 must return pre_ref exactly,
through gemm_nt_gelu and through gemm_nt_act with a caller-owned,
NaN-filled aux.  Bounds, got in bf16 against an fp64 reference:
  forward  1, 3, 5, 6:  |got - ref| <= 2^-8 |ref| + F (1 + |pre_ref|)
  backward 2, 4:        |got - ref| <= 2^-8 |ref| + B |pre_ref| (1 + |aux|)
2^-8 |ref| is the worst case of the one bf16 rounding.  F and B cover the
fp32 evaluation of act_apply's formula: with exactly these input
distributions plain fp32 torch on the CPU against fp64 measured 6.0e-8 for
F's term and 3.2e-7 for B's; the device's __expf gets a margin of 8x over
libm, so F = 5e-7 and B = 2.6e-6.  Neither was measured against the kernel.
Modes 1, 2, 5 are tanh-gelu.  Modes 3, 4, 6 are nominally erf-gelu but the
256 kernel computes the tanh form: there they are held to the tanh
reference with the bounds above, and on both paths to the erf reference
with E added, E being the largest |erf form - tanh form| of gelu (forward,
about 4.7e-4) and of dgelu (backward, about 8.7e-4, times |pre_ref|),
computed here in fp64 on a grid of step 2^-12 over [-10, 10].  The 128
path applies its activation through aten.
256 path: (256,128,64) (257,264,192) (512,384,320) (256,256,768);
128 path: (100,136,96) (255,512,64).

3. torch.ops.easydist_amd.gemm_nt / gemm_nt_act / gemm_nt_gelu / gemm_nn /
gemm_nn_act on device tensors under EASYDIST_GEMM_POLICY = hand, aten and
auto (with an empty tune cache), at (512,384,320), (100,136,96) and the
unsupported (16,12,40) that must fall back to aten.  bt is a transposed
view, gemm_nn's b is [K, N] row-major and aux is a slice of a wider
tensor, so the wrappers' .contiguous() calls copy.  Plain results are
exact under every policy (hipBLASLt accumulates these integers exactly as
well); activated ones meet the section 2 bounds of their nominal function,
the erf modes with E since the aten route applies gelu_fast.

4. gelu_fast / gelu_bwd_fast cap their grid at 8192 blocks of 256 threads
of 8 elements; n = 2^24 + 2400 gives 300 threads a second trip of the
grid-stride loop.  Data are bf16(3 * randn), references fp64 tanh forms
computed on the device, bounds as in section 2; the last 2400 elements are
asserted on their own.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

BF = torch.bfloat16
F_TOL = 5e-7     # 8 x 6.0e-8, see the docstring
B_TOL = 2.6e-6   # 8 x 3.2e-7

# (M, N, K)
CASES_256 = [(256, 128, 64), (256, 256, 128), (257, 264, 192),
             (512, 384, 320), (768, 768, 256), (1280, 768, 64),
             (256, 256, 768)]
CASES_128 = [(16, 8, 32), (100, 136, 96), (255, 512, 64), (512, 120, 128),
             (512, 512, 96)]
ACT_CASES_256 = [(256, 128, 64), (257, 264, 192), (512, 384, 320),
                 (256, 256, 768)]
ACT_CASES_128 = [(100, 136, 96), (255, 512, 64)]
WRAP_CASES = [(512, 384, 320), (100, 136, 96), (16, 12, 40)]
_SEEDED = CASES_256 + CASES_128 + [(16, 12, 40)]


def _is_256(M, N, K):
    return K % 64 == 0 and M >= 256 and N >= 128


def _sid(s):
    return "M{}N{}K{}".format(*s)


@pytest.fixture(scope="module")
def ext():
    import easydist_amd.ops as ops
    e = ops.load_extension()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _poison(*shapes):
    """Allocate, NaN-fill and free bf16 tensors of the output sizes so the
    outputs of the next call most likely reuse poisoned memory."""
    ts = [torch.full(s, float("nan"), device="cuda", dtype=BF)
          for s in shapes]
    torch.cuda.synchronize()
    del ts


# ------------------------------------------------------------- references --
_GELU_C = math.sqrt(2.0 / math.pi)
_GELU_A = 0.044715


def _gelu_tanh(x):
    t = torch.tanh(_GELU_C * (x + _GELU_A * x * x * x))
    return 0.5 * x * (1.0 + t)


def _dgelu_tanh(x):
    t = torch.tanh(_GELU_C * (x + _GELU_A * x * x * x))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _GELU_C \
        * (1.0 + 3.0 * _GELU_A * x * x)


def _gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _dgelu_erf(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) \
        + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


_FWD = {"tanh": _gelu_tanh, "erf": _gelu_erf}
_BWD = {"tanh": _dgelu_tanh, "erf": _dgelu_erf}


@functools.lru_cache(maxsize=None)
def _erf_gap():
    """(E forward, E backward per unit of gradient), fp64, dense grid."""
    x = torch.arange(-10 * 4096, 10 * 4096 + 1, dtype=torch.float64) / 4096
    return (float((_gelu_erf(x) - _gelu_tanh(x)).abs().max()),
            float((_dgelu_erf(x) - _dgelu_tanh(x)).abs().max()))


def _assert_tiles_nonzero(ref, tag):
    M, N = ref.shape
    for m in range(0, M, 128):
        for n in range(0, N, 128):
            assert bool(ref[m:m + 128, n:n + 128].any()), (tag, m, n)


@functools.lru_cache(maxsize=None)
def _plain_case(shape):
    """Section 1 data and references, on the CPU, made once per shape."""
    M, N, K = shape
    g = torch.Generator().manual_seed(700 + _SEEDED.index(shape))
    a = torch.randint(-2, 3, (M, K), generator=g).to(BF)
    bt = torch.randint(-2, 3, (N, K), generator=g).to(BF)
    bias = torch.randint(-8, 9, (N,), generator=g).to(BF)
    acc = a.float() @ bt.float().t()
    ref = {False: acc.to(BF), True: (acc + bias.float()).to(BF)}
    for with_bias, r in ref.items():
        _assert_tiles_nonzero(r, (shape, with_bias))
    return {"a": a, "bt": bt, "bias": bias, "ref": ref}


@functools.lru_cache(maxsize=None)
def _act_case(shape):
    """Section 2 data and pre_ref, on the CPU, made once per shape."""
    M, N, K = shape
    g = torch.Generator().manual_seed(800 + _SEEDED.index(shape))
    a = torch.randint(-1, 2, (M, K), generator=g).to(BF)
    bt = (torch.randint(-4, 5, (N, K), generator=g).float() / 16).to(BF)
    bias = (torch.randint(-16, 17, (N,), generator=g).float() / 16).to(BF)
    aux = (2 * torch.randn(M, N, generator=g)).to(BF)
    pre_ref = (a.float() @ bt.float().t() + bias.float()).to(BF)
    _assert_tiles_nonzero(pre_ref, shape)
    share = float((pre_ref.float().abs() < 3).float().mean())
    assert share >= 0.5, (shape, share)
    return {"a": a, "bt": bt, "bias": bias, "aux": aux, "pre_ref": pre_ref}


# ----------------------------------------------------------------- checks --
def _check_exact(got, ref, tag):
    ref = ref.to(got.device)
    assert got.dtype == BF and got.shape == ref.shape, tag
    assert bool(torch.isfinite(got).all()), tag
    bad = int((got != ref).sum())
    maxd = float((got.float() - ref.float()).abs().max())
    print(tag, "mismatches", bad, "max diff", maxd)
    assert bad == 0, (tag, bad, maxd)


def _check_bound(got, ref, bound, tag):
    assert got.dtype == BF and got.shape == ref.shape, tag
    assert bool(torch.isfinite(got).all()), tag
    err = (got.double() - ref).abs()
    over = int((err > bound).sum())
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    print(tag, "over bound", over, "max err/bound", worst,
          "max err", float(err.max()))
    assert over == 0, (tag, over, worst, float(err.max()))


def _check_fwd(got, pre_ref, form, tag, extra=0.0):
    x = pre_ref.to(got.device).double()
    ref = _FWD[form](x)
    bound = 2.0 ** -8 * ref.abs() + F_TOL * (1 + x.abs()) + extra
    _check_bound(got, ref, bound, (tag, "fwd", form))


def _check_bwd(got, pre_ref, aux, form, tag, extra=0.0):
    g = pre_ref.to(got.device).double()
    x = aux.to(got.device).double()
    ref = g * _BWD[form](x)
    bound = 2.0 ** -8 * ref.abs() + B_TOL * g.abs() * (1 + x.abs()) \
        + extra * g.abs()
    _check_bound(got, ref, bound, (tag, "bwd", form))


def _check_mode(got, mode, case, tag, tanh_form):
    """Hold `got` to mode's nominal function; tanh_form: the erf modes are
    known to compute the tanh form and are held to it as well."""
    e_fwd, e_bwd = _erf_gap()
    pre_ref, aux = case["pre_ref"], case["aux"]
    if mode in (1, 5):
        _check_fwd(got, pre_ref, "tanh", tag)
    elif mode == 2:
        _check_bwd(got, pre_ref, aux, "tanh", tag)
    elif mode in (3, 6):
        if tanh_form:
            _check_fwd(got, pre_ref, "tanh", tag)
        _check_fwd(got, pre_ref, "erf", tag, extra=e_fwd)
    elif mode == 4:
        if tanh_form:
            _check_bwd(got, pre_ref, aux, "tanh", tag)
        _check_bwd(got, pre_ref, aux, "erf", tag, extra=e_bwd)
    else:
        raise AssertionError(mode)


# ------------------------------------------------------- 1. plain, exact ---
@requires_gpu
@pytest.mark.parametrize("shape", CASES_256 + CASES_128, ids=_sid)
def test_gemm_nt_exact(ext, shape):
    M, N, K = shape
    case = _plain_case(shape)
    a, bt, bias = (case[k].cuda() for k in ("a", "bt", "bias"))
    for with_bias in (True, False):
        _poison((M, N))
        c = ext.gemm_nt(a, bt, bias if with_bias else None)
        torch.cuda.synchronize()
        _check_exact(c, case["ref"][with_bias], (shape, "bias", with_bias))


# ---------------------------------------------------- 2. epilogue modes ----
@requires_gpu
@pytest.mark.parametrize("shape", ACT_CASES_256 + ACT_CASES_128, ids=_sid)
def test_gemm_nt_epilogues(ext, shape):
    M, N, K = shape
    case = _act_case(shape)
    a, bt, bias, aux = (case[k].cuda() for k in ("a", "bt", "bias", "aux"))
    tanh_form = _is_256(*shape)

    for mode in (1, 2, 3, 4):
        _poison((M, N))
        got = ext.gemm_nt_act(a, bt, bias, mode,
                              aux if mode in (2, 4) else None)
        torch.cuda.synchronize()
        _check_mode(got, mode, case, (shape, "act", mode), tanh_form)

    for mode in (5, 6):
        # caller-owned aux: an output here, poisoned by the caller
        _poison((M, N))
        pre = torch.full((M, N), float("nan"), device="cuda", dtype=BF)
        got = ext.gemm_nt_act(a, bt, bias, mode, pre)
        torch.cuda.synchronize()
        _check_exact(pre, case["pre_ref"], (shape, "act aux", mode))
        _check_mode(got, mode, case, (shape, "act", mode), tanh_form)

    for tanh_approx, mode in ((True, 5), (False, 6)):
        _poison((M, N), (M, N))
        got, pre = ext.gemm_nt_gelu(a, bt, bias, tanh_approx)
        torch.cuda.synchronize()
        _check_exact(pre, case["pre_ref"], (shape, "gelu pre", mode))
        _check_mode(got, mode, case, (shape, "gelu", mode), tanh_form)


# ------------------------------------------------- 3. the wrapper ops ------
def _views(case, with_aux):
    """Device inputs as the non-contiguous views the wrappers must copy."""
    a = case["a"].cuda()
    b_kn = case["bt"].cuda().t().contiguous()        # [K, N] row-major
    bt_view = b_kn.t()                               # [N, K], strided
    bias = case["bias"].cuda()
    assert not bt_view.is_contiguous()
    aux_view = None
    if with_aux:
        M, N = case["aux"].shape
        wide = torch.full((M, N + 16), float("nan"), device="cuda", dtype=BF)
        aux_view = wide[:, 8:8 + N]
        aux_view.copy_(case["aux"])
        assert not aux_view.is_contiguous()
    return a, b_kn, bt_view, bias, aux_view


@requires_gpu
@pytest.mark.parametrize("shape", WRAP_CASES, ids=_sid)
@pytest.mark.parametrize("policy", ["hand", "aten", "auto"])
def test_gemm_wrapper_ops(ext, monkeypatch, policy, shape):
    import easydist_amd.ops.gemm as gemm_mod
    ops = torch.ops.easydist_amd
    monkeypatch.setenv("EASYDIST_GEMM_POLICY", policy)
    if policy == "auto":
        monkeypatch.setattr(gemm_mod, "_tune_cache", {})
    M, N, K = shape

    plain = _plain_case(shape)
    a, b_kn, bt_view, bias, _ = _views(plain, False)
    for with_bias in (True, False):
        b_arg = bias if with_bias else None
        ref = plain["ref"][with_bias]
        _poison((M, N))
        c = ops.gemm_nt(a, bt_view, b_arg)
        torch.cuda.synchronize()
        _check_exact(c, ref, (policy, shape, "gemm_nt", with_bias))
        _poison((M, N))
        c = ops.gemm_nn(a, b_kn, b_arg)
        torch.cuda.synchronize()
        _check_exact(c, ref, (policy, shape, "gemm_nn", with_bias))

    # the erf modes may take the kernel's tanh form or aten's erf,
    # depending on the route: they are held to the erf reference plus E
    case = _act_case(shape)
    a, b_kn, bt_view, bias, aux_view = _views(case, True)
    for mode in (1, 2, 3, 4):
        x = aux_view if mode in (2, 4) else None
        _poison((M, N))
        got = ops.gemm_nt_act(a, bt_view, bias, mode, x)
        torch.cuda.synchronize()
        _check_mode(got, mode, case, (policy, shape, "gemm_nt_act", mode),
                    False)
        _poison((M, N))
        got = ops.gemm_nn_act(a, b_kn, bias, mode, x)
        torch.cuda.synchronize()
        _check_mode(got, mode, case, (policy, shape, "gemm_nn_act", mode),
                    False)
    for tanh_approx, mode in ((True, 5), (False, 6)):
        _poison((M, N), (M, N))
        got, pre = ops.gemm_nt_gelu(a, bt_view, bias, tanh_approx)
        torch.cuda.synchronize()
        _check_exact(pre, case["pre_ref"],
                     (policy, shape, "gemm_nt_gelu pre", mode))
        _check_mode(got, mode, case, (policy, shape, "gemm_nt_gelu", mode),
                    False)
    if policy == "auto" and shape != (16, 12, 40):
        assert gemm_mod._tune_cache, "auto policy never profiled a shape"


# -------------------------------------- 4. gelu kernels, grid-stride loop --
@requires_gpu
def test_gelu_fast_grid_stride(ext):
    n = 2 ** 24 + 2400
    tail = 2400
    assert n % 8 == 0 and (n - 8192 * 256 * 8) // 8 == 300
    gen = torch.Generator().manual_seed(900)
    x = (3 * torch.randn(n, generator=gen)).to(BF).cuda()
    g = (3 * torch.randn(n, generator=gen)).to(BF).cuda()

    _poison((n,))
    y = ext.gelu_fast(x)
    _poison((n,))
    dy = ext.gelu_bwd_fast(g, x)
    torch.cuda.synchronize()

    _check_fwd(y, x, "tanh", "gelu_fast")
    _check_fwd(y[-tail:], x[-tail:], "tanh", "gelu_fast tail")
    _check_bwd(dy, g, x, "tanh", "gelu_bwd_fast")
    _check_bwd(dy[-tail:], g[-tail:], x[-tail:], "tanh", "gelu_bwd_fast tail")
