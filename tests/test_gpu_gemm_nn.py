"""The native NN GEMM kernels: C = a @ b (+bias) with b [K, N] row-major.

1. ext.gemm_nn, exact.  a, b integers in [-2, 2] as bf16, bias in [-8, 8]:
every partial sum is an integer far below 2^24, so the result must equal
bf16(fp64(a) @ fp64(b) + bias) element for element.  Every 128x128 tile of
every reference holds a non-zero entry (asserted on the CPU); the output
memory is NaN-poisoned.  Shapes (M, N, K), gemm_nn_256 (M, N >= 256, K % 64):
  (256, 256, 64)   one workgroup, one k-tile: prologue + dummy-stage tail
  (256, 256, 128)  two k-tiles;  (256, 256, 768) the workload's K
  (257, 264, 192)  1-row M tail, 8-col N tail (tn_stage clamp), 4 WGs, NT 3
  (512, 384, 320)  5 k-tiles, buffer parity wraps, half-wide N edge tile
  (768, 768, 256)  9 workgroups, xcd_swizzle remainder
gemm_nn_128 (the rest of the envelope): (16, 8, 32) the minimum; (100, 136,
96) M, N tails; (255, 512, 64), (512, 248, 128) just under the M and N
thresholds; (512, 512, 96) K % 64 != 0.

2. ext.gemm_nn_act against fp64, inputs and bounds of
test_gpu_gemm_nt_exact.py section 2: a integers in [-1, 1], b and bias
integers/16, |b| <= 4/16, |bias| <= 1, so pre_ref = bf16(a @ b + bias) is
exactly what the epilogue reads back; aux is bf16(2 * randn).
  forward  1, 5:  |got - ref| <= 2^-8 |ref| + F (1 + |pre_ref|)
  backward 2, 4:  |got - ref| <= 2^-8 |ref| + B |pre_ref| (1 + |aux|)
with that file's F = 5e-7, B = 2.6e-6.  Mode 4 is nominally erf-gelu:
gemm_nn_256 computes the tanh form and is held to the tanh reference; both
paths are held to the erf reference with E |pre_ref| added, E the largest
|dgelu_erf - dgelu_tanh| in fp64 on a grid of step 2^-12 over [-10, 10] (the
128 path applies aten's erf).  Mode 5 must return pre_ref exactly in a
caller-owned, NaN-filled aux.  Two shapes of the 256 path, one of the 128.

3. torch.ops.easydist_amd.gemm_nn, policy hand, a [512, 1024], b [1024, 2048]:
the peak of a warm call stays under the 2 MiB output plus 1 MiB (a transposed
copy of b is 4 MiB), and the result is exact.

4. One gemm_nn_act call (mode 2, (257, 264, 192), policy hand) captured in a
graph, replayed twice with the rows of a reversed in place in between (which
reverses the rows of pre_ref): each replay meets the section 2 bound.
"""
import functools
import math

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X")]
BF = torch.bfloat16
F_TOL, B_TOL = 5e-7, 2.6e-6
CASES_256 = [(256, 256, 64), (256, 256, 128), (257, 264, 192),
             (512, 384, 320), (768, 768, 256), (256, 256, 768)]
CASES_128 = [(16, 8, 32), (100, 136, 96), (255, 512, 64), (512, 248, 128),
             (512, 512, 96)]
ACT_CASES = [(257, 264, 192), (256, 256, 768), (100, 136, 96)]
COPY_CASE = (512, 2048, 1024)
_C, _A = math.sqrt(2.0 / math.pi), 0.044715


@pytest.fixture(scope="module")
def ext():
    import easydist_amd.ops as ops
    assert ops.load_extension() is not None, "HIP extension must be built"
    return ops.load_extension()


def _poison(M, N):
    """NaN-fill and free a block the next output most likely reuses."""
    t = torch.full((M, N), float("nan"), device="cuda", dtype=BF)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _case(shape, act):
    """Seeded device inputs and CPU references of section 1 or 2 (act)."""
    M, N, K = shape
    g = torch.Generator().manual_seed(1700 + 50 * act + M + 3 * N + 7 * K)
    lim, blim, div = (1, 16, 16.0) if act else (2, 8, 1.0)
    a = torch.randint(-lim, lim + 1, (M, K), generator=g).to(BF)
    b = (torch.randint(-2 * (1 + act), 2 * (1 + act) + 1, (K, N), generator=g)
         / div).to(BF)
    bias = (torch.randint(-blim, blim + 1, (N,), generator=g) / div).to(BF)
    aux = (2 * torch.randn(M, N, generator=g)).to(BF)
    acc = a.double() @ b.double()
    ref = {False: acc.to(BF), True: (acc + bias.double()).to(BF)}
    for r in ref.values():
        for m in range(0, M, 128):
            for n in range(0, N, 128):
                assert bool(r[m:m + 128, n:n + 128].any()), (shape, m, n)
    return a.cuda(), b.cuda(), bias.cuda(), aux.cuda(), ref


def _dgelu(x, erf):
    if erf:
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) \
            + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    t = torch.tanh(_C * (x + _A * x * x * x))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _C \
        * (1.0 + 3.0 * _A * x * x)


def _check_exact(got, ref, tag):
    bad = int((got != ref.cuda()).sum()) + int((~torch.isfinite(got)).sum())
    assert got.dtype == BF and got.shape == ref.shape and bad == 0, (tag, bad)


def _check_act(got, mode, pre_ref, aux, erf, tag):
    """Section 2 bound of `mode`; erf: the erf reference, E |pre_ref| added."""
    p, x = pre_ref.cuda().double(), aux.double()
    if mode in (2, 4):
        ref = p * _dgelu(x, erf)
        bound = 2.0 ** -8 * ref.abs() + B_TOL * p.abs() * (1 + x.abs())
        if erf:
            grid = torch.arange(-40960, 40961, dtype=torch.float64) / 4096
            bound += float((_dgelu(grid, True) - _dgelu(grid, False))
                           .abs().max()) * p.abs()
    else:
        ref = 0.5 * p * (1.0 + torch.tanh(_C * (p + _A * p * p * p)))
        bound = 2.0 ** -8 * ref.abs() + F_TOL * (1 + p.abs())
    assert got.dtype == BF and bool(torch.isfinite(got).all()), tag
    err = (got.double() - ref).abs()
    assert not bool((err > bound).any()), (tag, erf, float(err.max()))


@pytest.mark.parametrize("shape", CASES_256 + CASES_128, ids=str)
def test_gemm_nn_exact(ext, shape):
    a, b, bias, _, ref = _case(shape, False)
    for with_bias in (True, False):
        _poison(shape[0], shape[1])
        c = ext.gemm_nn(a, b, bias if with_bias else None)
        torch.cuda.synchronize()
        _check_exact(c, ref[with_bias], (shape, "bias", with_bias))


@pytest.mark.parametrize("shape", ACT_CASES, ids=str)
def test_gemm_nn_epilogues(ext, shape):
    a, b, bias, aux, ref = _case(shape, True)
    for mode in (1, 2, 4, 5):
        _poison(shape[0], shape[1])
        # mode 5: a caller-owned aux, an output here
        x = {1: None, 5: torch.full_like(aux, float("nan"))}.get(mode, aux)
        got = ext.gemm_nn_act(a, b, bias, mode, x)
        torch.cuda.synchronize()
        if mode != 4 or shape in CASES_256:
            _check_act(got, mode, ref[True], aux, False, (shape, mode))
        if mode == 4:
            _check_act(got, mode, ref[True], aux, True, (shape, mode))
        if mode == 5:
            _check_exact(x, ref[True], (shape, "mode 5 aux"))


def test_gemm_nn_no_weight_copy(ext, monkeypatch):
    monkeypatch.setenv("EASYDIST_GEMM_POLICY", "hand")
    a, b, _, _, ref = _case(COPY_CASE, False)
    torch.ops.easydist_amd.gemm_nn(a, b, None)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    c = torch.ops.easydist_amd.gemm_nn(a, b, None)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    assert extra < c.numel() * 2 + 2 ** 20, extra
    _check_exact(c, ref[False], COPY_CASE)


def test_gemm_nn_act_graph_replay(ext, monkeypatch):
    monkeypatch.setenv("EASYDIST_GEMM_POLICY", "hand")
    a, b, bias, aux, ref = _case((257, 264, 192), True)
    a, pre_ref = a.clone(), ref[True]
    op = torch.ops.easydist_amd.gemm_nn_act
    op(a, b, bias, 2, aux)          # eager warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op(a, b, bias, 2, aux)
    for flipped in (False, True):
        if flipped:
            a.copy_(a.flip(0))
            pre_ref = pre_ref.flip(0)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _check_act(out, 2, pre_ref, aux, False, ("replay", flipped))
