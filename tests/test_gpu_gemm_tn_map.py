"""Split-R TN GEMMs under the two workgroup maps (EASYDIST_TN_MAP).

The map only moves (tile, slice) pairs between workgroup ids.  Inputs are
integers in [-2, 2] stored as bf16, so every product and every partial sum
is an integer below 2^24 and exact in fp32 whatever order the atomics land
in: the outputs under BOTH maps must equal the fp32 reference rounded to
bf16 element for element, and the fused column sums must equal
a.float().sum(0).  A (tile, slice) that is missed or visited twice shows
up as a wrong integer; the split-R workspace is zero-filled, so an
unvisited tile reads as zero (no reference here has an all-zero 256x256
tile: checked on the CPU for these seeds, and asserted below).

Both tile sizes are instantiations of one kernel template.  The older TN
tests never reach gemm_tn_256_kernel with a split (it needs R >= 2048 and
P, Q >= 256); the shapes with P, Q >= 256 are the smallest that do.  The
256-tile kernel's r-loop has two staging forms (EASYDIST_TN256_STAGING: the
three-buffer ring and the older issue-then-drain loop); both run under both
maps, and two shapes give the ring a last slice shorter than its prefetch
distance.  The shapes with P or Q below 256 reach gemm_tn_kernel, the
128-tile instantiation: with and without a split, with one r-tile and with
several per slice, and with a second tile column that skips the column sum.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

# (R, P, Q)
CASES = [
    (2048, 256, 256),   # one tile, splitr 8, 8 workgroups
    (2048, 512, 256),   # 2 tiles, 16 workgroups
    (2304, 768, 256),   # 3 tiles x 9 slices = 27, swizzle remainder 3
    (4096, 768, 768),   # 9 tiles x 16 slices
    (2048, 384, 256),   # partial edge tile
    (1024, 256, 128),   # 128-tile kernel with its power-of-two split
    (2336, 768, 256),   # 73 r-tiles, 9 slices of 9: the last holds 1 tile
    (2080, 256, 512),   # 65 r-tiles, 8 slices of 9: the last holds 2 tiles
    # the 128-tile instantiation's remaining paths
    (32, 128, 128),     # one r-tile, no split: direct stores, empty loop tail
    (96, 128, 256),     # 3 r-tiles, no split, 2 tiles: buffers wrap, q0 != 0
    (512, 128, 384),    # 3 tiles x 16 slices of one r-tile
    (4096, 256, 128),   # R fits the 256 kernel but Q < 256: 8 r-tiles a slice
]


@pytest.fixture(scope="module")
def ext():
    import easydist_amd.ops as ops
    e = ops.load_extension()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _inputs(idx, R, P, Q):
    g = torch.Generator().manual_seed(400 + idx)
    a = torch.randint(-2, 3, (R, P), generator=g).to(torch.bfloat16)
    b = torch.randint(-2, 3, (R, Q), generator=g).to(torch.bfloat16)
    return a, b


@requires_gpu
@pytest.mark.parametrize("case", list(enumerate(CASES)),
                         ids=lambda c: "R{}P{}Q{}".format(*c[1]))
def test_gemm_tn_map_modes(ext, monkeypatch, case):
    idx, (R, P, Q) = case
    a, b = (t.cuda() for t in _inputs(idx, R, P, Q))
    ref32 = a.float().t() @ b.float()
    ref = ref32.to(torch.bfloat16)
    ref_sum = a.float().sum(0)
    for p in range(0, P, 256):
        for q in range(0, Q, 256):
            assert bool(ref32[p:p + 256, q:q + 256].any()), (p, q)

    for staging in ("1", "0"):
        monkeypatch.setenv("EASYDIST_TN256_STAGING", staging)
        for mode in ("0", "1"):
            monkeypatch.setenv("EASYDIST_TN_MAP", mode)
            c = ext.gemm_tn(a, b)
            c2, asum = ext.gemm_tn_asum(a, b)
            torch.cuda.synchronize()
            for name, got in (("gemm_tn", c), ("gemm_tn_asum", c2)):
                assert got.dtype == torch.bfloat16 and got.shape == (P, Q)
                bad = int((got != ref).sum())
                assert bad == 0, \
                    (staging, mode, name, bad,
                     float((got.float() - ref.float()).abs().max()))
            assert torch.equal(asum, ref_sum), \
                (staging, mode, float((asum - ref_sum).abs().max()))
