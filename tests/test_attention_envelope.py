"""The flash kernels' dispatch envelope (ops.attention._kernel_ok).

Any sequence length is inside: S % 128 != 0 runs the ragged-tail
instantiations.  Head dim, dtype and shape agreement still decide.
"""
import pytest
import torch

from easydist_amd.ops import attention


def _qkv(S, D, dtype=torch.bfloat16):
    return tuple(torch.zeros(2, 3, S, D, dtype=dtype) for _ in range(3))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [1, 63, 197, 320])
def test_any_sequence_length_is_inside(S, D):
    assert attention._kernel_ok(*_qkv(S, D))


@pytest.mark.parametrize("S", [128, 197])
def test_still_outside(S):
    # head dim
    assert not attention._kernel_ok(*_qkv(S, 32))
    # dtype
    assert not attention._kernel_ok(*_qkv(S, 64, torch.float16))
    assert not attention._kernel_ok(*_qkv(S, 64, torch.float32))
    # q and k/v of different lengths
    q, k, v = _qkv(S, 64)
    assert not attention._kernel_ok(q, k[:, :, : S - 1], v[:, :, : S - 1])
    assert not attention._kernel_ok(q, k, v[:, :1])
    # nothing to compute
    assert not attention._kernel_ok(q[:0], k[:0], v[:0])
    # not [B, H, S, D]
    assert not attention._kernel_ok(q[0], k[0], v[0])
