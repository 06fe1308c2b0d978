"""Host check of the split-R TN GEMM workgroup map (gemm_tn_map.h).

The header is plain C++ shared by the launch code and the kernels; a small
stand-alone program (tests/csrc/gemm_tn_map_check.cpp) built with the
system C++ compiler checks: both modes are bijections onto (tile, slice)
for ntile 1..40 x splitr 1..64, mode 0 is the old tile-major arithmetic,
the modes coincide at splitr == 1, and at the four per-layer dW shapes of
the flagship step the slice-major map's per-XCD distinct-strip counts are
131 / 189 / 131 / 174 (tile-major: 345 / 483 / 284 / 322).
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc", "gemm_tn_map_check.cpp")
INC = os.path.join(REPO, "easydist_amd", "ops", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_gemm_tn_map_host_check(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler found")
    exe = str(tmp_path / "gemm_tn_map_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", INC,
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK"), r.stdout
