"""Host check of the attention workgroup map (attn_block_map.h).

The header is plain C++ shared by the launch code and the kernels; a small
stand-alone program (tests/csrc/attn_block_map_check.cpp) built with the
system C++ compiler checks, for both modes and both heavy_last_index
settings: bijection for nblk 1..40 x nbh 1..70, equal causal weight per
`L % 8` group and head locality in balanced mode at nblk {8,16,24} x nbh
{8,96,256,768}, the 16/9 legacy imbalance at (8, 768), and that legacy
mode is (L % nblk, L / nblk).
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc", "attn_block_map_check.cpp")
INC = os.path.join(REPO, "easydist_amd", "ops", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_attn_block_map_host_check(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler found")
    exe = str(tmp_path / "attn_block_map_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", INC,
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK"), r.stdout
