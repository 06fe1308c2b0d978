"""Host check of the attention workgroup map at the block counts of the
64-key dkv geometry (EASYDIST_DKV_GEOM=1: nblk = ceil(S / 64)).

tests/csrc/attn_block_map_geom_check.cpp reuses the predicates of
tests/csrc/attn_block_map_check.cpp on (nblk, nbh) pairs given on the
command line: the bench shape (S = 1024: nblk 16, 768 heads), S = 2048 at
256 heads, and the small GPU-test shapes (nblk 2, 4, 5, 6 with 2, 6 and 9
heads).  Bijection for all; ascending block order within a head (the
causal-heavy block first); equal weight per XCD group and whole heads per
group where the head count is a multiple of 8.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(REPO, "easydist_amd", "ops", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


SRC =os.path.join(REPO, "tests", "csrc", "attn_block_map_geom_check.cpp")

PAIRS = [(16, 768), (32, 256), (16, 8), (18, 768),
         (2, 6), (2, 9), (4, 6), (4, 9), (5, 6), (5, 9),
         (2, 2), (4, 2), (6, 6)]


def test_attn_block_map_dkv_geom(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler found")
    exe = str(tmp_path / "attn_block_map_geom_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", INC,
                    "-I", os.path.dirname(SRC), SRC, "-o", exe], check=True)
    args = [str(x) for p in PAIRS for x in p]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK %d pairs" % len(PAIRS)), r.stdout
