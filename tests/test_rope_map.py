"""Host check of the RoPE kernel's work-item map (rope_map.h).

The header is plain C++ shared by the launch code and the kernel; a small
stand-alone program (tests/csrc/rope_map_check.cpp) built with the system C++
compiler decodes every item of every block pass at the shapes of
tests/test_gpu_rope.py (strided inputs included) and a few more, and checks
it against a plain 64-bit decode: input, output and table offsets, bounds and
16-byte alignment of every vector the kernel touches, and that the items
write every output vector exactly once. Shapes of more than 2^31 elements
are sampled for offsets that wrap.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc", "rope_map_check.cpp")
INC = os.path.join(REPO, "easydist_amd", "ops", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_rope_map_host_check(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler found")
    exe = str(tmp_path / "rope_map_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", INC,
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK"), r.stdout
