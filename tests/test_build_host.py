"""The host-only half of the construction drivers (panman_amd/csrc/pm_build.h: the code table
and its packings, a topology's arrays, the NucMut run rule, the block-mutation records) as a
stand-alone program under AddressSanitizer (with its leak checker) and UBSan:
tests/build_host_check.cpp, built with g++ and run as a child process.  CPU only; nothing is
loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_build_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "build_host_check")
    src = [os.path.join(ROOT, "tests", "build_host_check.cpp"), os.path.join(ROOT, "panman_amd", "csrc", "pm_newick.cpp")]
    built = subprocess.run(["g++"] + FLAGS + src + ["-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
