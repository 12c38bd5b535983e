"""The host-only text plumbing of the extraction drivers (panman_amd/csrc/pm_text.h: the text
collector behind pm_vcf / pm_maf / pm_gfa and the batch cutter) as a stand-alone program under
AddressSanitizer (with its leak checker) and UBSan: tests/text_host_check.cpp, built with g++ and
run as a child process.  CPU only; nothing is loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_text_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "text_host_check")
    src = os.path.join(ROOT, "tests", "text_host_check.cpp")
    built = subprocess.run(["g++"] + FLAGS + [src, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
