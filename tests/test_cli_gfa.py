"""bin/panmanUtils takes --gfa (src/panmanUtils.cpp:699-732); the extraction itself needs the GPU
(tests/test_gpu_gfa.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "panmanUtils")


def _run(args, cwd):
    if not os.path.exists(CLI):
        pytest.fail(f"{CLI} missing: run `make`")
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def test_help_lists_gfa(tmp_path):
    r = _run(["-h"], tmp_path)
    assert r.returncode == 0 and "--gfa [ -g ]" in r.stdout
    assert "--maf and --gfa" in r.stdout   # the treeID line


def test_gfa_is_part_of_the_gpu_path(tmp_path):
    for flag in ("--gfa", "-g"):
        r = _run(["x.panman", flag], tmp_path)   # no such file: the command is taken, the load fails
        assert r.returncode != 0
        assert "not part of the GPU path" not in r.stderr and "unrecognised option" not in r.stderr
        assert "x.panman" in r.stderr
