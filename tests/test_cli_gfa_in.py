"""bin/panmanUtils takes --input-gfa / -G (src/panmanUtils.cpp:1326-1362); the construction itself
needs the GPU (tests/test_gpu_gfa_in.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "panmanUtils")


def _run(args, cwd):
    if not os.path.exists(CLI):
        pytest.fail(f"{CLI} missing: run `make`")
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def test_help_lists_input_gfa(tmp_path):
    r = _run(["-h"], tmp_path)
    assert r.returncode == 0 and "--input-gfa [ -G ] arg" in r.stdout


def test_input_gfa_needs_a_newick(tmp_path):
    for flag in ("-G", "--input-gfa"):
        r = _run([flag, "x.gfa", "-o", "out"], tmp_path)
        assert r.returncode != 0
        assert "newick string not provided" in r.stderr
        assert "not part of the GPU path" not in r.stderr and "unrecognised option" not in r.stderr


def test_input_gfa_needs_an_output_file(tmp_path):
    r = _run(["-G", "x.gfa", "-N", "x.nwk"], tmp_path)
    assert r.returncode != 0 and "Output file not provided!" in r.stderr
    assert "--input-gfa [ -G ] arg" in r.stdout   # the option table, as the reference prints it
