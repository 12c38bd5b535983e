"""panmanUtils --printMutations / -p (src/panmanUtils.cpp:1008-1071) against tests/_mutations_ref.py:
to stdout and to ./info/<o>.mutations on a two-tree file with -d 1, the timing line, the --input-file
error; and the ABI: both symbols and option id 26."""
import ctypes
import os
import subprocess

import pytest

import panman_amd
import _mutations_ref
from _mutations_cases import issue_case, random_case
from panman_amd.panmat import PanmanFile, write_panman

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "panmanUtils")


def _run(args, cwd):
    if not os.path.exists(CLI):
        pytest.fail(f"{CLI} missing: run `make`")
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def _two_trees(tmp_path):
    """A file of two trees; the reference's text of the second as the file holds it (a loaded tree
    numbers its nodes in Newick order and names its internal nodes anew)."""
    path = str(tmp_path / "in.panman")
    write_panman(path, [issue_case()[0], random_case(20, 2)])
    f = PanmanFile(path)
    want = _mutations_ref.print_mutations(f.to_panmat(1))[0]
    first = _mutations_ref.print_mutations(f.to_panmat(0))[0]
    f.close()
    return path, want, first


def test_abi_names_the_call_and_the_option():
    text = open(os.path.join(ROOT, "include", "panman_gpu.h")).read()
    assert "#define PM_OPT_MUTATIONS_BATCH_BYTES 26\n" in text
    assert "int pm_print_mutations(" in text and "int pm_print_mutations_fd(" in text
    lib = ctypes.CDLL(panman_amd.LIB_PATH)
    assert lib.pm_print_mutations and lib.pm_print_mutations_fd


def test_input_file_form_is_refused(tmp_path):
    path = str(tmp_path / "in.panman")
    write_panman(path, [issue_case()[0]])
    (tmp_path / "nodes.txt").write_text("a\n")
    r = _run(["-I", path, "-p", "--input-file", "nodes.txt"], tmp_path)
    assert r.returncode == 1 and "not built" in r.stderr and "--input-file" in r.stderr
    r = _run(["-h"], tmp_path)
    assert "--printMutations [ -p ]" in r.stdout


@pytest.mark.gpu
def test_print_mutations_command(tmp_path):
    path, want, first = _two_trees(tmp_path)
    assert want.count(" > ") > 20 and want != first
    r = _run(["-I", path, "-p", "-d", "1", "-o", "x"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "info" / "x.mutations").read() == want
    assert "\nMutation extract execution time: " in r.stdout and r.stdout.rstrip().endswith("nanoseconds")
    assert "Substitutions:" not in r.stdout
    r = _run([path, "--printMutations", "--treeID", "1"], tmp_path)   # stdout
    assert r.returncode == 0, r.stderr
    assert want + "\nMutation extract execution time: " in r.stdout
    r = _run(["-I", path, "-p"], tmp_path)                            # the tree defaults to 0
    assert r.returncode == 0, r.stderr
    assert first + "\nMutation extract execution time: " in r.stdout
    r = _run(["-I", path, "-p", "-d", "2"], tmp_path)
    assert r.returncode == 1 and "TreeID out of range" in r.stderr
