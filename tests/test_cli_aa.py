"""panmanUtils --aa-translation (src/panmanUtils.cpp:895-938): the argument errors run here, the
command itself against tests/_aa_ref.py needs the GPU."""
import os
import subprocess

import pytest

import _aa_ref
from _aa_cases import issue_case, random_case
from panman_amd.panmat import PanmanFile, write_panman

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "panmanUtils")


def _run(args, cwd):
    if not os.path.exists(CLI):
        pytest.fail(f"{CLI} missing: run `make`")
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def _written(path, pm, start, end):
    """Write the PanMAT; the reference result of the file's tree (a loaded tree numbers its nodes
    in Newick order: the same lines in another order)."""
    write_panman(path, [pm])
    f = PanmanFile(path)
    want = _aa_ref.aa(f.to_panmat(0), start, end)
    f.close()
    strings = lambda text: sorted(line.partition("\t")[2] for line in text.split("\n"))   # (it also renames internal nodes)
    assert strings(want[0]) == strings(_aa_ref.aa(pm, start, end)[0])
    return want


def test_argument_errors(tmp_path):
    pm, _, _, _, _ = issue_case()
    path = str(tmp_path / "in.panman")
    write_panman(path, [pm])
    r = _run(["-h"], tmp_path)
    assert "--aa-translation" in r.stdout and "--start [ -x ]" in r.stdout and "--end [ -y ]" in r.stdout
    r = _run(["-I", path, "--aa-translation", "-x", "0", "-y", "9"], tmp_path)
    assert r.returncode == 1 and "TreeID not provided!" in r.stderr
    r = _run(["-I", path, "--aa-translation", "-d", "3", "-x", "0", "-y", "9"], tmp_path)
    assert r.returncode == 1 and "TreeID out of range" in r.stderr
    for args in (["-x", "0"], ["-y", "9"], []):
        r = _run(["-I", path, "--aa-translation", "-d", "0"] + args, tmp_path)
        assert r.returncode == 1 and "Start/End Coordinate not provided" in r.stdout
    r = _run(["-I", path, "--aa-translation", "-d", "0", "-x"], tmp_path)
    assert r.returncode == 1 and "required argument" in r.stderr
    r = _run([path, "--vcf"], tmp_path)   # still outside the GPU path
    assert r.returncode != 0 and "not part of the GPU path" in r.stderr


@pytest.mark.gpu
def test_aa_translation_command(tmp_path):
    pm, start, end = random_case(30, 17, 4)
    path = str(tmp_path / "in.panman")
    text, ref_codons, _ = _written(path, pm, start, end)
    assert text.count("\n") > 5
    r = _run(["-I", path, "--aa-translation", "-d", "0", "-x", str(start), "-y", str(end), "-o", "t"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "info" / "t.tsv").read() == text
    assert f"\n{ref_codons} {ref_codons} {ref_codons}\n" in r.stdout
    assert "\nAmino Acid translate execution time: " in r.stdout and r.stdout.rstrip().endswith("nanoseconds")
    r = _run([path, "--aa-translation", "--treeID", "0", "--start", str(start), "--end", str(end)], tmp_path)   # stdout
    assert r.returncode == 0, r.stderr
    assert f"\n{ref_codons} {ref_codons} {ref_codons}\n" + text + "\nAmino Acid translate execution time: " in r.stdout
    r = _run(["-I", path, "--aa-translation", "-d", "0", "-x", "5", "-y", "5"], tmp_path)
    assert r.returncode == 1 and "End coordinate must be greater than start" in r.stderr
