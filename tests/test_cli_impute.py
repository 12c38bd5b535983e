"""`panmanUtils --impute` (src/panmanUtils.cpp:328-354) end to end on a two-tree file: the stdout lines, the
written PanMAN read back against the restatement's image (tests/_impute_ref.py), the ./info/<o>_<i>.moves files
against its plans, -D, and a missing -o."""
import os
import re
import subprocess

import numpy as np
import pytest

import _impute_cases as cases
import _impute_ref as ref
from _panmat import tree_dump
from _subnet_ref import sorted_blocks, to_lists
from _trees import parse_newick
from panman_amd.panmat import PanmanFile, write_panman

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "panmanUtils")


def _run(args, cwd):
    if not os.path.exists(CLI):
        pytest.fail(f"{CLI} missing: run `make`")
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def two_trees(tmp_path_factory):
    """A file of two planted trees (branch lengths in eighths), and each tree as the loader hands it over: the
    internal nodes named node_<k>, every list grouped by block."""
    directory = tmp_path_factory.mktemp("impute_cli")
    nwk = "".join(f"(s{i}," for i in range(19)) + "s19" + ")" * 19 + ";"
    names, off, idx, root = parse_newick(nwk)
    pms = [cases.planted(np.random.default_rng(seed), names, off, idx, root, winners=3, losers=1) for seed in (11, 12)]
    path = str(directory / "in.panman")
    write_panman(path, pms)
    f = PanmanFile(path)
    try:
        loaded = [to_lists(f.to_panmat(i)) for i in range(2)]
    finally:
        f.close()
    return directory, path, loaded


def _expect(loaded, distance):
    return [ref.impute(pm, distance) for pm in loaded]


@pytest.mark.parametrize("flags,distance", [([], 5), (["-D", "0"], 0), (["--max-insertion-impute-distance=-1"], -1)])
def test_impute_command(two_trees, flags, distance):
    directory, path, loaded = two_trees
    want = _expect(loaded, distance)
    if distance == 5:
        assert sum(w[2]["moves_found"] for w in want) >= 2 and sum(w[2]["imputed_bases"] for w in want) > 0
    if distance == -1:
        assert all(w[2]["pairs"] == 0 for w in want)
    out = f"imp{distance + 1}"
    r = _run(["-I", path, "--impute", "-o", out] + flags, directory)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    at = 0
    for _, _, stats in want:
        k, a, m = stats["imputed_bases"], stats["insertion_nodes"], stats["moves_found"]
        at = lines.index(f"Imputed {k}/{k} SNPs/MNPs to N", at)
        assert lines[at + 1] == f"Moved 0/{a} nodes with insertions to N ({m} moves found, not applied)"
        at += 2
    assert re.search(r"\nImputation time: \d+ nanoseconds\n", r.stdout)
    g = PanmanFile(str(directory / "panman" / (out + ".panman")))
    try:
        assert len(g) == 2
        for i in range(2):
            assert sorted_blocks(tree_dump(g, i)) == ref.dump(want[i][0])
    finally:
        g.close()
    for i in range(2):
        assert (directory / "info" / f"{out}_{i}.moves").read_text() == want[i][1]


def test_distance_changes_the_plan(two_trees):
    _, _, loaded = two_trees
    assert [w[1] for w in _expect(loaded, 5)] != [w[1] for w in _expect(loaded, -1)]


def test_missing_output_file(two_trees):
    directory, path, _ = two_trees
    r = _run(["-I", path, "--impute"], directory)
    assert r.returncode != 0 and "Output file not provided!" in r.stderr
    r = _run(["-I", path, "--impute", "-o", "bad", "-D", "five"], directory)
    assert r.returncode != 0 and "max-insertion-impute-distance" in r.stderr
    assert not (directory / "panman" / "bad.panman").exists()
