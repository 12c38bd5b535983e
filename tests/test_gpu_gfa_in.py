"""pm_gfa_build on the GPU: the hand cases and random unambiguous inputs against the Python
restatement (tests/_gfa_in_ref.py, pinned to the reference's source by tests/test_gfa_in_ref.py),
the order-independent property that the built PanMAN replays what every "P" line spells (also on
inputs whose block order the reference leaves to library internals), the round trip through pm_gfa,
batches, limits, the facade, the CLI."""
import os
import subprocess

import numpy as np
import pytest

import panman_amd
from _gfa_cases import random_case
from _gfa_in_ref import (AMBIGUOUS_SEEDS, UNAMBIGUOUS_SEEDS, build, panmat_blocks, panmat_records, random_gfa)
from _gfa_ref import gfa_to_sequences
from _panmat import parse_records
from _trees import to_newick
from test_gfa_in_ref import CASE1, CASE2, CASE3, gfa_text
from test_gfa_ref import ROUND_TRIP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "panmanUtils")
BI, BD = 1, 0

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    e.close()


def _built(engine, text, newick):
    f = engine.gfa_build(text, newick)
    try:
        return f.to_panmat(0)
    finally:
        f.close()


def _replays_its_paths(engine, pm, text):
    """Every tip with a "P" line replays to what the line spells; every aligned record is as long as
    the blocks together.  Returns the number of tips compared."""
    want = gfa_to_sequences(text)
    got = parse_records(engine.fasta(pm, False))
    tips = [pm.names[v] for v in pm.leaves()]
    assert sorted(got) == sorted(tips)
    compared = [t for t in tips if t in want]
    for t in compared:
        assert got[t] == want[t], t
    total = sum(len(s) for s in panmat_blocks(pm))
    if total:
        assert {len(r) for r in parse_records(engine.fasta(pm, True)).values()} == {total}
    return len(compared)


HAND = {
    "skipped_segment": (CASE1, ["ACG", "TT", "GAC"], {("node_1", 0, BI, 0), ("node_1", 2, BI, 0), ("a", 1, BI, 0)}),
    "rearrangement": (CASE2, ["TTA", "ACGT", "AAC", "CCG", "GGT", "TTA", "ACGT"],
                      {("node_1", 2, BI, 0), ("node_1", 3, BI, 0), ("node_1", 4, BI, 0), ("a", 5, BI, 0), ("a", 6, BI, 0),
                       ("b", 0, BI, 0), ("b", 1, BI, 0)}),
    "reverse_strand": (CASE3, ["ACG", "TTG"], {("node_1", 0, BI, 0), ("node_1", 1, BI, 0), ("b", 1, BD, 1)}),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_case(engine, oracle, name):
    (text, newick), blocks, records = HAND[name]
    pm = _built(engine, text, newick)
    assert panmat_blocks(pm) == blocks
    assert panmat_records(pm) == records
    ref = build(text, newick)
    assert ref.blocks == blocks and ref.records(oracle) == records
    assert len(pm._arrays["gap_primary"]) == 0 and len(pm._arrays["nuc_mut_primary"]) == 0
    assert _replays_its_paths(engine, pm, text) == 2


@pytest.mark.parametrize("seed", UNAMBIGUOUS_SEEDS)
def test_random_unambiguous_matches_the_reference(engine, oracle, seed):
    text, newick = random_gfa(seed)
    ref = build(text, newick)
    pm = _built(engine, text, newick)
    assert pm.names == ref.names and (pm.child_offsets == ref.off).all() and (pm.child_index == ref.idx).all()
    assert panmat_blocks(pm) == ref.blocks
    assert panmat_records(pm) == ref.records(oracle)
    a = pm._arrays
    for v in range(pm.num_nodes):   # ascending block id within a node
        ids = a["block_mut_primary"][int(a["block_mut_offsets"][v]):int(a["block_mut_offsets"][v + 1])]
        assert (np.diff(ids) > 0).all()
    assert _replays_its_paths(engine, pm, text) >= 6


@pytest.mark.parametrize("seed,repeats", [(s, False) for s in AMBIGUOUS_SEEDS] + [(s, True) for s in range(100, 108)])
def test_any_input_replays_its_paths(engine, seed, repeats):
    """Inputs on which the reference's block order hangs on library internals (ties, repeated
    segments): whatever the order, every path is replayed."""
    text, newick = random_gfa(seed, repeats=repeats)
    assert _replays_its_paths(engine, _built(engine, text, newick), text) >= 6


@pytest.mark.parametrize("leaves,seed", ROUND_TRIP)
def test_round_trip_through_pm_gfa(engine, leaves, seed):
    """pm_gfa(pm) -> gfa_build with pm's Newick: compared against what the GFA text spells, not against
    pm, so the tips the writer is known to break do not enter."""
    pm = random_case(leaves, seed)
    text = engine.gfa(pm)
    names = [n if pm.child_offsets[v] == pm.child_offsets[v + 1] else "" for v, n in enumerate(pm.names)]
    newick = to_newick(pm.child_offsets, pm.child_index, pm.root, names)
    assert _replays_its_paths(engine, _built(engine, text, newick), text) == leaves


def _dump(pm):
    a = pm._arrays
    keys = ("block_primary", "block_seq_offsets", "block_seq", "block_mut_offsets", "block_mut_primary", "block_mut_info",
            "block_mut_inversion", "gap_primary", "nuc_mut_offsets")
    return pm.names, [a[k].tolist() for k in keys]


def test_batches_give_the_same_panman(engine):
    text, newick = random_gfa(27)
    want = _built(engine, text, newick)
    assert len(panmat_blocks(want)) == 23 and len(want._arrays["block_mut_primary"]) > 23
    try:
        for batch in (1, 5):
            engine.set_gfa_in_batch_sites(batch)
            assert _dump(_built(engine, text, newick)) == _dump(want), batch
    finally:
        engine.set_gfa_in_batch_sites((1 << 24) - 1)
    for bad in (0, 1 << 24):
        with pytest.raises(panman_amd.PanmanError):
            engine.set_gfa_in_batch_sites(bad)


def test_limits(engine):
    segments = {"s1": "ACG", "s2": "TT"}
    cases = {
        "undefined segment s9": (gfa_text(segments, {"a": "s1+,s9+", "b": "s1+"}), "(a,b);"),
        "empty step": (gfa_text(segments, {"a": "s1+,,s2+", "b": "s1+"}), "(a,b);"),
        "no P line": (gfa_text(segments, {}), "(a,b);"),
        "Newick": (gfa_text(segments, {"a": "s1+", "b": "s1+"}), "((a,b);"),
    }
    for what, (text, newick) in cases.items():
        with pytest.raises(panman_amd.PanmanError) as err:
            engine.gfa_build(text, newick)
        assert "rc=-1" in str(err.value) and what in str(err.value), what
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.gfa_build(cases["undefined segment s9"][0], "(a,b);")
    assert "path a" in str(err.value)
    pm = _built(engine, *CASE1)   # the context is still usable
    assert panmat_blocks(pm) == ["ACG", "TT", "GAC"]


def test_paths_without_steps_and_a_tree_without_paths(engine):
    text = "S\ts1\tACGT\nP\ta\t\t*\nP\tb\t\t*\n"
    pm = _built(engine, text, "(a,b);")
    assert panmat_blocks(pm) == [] and panmat_records(pm) == set()
    pm = _built(engine, gfa_text({"s1": "ACGT"}, {"x": "s1+", "y": "s1-"}), "(a,(b,c));")   # no leaf has a path
    assert panmat_blocks(pm) == ["ACGT"] and panmat_records(pm) == set()


# ---- the C++ facade and the command line ---------------------------------------------------------------------

PROGRAM = r"""
#include <fstream>
#include <iostream>
#include "panman_tree.hpp"
int main(int argc, char** argv) {
    try {
        std::ifstream gfa(argv[1]), nwk(argv[2]);
        panman_gpu::Tree t(gfa, nwk, panman_gpu::GFA);
        t.printFASTAUltraFast(std::cout, false);
    } catch (const panman_gpu::Error& e) {
        std::cerr << "Error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gfa_in")
    text, newick = random_gfa(UNAMBIGUOUS_SEEDS[0])
    (d / "x.gfa").write_text(text)
    (d / "x.nwk").write_text(newick + "\n")
    return d, text, newick


def test_facade_builds_from_a_gfa(engine, files):
    d, text, newick = files
    (d / "main.cpp").write_text(PROGRAM)
    lib = os.path.dirname(panman_amd.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(d / "build_gfa"),
                    str(d / "main.cpp"), "-L", lib, "-l:libpanman_amd.so", f"-Wl,-rpath,{lib}"],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([str(d / "build_gfa"), "x.gfa", "x.nwk"], cwd=d, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == engine.fasta(_built(engine, text, newick), False)


def test_cli_input_gfa(engine, files):
    d, text, newick = files
    r = subprocess.run([CLI, "-G", "x.gfa", "-N", "x.nwk", "-o", "out"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "not part of the GPU path" not in r.stderr and "unrecognised option" not in r.stderr
    for line in ("Creating PanMAN from GFA and Newick", "Data load time: ", "Writing PanMAN"):
        assert line in r.stdout
    f = panman_amd.PanmanFile(str(d / "panman" / "out.panman"))
    try:
        loaded = f.to_panmat(0)
    finally:
        f.close()
    want = _built(engine, text, newick)
    assert panmat_blocks(loaded) == panmat_blocks(want) and panmat_records(loaded) == panmat_records(want)
    r = subprocess.run([CLI, "-I", "panman/out.panman", "--fasta"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert engine.fasta(want, False) in r.stdout
