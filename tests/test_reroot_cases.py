"""The oracle's restatement of Tree::reroot (oracle/pm_oracle.cpp, reroot_dump) against the hand-derived
dumps of tests/_reroot_cases.py, and the edge-case builders of the GPU tests on the CPU: each builder's stated
property holds in the oracle's dump, and rerooting leaves every FASTA record unchanged."""
import os

import pytest

import _reroot_cases as cases
from _panmat import panmat_from_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_oracle_matches_hand_case(oracle, name):
    case, leaf, want = cases.HAND[name]
    assert oracle.reroot(cases.hand_panmat(case), leaf) == want


def test_hand_cases_cover_every_record_kind():
    """The hand texts themselves: BI, BI inverted, BD, BD with the inversion flag, and NS / ND / NI both as
    main and as gap-slot records (ND and NI)."""
    text = "".join(want for _, _, want in cases.HAND.values())
    assert cases.b_lines(text.replace("newick", "x\tnewick")) >= {("1", "0"), ("1", "1"), ("0", "0"), ("0", "1")}
    kinds = set()
    for line in text.splitlines():
        f = line.split("\t")
        if len(f) > 1 and f[1] == "N":
            kinds.add((f[4] != "-1", int(f[5]) & 15))
    assert kinds == {(False, 0), (False, 1), (False, 2), (True, 1), (True, 2)}


@pytest.mark.parametrize("name", list(cases.EDGE))
def test_edge_case_holds_its_property(oracle, name):
    case = cases.EDGE[name]()
    dump = oracle.reroot(case.pm, case.leaf)
    assert not dump.startswith("#error"), dump
    case.check(dump)
    back = panmat_from_dump(dump, case.pm)
    before = oracle.fasta(case.pm, True)
    assert oracle.fasta(back, True) == before
    assert oracle.fasta(back, False) == oracle.fasta(case.pm, False)
    # the aligned records hold every canonical column but the blocks' end sentinels
    record = before.split(">")[1].partition("\n")[2].replace("\n", "")
    assert len(record) + len(case.pm.blocks) == case.columns


def test_unary_root_and_missing_block_id(oracle):
    pm, leaf = cases.unary_root()
    assert oracle.reroot(pm, leaf) == "#error\tunary root\n"
    pm, leaf = cases.block_ids_0_2()
    assert oracle.reroot(pm, leaf) == "#error\tBlock with id 1 -1 not found!\n"


def test_chunk_sizes_cut_a_record():
    """The sizes the GPU test sets (PM_OPT_REROOT_CHUNK_SITES): 1, 2, 7, 64 and the column count minus one, itself
    and plus one; runs() asserts on the dump that sizes 7 and 64 cut a record."""
    c = cases.RUN_COLUMNS
    assert cases.CHUNK_SIZES == (1, 2, 7, 64, c - 1, c, c + 1) and c % 7 and c % 64
    assert "#define PM_OPT_REROOT_CHUNK_SITES 27\n" in open(os.path.join(ROOT, "include", "panman_gpu.h")).read()
