"""GPU N imputation (pm_impute; Tree::imputeNs, src/impute.cpp:4-337 up to the plan of moves) against the
plain-Python restatement tests/_impute_ref.py, which walks the tree with one running sequence and undoes every
list on the way up, and builds every candidate's MutationList by concatenation -- where pm_impute reads replayed
rows at the parent and folds (node, candidate) pairs' path steps once per coordinate.  The image (a tree_dump
with sorted blocks), the plan text and the stats are compared whole; the kernels' edges are hand-built at the
smallest sizes where they can go wrong."""
import os

import numpy as np
import pytest

import _impute_cases as cases
import _impute_ref as ref
import panman_amd
from _panmat import tree_dump
from _subnet_ref import sorted_blocks
from _trees import names_for, parse_newick, to_newick
from panman_amd._lib import header_symbols, load
from panman_amd.panmat import PanMAT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, C, G, T, N = cases.A, cases.C, cases.G, cases.T, cases.N
NS, ND, NI, S = cases.NS, cases.ND, cases.NI, cases.NSNPS
PLANTED_SEED = {"join40": 1, "caterpillar70": 1}


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    e.close()


def _gpu(engine, pm, distance=5):
    f, plan, stats = engine.impute(pm, distance)
    try:
        return sorted_blocks(tree_dump(f)), plan, stats
    finally:
        f.close()


def _check(engine, pm, distance=5, want=None):
    """The GPU's (image, plan, stats), after they matched the restatement's."""
    got = _gpu(engine, pm, distance)
    out, plan, stats = want if want is not None else ref.impute(pm, distance)
    assert got[0] == ref.dump(out)
    assert got[1] == plan
    assert got[2] == stats
    return got


# ---- the hand cases ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_hand_cases(engine, name):
    _check(engine, cases.HAND[name]())   # (branch_length is None in all of them)


@pytest.mark.parametrize("length,distance", [(0.5, 0), (0.5, -1), (1.0, 1), (1.0, 2), (1.0, 3)])
def test_distance_edges(engine, length, distance):
    _check(engine, cases.sibling_donor(length), distance)
    _check(engine, cases.grandparent_donor(length), distance)


# ---- planted random cases ---------------------------------------------------------------------------------

def _caterpillar(leaves):
    nwk = "".join(f"(s{i}," for i in range(leaves - 1)) + f"s{leaves - 1}" + ")" * (leaves - 1) + ";"
    return parse_newick(nwk)


def _random_join(leaves, seed):
    off, idx, root = panman_amd.random_join_tree(leaves, seed=seed)
    return parse_newick(to_newick(off, idx, root, names_for(off)))


def planted_case(which):
    names, off, idx, root = _random_join(40, 5) if which == "join40" else _caterpillar(70)
    return cases.planted(np.random.default_rng(PLANTED_SEED[which]), names, off, idx, root)


def assert_covers(pm, plan):
    """At least 3 winners, 1 attempt with candidates and no winner, 1 attempt with no candidate, and 1 NS record
    that is partly N below the root."""
    heads = [l.split("\t") for l in plan.splitlines() if l.split("\t")[1] not in ("B", "N")]
    assert sum(h[3] != "." for h in heads) >= 3
    assert sum(h[3] == "." and int(h[2]) > 0 for h in heads) >= 1
    assert sum(int(h[2]) == 0 for h in heads) >= 1
    partial = 0
    for v in range(pm.num_nodes):
        for m in pm.nuc_muts[v]:
            codes = [ref.code(m, i) for i in range(ref.length(m))]
            partial += v != pm.root and ref.mtype(m) == NS and N in codes and any(c != N for c in codes)
    assert partial >= 1


@pytest.fixture(scope="module", params=["join40", "caterpillar70"])
def random_case(request):
    """The planted PanMAT and the restatement's answers at the three distances, computed once; the coverage is
    asserted on the restatement alone, before the GPU is asked."""
    pm = planted_case(request.param)
    want = {d: ref.impute(pm, d) for d in (0, 2, 5)}
    for d in want:
        assert_covers(pm, want[d][1])
    return pm, want


@pytest.mark.parametrize("distance", [0, 2, 5])
def test_planted_random(engine, random_case, distance):
    pm, want = random_case
    _check(engine, pm, distance, want[distance])


def test_batches_do_not_change_the_result(engine, random_case):
    pm, want = random_case
    results = []
    try:
        for entries in (1, 97, 1 << 25):   # every pair alone; cuts mid-list; the default
            engine.set_impute_batch_entries(entries)
            results.append(_check(engine, pm, 5, want[5]))
    finally:
        engine.set_impute_batch_entries(1 << 25)
    assert results[0] == results[1] == results[2]


# ---- kernel edges -----------------------------------------------------------------------------------------

def _long(block_len=400):
    """The seven-node tree with block 0 of `block_len` bases (ACGT repeated) and block 1 as in cases.base()."""
    pm = PanMAT(["r", "p", "a", "b", "q", "c", "d"], np.array([0, 2, 4, 4, 4, 6, 6, 6], np.int32),
                np.array([1, 4, 2, 3, 5, 6], np.int32), 0)
    pm.add_block(0, "ACGT" * (block_len // 4))
    pm.add_gaps(0, [(3, 4), (7, 4)])
    pm.add_block(1, "GGGGCCCC")
    pm.add_gaps(1, [(2, 8)])
    pm.add_block_mut(0, 0, True, False)
    pm.add_block_mut(0, 1, True, False)
    return pm


@pytest.mark.parametrize("records", [255, 256, 257])
def test_records_at_the_block_edge(engine, records):
    """`records` records in the tree, one per lane: a's first and last are erased (an NSNPS of N), every third
    one between too, and b's whole list goes."""
    pm = _long()
    a, b = pm.index("a"), pm.index("b")
    pm.add_nuc_mut(b, 0, 0, -1, S, [N])
    pm.add_nuc_mut(b, 0, 1, -1, NS, [N, N])
    k = records - 2
    for i in range(k):
        erased = i == 0 or i == k - 1 or i % 3 == 0
        pm.add_nuc_mut(a, 0, i, -1, S, [N if erased else G])
    assert sum(len(l) for l in pm.nuc_muts) == records
    image, _, stats = _check(engine, pm)
    assert stats["imputed_bases"] == 3 + sum(1 for i in range(k) if i == 0 or i == k - 1 or i % 3 == 0)
    assert "\nb\tN\t" not in image


def test_winner_regroups_across_the_six_base_cut(engine):
    """Eight slots fold to eight substitutions: NS of 6 (its N imputed away, five SNPs back) and NS of 2; cells in
    block 0 and block 1, so the ranks cross a block base."""
    pm = cases.base()
    a, b = pm.index("a"), pm.index("b")
    pm.add_nuc_mut(a, 1, 2, 0, NI, [N, A, C, G, T, A])
    pm.add_nuc_mut(a, 1, 2, 6, NI, [C, G])
    pm.add_nuc_mut(a, 0, 9, -1, S, [G])
    pm.add_nuc_mut(b, 1, 2, 0, NI, [T, T, T, T, T, T])
    pm.add_nuc_mut(b, 1, 2, 6, NI, [T, T])
    _, plan, stats = _check(engine, pm)
    lines = plan.splitlines()
    assert lines[0] == "a\t1\t1\tb\t1\t0"          # 9 bases before; 1 + 5 + 2 after the N went
    assert lines[1] == "a\tN\t0\t9\t-1\t19\t400000"
    assert [l.split("\t")[4] for l in lines[2:]] == ["1", "2", "3", "4", "5", "6"]
    assert lines[-1] == "a\tN\t1\t2\t6\t32\t240000"
    assert stats["moves_found"] == 1


def _deep():
    """r -> (A, B); A -> (A1, la); A1 -> (A2, l1); A2 -> (x, l2); B -> (B1, lb); B1 -> (y, l3)."""
    names = ["r", "A", "A1", "A2", "x", "l2", "l1", "la", "B", "B1", "y", "l3", "lb"]
    kids = {"r": ["A", "B"], "A": ["A1", "la"], "A1": ["A2", "l1"], "A2": ["x", "l2"], "B": ["B1", "lb"], "B1": ["y", "l3"]}
    off, idx = [0], []
    for n in names:
        idx += [names.index(k) for k in kids.get(n, [])]
        off.append(len(idx))
    pm = PanMAT(names, np.array(off, np.int32), np.array(idx, np.int32), 0)
    pm.add_block(0, "ACGTACGTAC")
    pm.add_gaps(0, [(3, 4), (7, 4)])
    pm.add_block_mut(0, 0, True, False)
    return pm


def test_paths_of_one_and_of_seven_steps(engine):
    """x's parent A2 holds the run: a path of one step, x's own list, improvement 0.  y holds it too: y, B1, B
    upward (inverted), A, A1, A2 downward, then x -- seven steps, both directions, substitutions on both."""
    pm = _deep()
    ix = pm.index
    pm.add_nuc_mut(ix("x"), 0, 3, 0, NI, [N, N, N])
    pm.add_nuc_mut(ix("A2"), 0, 3, 0, NI, [A, C, G])
    pm.add_nuc_mut(ix("y"), 0, 3, 0, NI, [A, C, G])
    for k, n in enumerate(["y", "B", "A1"]):   # (three more bases on the path than the run saves: 3 - 3 = 0 wins)
        pm.add_nuc_mut(ix(n), 0, k, -1, S, [T])
    trace = {}
    want = ref.impute(pm, 5, trace)
    assert trace["x"] == ["A2", "y"]
    _, plan, _ = _check(engine, pm, 5, want)
    assert plan.splitlines()[0] == "x\t1\t2\tA2\t0\t0"
    # without the parent's copy the long path is the only one
    pm.nuc_muts[ix("A2")] = []
    trace = {}
    want = ref.impute(pm, 5, trace)
    assert trace["x"] == ["y"]
    _, plan, _ = _check(engine, pm, 5, want)
    # y's T goes back to A and B's to C (both left upward), A1's T stays: one NS of 3
    assert plan.splitlines() == ["x\t1\t1\ty\t0\t0", "x\tN\t0\t0\t-1\t48\t128000"]


def test_no_n_anywhere(engine):
    pm = cases.base()
    cases.mut(pm, "a", 0, 3, 0, NI, [A, C])
    cases.mut(pm, "b", 0, 1, -1, NS, [G, G])
    cases.mut(pm, "c", 0, 5, -1, ND, [0, 0])
    image, plan, stats = _check(engine, pm)
    assert image == ref.dump(pm) and plan == ""
    assert stats == {"imputed_bases": 0, "insertion_nodes": 0, "moves_found": 0, "pairs": 0}
    # only the replay launches: as many launches as for the root's N alone (never visited), fewer than with one N
    engine.set_profiling(True)
    try:
        engine.kernel_times()
        _gpu(engine, pm)
        replay_only = engine.kernel_times()[1][3]
        _gpu(engine, cases.root_n())
        assert engine.kernel_times()[1][3] == replay_only
        _gpu(engine, cases.nsnps_n())
        assert engine.kernel_times()[1][3] > replay_only
    finally:
        engine.set_profiling(False)


# ---- errors and the binding -------------------------------------------------------------------------------

def test_a_cell_written_twice(engine):
    pm = cases.base()
    cases.mut(pm, "a", 0, 1, -1, NS, [A, N])
    cases.mut(pm, "a", 0, 2, -1, S, [G])
    with pytest.raises(panman_amd.PanmanError, match="rc=-4.*a cell written twice in one list"):
        engine.impute(pm)
    # the same cell in two nodes' lists is no such thing
    pm.nuc_muts[pm.index("a")].pop()
    cases.mut(pm, "b", 0, 2, -1, S, [G])
    _check(engine, pm)


def test_secondary_blocks(engine):
    pm = cases.sibling_donor()
    pm.add_nuc_mut(pm.index("d"), 0, 5, -1, S, [C], secondary=3)
    with pytest.raises(panman_amd.PanmanError, match="rc=-4.*secondary blocks"):
        engine.impute(pm)


def test_cell_outside_its_block_or_slots(engine):
    pm = cases.sibling_donor()
    cases.mut(pm, "d", 0, 3, 3, NI, [N, A])          # slots 3 and 4 of 4
    with pytest.raises(panman_amd.PanmanError, match="rc=-1"):
        engine.impute(pm)
    pm = cases.sibling_donor()
    cases.mut(pm, "d", 0, 9, -1, NS, [N, A, C])      # positions 9, 10 (the sentinel) and 11
    with pytest.raises(panman_amd.PanmanError, match="rc=-1"):
        engine.impute(pm)


def test_length_nibble_above_six(engine):
    pm = cases.sibling_donor()
    pm.add_nuc_mut_raw(pm.index("d"), 0, 0, -1, (7 << 4) | NS, 0x111111)
    with pytest.raises(panman_amd.PanmanError, match="rc=-1.*nucleotide run longer than 6"):
        engine.impute(pm)


def test_records_the_walk_and_the_fold_read_differently(engine):
    """A deletion that carries codes (the walk would write them, the rows hold '-') and a single-base record whose
    length nibble is not 1 (length() in impute.cpp, 1 in consolidateNucMutations) are refused."""
    pm = cases.sibling_donor()
    pm.add_nuc_mut_raw(pm.index("d"), 0, 0, -1, (2 << 4) | ND, 0x120000)
    with pytest.raises(panman_amd.PanmanError, match="rc=-4.*a deletion that carries codes"):
        engine.impute(pm)
    pm = cases.sibling_donor()
    pm.add_nuc_mut_raw(pm.index("d"), 0, 0, -1, (2 << 4) | S, 0x120000)
    with pytest.raises(panman_amd.PanmanError, match="rc=-1.*single-base record whose length is not 1"):
        engine.impute(pm)


def test_raising_block_sequence(engine):
    pm = cases.grandparent_donor()
    pm.add_block_mut(pm.index("c"), 1, True, False)    # inverted on the path: a deletion ...
    pm.add_block_mut(pm.index("p"), 1, False, False)   # ... followed by p's deletion
    with pytest.raises(panman_amd.PanmanError, match="rc=-1.*Block deletion followed by inversion or deletion doesn't make sense"):
        engine.impute(pm)
    with pytest.raises(ValueError, match="Block deletion followed by inversion or deletion"):
        ref.impute(pm)


def test_symbol_is_exported_and_bound():
    assert "pm_impute" in header_symbols() and hasattr(load(), "pm_impute")
    assert "PM_OPT_IMPUTE_BATCH_ENTRIES 29" in open(os.path.join(ROOT, "include", "panman_gpu.h")).read()
