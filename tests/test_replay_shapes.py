"""CPU checks of the planted replay inputs (tests/_replay_shapes.py): every builder's census
shows the count that puts it on its kernel edge (the GPU suite, test_gpu_replay_edges.py,
runs the same builders), and wherever the FASTA rules are unambiguous -- every block present
at every leaf, no rotation, inversion or circular offset -- the oracle equals a direct
replay: the consensus with gap slots as '-', the deepest edit on the path wins, 'x' dropped,
'-' dropped when unaligned, wrapped at 70."""
import numpy as np
import pytest

from _panmat import random_panmat
from _replay_shapes import CASES, Census, Layout, block_text, built, direct_fasta, ladder, new_panmat, records, snp
from _trees import names_for, random_tree


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_sits_on_its_edge(name):
    case = CASES[name]
    pm, c = built(name)
    assert c.max_depth == case.depth and c.dfs == case.dfs == (case.depth <= 128)
    assert c.tile == (4096 if case.dfs else 16384)
    if case.groups is not None:
        assert len(c.groups) == case.groups
    if case.dfs and case.rebuild is not None:
        assert (c.rebuilds() > 0) == case.rebuild
    assert c.plain(pm) == case.plain
    case.check(c, pm)


@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n].plain))
def test_oracle_equals_direct_replay(oracle, name):
    pm, c = built(name)
    for aligned in (True, False):
        assert records(oracle.fasta(pm, aligned)) == records(direct_fasta(pm, aligned, c)), aligned


def test_bracketing_pairs_differ_by_one_edit():
    """Each capacity pair is one input and the same input with a single planted edit more."""
    def edits(name):
        pm, _ = built(name)
        return [(v, m) for v, lst in enumerate(pm.nuc_muts) for m in lst], [m for lst in pm.block_muts for m in lst]
    for a, b in (("D_ovr_1024", "D_ovr_1025"), ("D_plain_384", "D_plain_385"), ("D_ovr_64", "D_ovr_65"),
                 ("E_plain_16", "E_plain_17"), ("E_ovr_16", "E_ovr_17")):
        (na, ba), (nb, bb) = edits(a), edits(b)
        assert ba == bb and len(nb) == len(na) + 1 and set(na) <= set(nb), (a, b)
    (na, ba), (nb, bb) = edits("C_replay_6"), edits("C_replay_7")
    assert na == nb and len(bb) == len(ba) + 1 and set(ba) <= set(bb)


def test_layout_with_gap_slots_and_sparse_ids():
    """Position j of a block is preceded by slots[j] gap columns, position len is the sentinel;
    ids that are no block take no columns; the last gap entry of a position wins."""
    pm, lay = new_panmat(ladder(3), [9, 4, 6], ids=[1, 4, 5], gaps={1: [(0, 2), (3, 1)], 5: [(3, 2)]})
    pm.add_gaps(1, [(0, 1), (0, 2)])
    lay = Layout(pm)
    t1, t4, t5 = block_text(1, 5), block_text(4, 3), block_text(5, 3)
    assert lay.cons.decode() == "--" + t1[:3] + "-" + t1[3:] + "x" + t4 + "x" + t5 + "--" + "x"
    assert lay.col_start == [0, 0, 9, 9, 9, 13] and lay.width == [0, 9, 0, 0, 4, 6] and lay.columns == 19
    assert [lay.locate(k) for k in (0, 1, 2, 5, 6, 8, 9, 16, 17, 18)] == [
        (1, 0, 0), (1, 0, 1), (1, 0, -1), (1, 3, 0), (1, 3, -1), (1, 5, -1), (4, 0, -1), (5, 3, 0), (5, 3, 1), (5, 3, -1)]


def test_census_edit_rules():
    """Per node the last edit of a column wins; types 1 and 5 write '-'; types above 5 are
    no-ops; an edit is overriding when some ancestor edits its column, whatever a sibling does."""
    pm, lay = new_panmat(ladder(3), [11])       # ((s0,s1),s2): node_1 root, node_2, leaves
    root, inner = pm.index("node_1"), pm.index("node_2")
    s0, s1, s2 = pm.index("s0"), pm.index("s1"), pm.index("s2")
    snp(pm, lay, root, 2, "G")
    pm.add_nuc_mut(inner, 0, 1, -1, 0, [1, 2, 4])       # columns 1 .. 3: A C G
    pm.add_nuc_mut(inner, 0, 3, -1, 1, [0, 0])          # columns 3 .. 4 deleted: the later edit of 3 wins
    pm.add_nuc_mut(inner, 0, 6, -1, 6, [8])             # no-op type
    pm.add_nuc_mut(s0, 0, 4, -1, 5, [8])
    snp(pm, lay, s1, 7, "T")
    snp(pm, lay, s2, 7, "A")
    c = Census(pm)
    assert c.node_edits[inner] == {1: "A", 2: "C", 3: "-", 4: "-"} and c.edits == 8
    assert c.override[inner] == {2} and c.override[s0] == {4} and not c.override[s1] and not c.override[s2]
    assert c.dfs_order == [s0, s1, s2] and c.dfs_lp == [0, 2, 1] and c.groups == [(0, 3)]
    assert c.path_counts(s0, 0) == (4, 2) and c.max_leaf_tile() == (5, 2)      # s1: one more plain edit


def test_group_cut_on_random_trees():
    """Groups hold at most 16 leaves and 128 distinct path nodes, and are cut only when one more
    leaf would break either bound."""
    rng = np.random.default_rng(5)
    for leaves in (5, 40, 300):
        off, idx, root = random_tree(leaves, rng)
        pm = random_panmat(rng, off, idx, root, names_for(off), blocks=2, mut_rate=0.0, block_rate=0.0, options=False)
        c = Census(pm)
        assert sorted(c.dfs_order) == c.leaves and c.groups[0][0] == 0 and c.groups[-1][1] == len(c.leaves)
        for k, g in enumerate(c.groups):
            assert g[1] - g[0] <= 16 and c.group_nodes(g) <= 128
            if k + 1 < len(c.groups):
                assert g[1] == c.groups[k + 1][0]
                assert g[1] - g[0] == 16 or c.group_nodes((g[0], g[1] + 1)) > 128
