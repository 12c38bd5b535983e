"""PanMATs for the imputation tests (tests/_impute_ref.py, pm_impute): hand-built cases on one seven-node tree
whose answers tests/test_impute_ref.py works out in its comments, and a generator that plants the same insertion
run in relatives of a random PanMAT -- random_panmat alone never puts one run in two nodes."""
from __future__ import annotations

import numpy as np

from _panmat import random_panmat
from panman_amd.panmat import PanMAT

NS, ND, NI, NSNPS, NSNPI, NSNPD = 0, 1, 2, 3, 4, 5
A, C, G, T, N = 1, 2, 4, 8, 15


def base(lengths=None) -> PanMAT:
    """((a,b)p,(c,d)q)r in pre-order r p a b q c d.  Block 0 is ACGTACGTAC with 4 gap slots at positions 3 and
    7, block 1 is GGGGCCCC with 8 slots at position 2; the root inserts both forward."""
    pm = PanMAT(["r", "p", "a", "b", "q", "c", "d"], np.array([0, 2, 4, 4, 4, 6, 6, 6], np.int32),
                np.array([1, 4, 2, 3, 5, 6], np.int32), 0)
    pm.add_block(0, "ACGTACGTAC")
    pm.add_gaps(0, [(3, 4), (7, 4)])
    pm.add_block(1, "GGGGCCCC")
    pm.add_gaps(1, [(2, 8)])
    pm.add_block_mut(pm.index("r"), 0, True, False)
    pm.add_block_mut(pm.index("r"), 1, True, False)
    if lengths is not None:
        pm.branch_length = np.array([0.0 if n == "r" else lengths for n in pm.names], np.float32)
    return pm


def mut(pm, node, blk, pos, gap, typ, codes):
    pm.add_nuc_mut(pm.index(node), blk, pos, gap, typ, codes)


def ns_all_n():
    pm = base()
    mut(pm, "a", 0, 1, -1, NS, [N, N])
    return pm


def ns_partial_main():
    pm = base()
    mut(pm, "a", 0, 0, -1, NSNPS, [G])
    mut(pm, "a", 0, 4, -1, NS, [A, N, C, N])
    mut(pm, "a", 0, 9, -1, NSNPS, [G])
    return pm


def ns_partial_gap():
    pm = base()
    mut(pm, "a", 0, 3, 0, NS, [A, N, C, N])
    return pm


def nsnps_n():
    pm = base()
    mut(pm, "a", 0, 2, -1, NSNPS, [N])
    return pm


def n_in_insertion():
    pm = base()
    mut(pm, "a", 0, 3, 0, NI, [A, N])
    return pm


def root_n():
    pm = base()
    mut(pm, "r", 0, 0, -1, NS, [N])
    mut(pm, "r", 0, 3, 0, NI, [N])
    return pm


def merge_last_run_only():
    """a: I(3g0 A N), S(0 C), I(3g2 G) is one run of 3 with one N -- the substitution between does not end it;
    b holds the run as one record."""
    pm = base()
    mut(pm, "a", 0, 3, 0, NI, [A, N])
    mut(pm, "a", 0, 0, -1, NSNPS, [C])
    mut(pm, "a", 0, 3, 2, NI, [G])
    mut(pm, "b", 0, 3, 0, NI, [A, C, G])
    return pm


def merge_only_last_is_target():
    """a: I(5 main N), I(3g2 A), I(6 main C): the third continues the first run, but only the last run is a merge
    target, and that one (headed in a slot) compares gap positions: -1 - 2 != 1.  Three runs stay, so b's
    I(5 main A) is the first one's IndelPosition."""
    pm = base()
    mut(pm, "a", 0, 5, -1, NI, [N])
    mut(pm, "a", 0, 3, 2, NI, [A])
    mut(pm, "a", 0, 6, -1, NI, [C])
    mut(pm, "b", 0, 5, -1, NI, [A])
    return pm


def merge_main_head_ignores_gap():
    """a: I(5 main N A) then I(7g3 C): the head is at gap -1 and 7 - 5 == 2, so the slot record merges: one run
    (5, -1) of 3.  b holds I(5 main A C G)."""
    pm = base()
    mut(pm, "a", 0, 5, -1, NI, [N, A])
    mut(pm, "a", 0, 7, 3, NI, [C])
    mut(pm, "b", 0, 5, -1, NI, [A, C, G])
    return pm


def merge_gap_head_ignores_position():
    """a: I(3g0 N A) then I(7g2 C): the head is in a slot and 2 - 0 == 2, so the record at another position
    merges: one run (3, 0) of 3.  b holds I(3g0 A C G)."""
    pm = base()
    mut(pm, "a", 0, 3, 0, NI, [N, A])
    mut(pm, "a", 0, 7, 2, NI, [C])
    mut(pm, "b", 0, 3, 0, NI, [A, C, G])
    return pm


def sibling_donor(lengths=None):
    pm = base(lengths)
    mut(pm, "a", 0, 3, 0, NI, [N, N, N])
    mut(pm, "a", 0, 0, -1, NSNPS, [C])
    mut(pm, "b", 0, 3, 0, NI, [A, C, G])
    mut(pm, "b", 0, 9, -1, NSNPS, [G])
    return pm


def grandparent_donor(lengths=None):
    pm = base(lengths)
    mut(pm, "a", 0, 3, 0, NI, [N, N, N])
    mut(pm, "c", 0, 3, 0, NI, [A, C, G])
    mut(pm, "p", 0, 1, -1, NSNPS, [T])
    return pm


def tie_first_wins():
    pm = base()
    mut(pm, "a", 0, 3, 0, NI, [N, N, N])
    mut(pm, "b", 0, 3, 0, NI, [A, C, G])
    mut(pm, "c", 0, 3, 0, NI, [A, C, G])
    return pm


def block_ratchet():
    """b gives (2, 0); c would give nuc 3 but its path carries c's inversion of block 1: block improvement -1."""
    pm = base()
    mut(pm, "a", 0, 3, 0, NI, [N, N, N])
    mut(pm, "b", 0, 3, 0, NI, [A, C, G])
    mut(pm, "b", 0, 9, -1, NSNPS, [G])
    mut(pm, "c", 0, 3, 0, NI, [A, C, G])
    pm.add_block_mut(pm.index("c"), 1, False, True)
    return pm


def block_swap():
    """The path climbs out of c, which deletes block 1, and a deletes it too: deletion inverted to an insertion,
    then a's deletion cancels it."""
    pm = base()
    mut(pm, "a", 0, 3, 0, NI, [N, N, N])
    mut(pm, "c", 0, 3, 0, NI, [A, C, G])
    pm.add_block_mut(pm.index("c"), 1, False, False)
    pm.add_block_mut(pm.index("a"), 1, False, False)
    return pm


HAND = {f.__name__: f for f in (ns_all_n, ns_partial_main, ns_partial_gap, nsnps_n, n_in_insertion, root_n, merge_last_run_only,
                                merge_only_last_is_target, merge_main_head_ignores_gap, merge_gap_head_ignores_position,
                                sibling_donor, grandparent_donor, tie_first_wins, block_ratchet, block_swap)}


def cells_of(m):
    n = m[4] >> 4
    return [(m[0], m[2] + i, -1) if m[3] == -1 else (m[0], m[2], m[3] + i) for i in range(n)]


def drop_double_writes(pm: PanMAT):
    """Every record that writes a cell an earlier record of its list wrote is dropped (pm_impute refuses them)."""
    for v in range(pm.num_nodes):
        seen, keep = set(), []
        for m in pm.nuc_muts[v]:
            cs = cells_of(m)
            if any(c in seen for c in cs):
                continue
            seen.update(cs)
            keep.append(m)
        pm.nuc_muts[v] = keep


def planted(rng, names, off, idx, root, winners=4, losers=2) -> PanMAT:
    """A random PanMAT (no block mutation below the root) with branch lengths in eighths, plus one more block,
    ACGTACGTACGT with 6 slots at positions 2 and 5, that the random lists never touch.  Sibling pairs (x, y) get
    the same insertion run in it, all N in x: `winners` pairs where y's list holds nothing else and y's branch
    is 0.5 long, so the move pays at every distance; `losers` pairs where y keeps its random list."""
    pm = random_panmat(rng, off, idx, root, names, block_rate=0, options=False)
    drop_double_writes(pm)
    blk = 1 + max(b for b, _ in pm.blocks)
    pm.add_block(blk, "ACGTACGTACGT")
    pm.add_gaps(blk, [(2, 6), (5, 6)])
    pm.add_block_mut(root, blk, True, False)
    pm.branch_length = (rng.integers(0, 17, size=pm.num_nodes) / 8).astype(np.float32)
    pm.branch_length[root] = 0
    pairs = []
    for v in range(pm.num_nodes):
        ks = [int(c) for c in idx[off[v]:off[v + 1]]]
        if len(ks) >= 2 and v != root:
            pairs.append((ks[0], ks[1]))
    order = rng.permutation(len(pairs))
    assert len(pairs) >= winners + losers
    for k, j in enumerate(order[:winners + losers]):
        x, y = pairs[int(j)]
        ln = int(rng.integers(2, 7))
        pos, gap = (2, int(rng.integers(0, 7 - ln))) if k % 2 == 0 else (5, int(rng.integers(0, 7 - ln)))
        pm.add_nuc_mut(x, blk, pos, gap, NI, [N] * ln)
        if k < winners:
            pm.nuc_muts[y] = []
            pm.branch_length[y] = 0.5
        pm.add_nuc_mut(y, blk, pos, gap, NI, [int(rng.choice([A, C, G, T])) for _ in range(ln)])
    return pm
