"""PanMATs for the MAF tests: the hand cases that pin tests/_maf_ref.py to src/maf.cpp:68-188
(in the from_fixture dict format), the random block PanMATs of the replay tests, and shaped
trees for the kernels' edges (block widths, many blocks, many tips, digit widths)."""
from __future__ import annotations

import copy

import numpy as np

from _panmat import from_fixture, random_panmat
from _trees import names_for, parse_newick, random_tree
from panman_amd.panmat import PanMAT

# The root of "(t0,t1)r;" is addressed as "r" here; the Newick helper names it itself.
CASE_A = {
    "newick": "(t0,t1)r;",
    "blocks": [[0, "ACG"], [1, "TT"]],
    "gaps": [[1, [[1, 2]]]],
    "block_muts": {"r": [[0, 1, 0], [1, 1, 0]], "t1": [[1, 0, 0]]},
    "nuc_muts": {"t0": [[0, 1, -1, 3, [8]], [1, 1, 0, 2, [1]]], "t1": [[0, 0, -1, 5, [0]]]},
    "rotation": {}, "inverted": {}, "circular": {},
}


def _variant(**changes):
    k = copy.deepcopy(CASE_A)
    for key, value in changes.items():
        k[key] = value
    return k


def _text(*paragraphs):
    return "##maf version=1\n" + "".join("a\n" + "".join(line + "\n" for line in p) + "\n" for p in paragraphs)


# Block 0's word is 0x12400000 and block 1's 0x88000000: a signed comparison would swap them.
HAND = {
    "A": (CASE_A, _text(["s\tt0\t0\t3\t+\t6\tATG-", "s\tt1\t0\t2\t+\t2\t-CG-"], ["s\tt0\t3\t3\t+\t6\tTA-T-"])),
    "B_circular": (_variant(circular={"t0": 4}),
                   _text(["s\tt0\t2\t3\t+\t6\tATG-", "s\tt1\t0\t2\t+\t2\t-CG-"], ["s\tt0\t5\t3\t+\t6\tTA-T-"])),
    "C_inverted": (_variant(inverted={"t0": 1}),
                   _text(["s\tt0\t3\t3\t+\t6\tATG-", "s\tt1\t0\t2\t+\t2\t-CG-"], ["s\tt0\t0\t3\t+\t6\tTA-T-"])),
    "D_reverse_strand": (_variant(block_muts={"r": [[0, 1, 0], [1, 1, 1]], "t1": [[1, 0, 0]]}),
                         _text(["s\tt0\t0\t3\t+\t6\tATG-", "s\tt1\t0\t2\t+\t2\t-CG-"], ["s\tt0\t3\t3\t-\t6\tTA-T-"])),
    "E_equal_blocks": (_variant(blocks=[[0, "ACG"], [1, "TT"], [2, "ACG"]],
                                block_muts={"r": [[0, 1, 0], [1, 1, 0], [2, 1, 0]], "t1": [[1, 0, 0]]}),
                       _text(["s\tt0\t0\t3\t+\t9\tATG-", "s\tt1\t0\t2\t+\t5\t-CG-",
                              "s\tt0\t6\t3\t+\t9\tACG-", "s\tt1\t2\t3\t+\t5\tACG-"], ["s\tt0\t3\t3\t+\t9\tTA-T-"])),
    "F_block_nobody_holds": (_variant(blocks=[[0, "ACG"], [1, "TT"], [2, "GGGG"]]),
                             _text(["s\tt0\t0\t3\t+\t6\tATG-", "s\tt1\t0\t2\t+\t2\t-CG-"], [],
                                   ["s\tt0\t3\t3\t+\t6\tTA-T-"])),
    "G_offset_above_src_size": (_variant(circular={"t1": 5}),
                                _text(["s\tt0\t0\t3\t+\t6\tATG-", "s\tt1\t-3\t2\t+\t2\t-CG-"],
                                      ["s\tt0\t3\t3\t+\t6\tTA-T-"])),
}


def hand_panmat(case: dict) -> PanMAT:
    names, _, _, root = parse_newick(case["newick"])
    k = dict(case)
    k["block_muts"] = {(names[root] if node == "r" else node): lst for node, lst in case["block_muts"].items()}
    return from_fixture(k)


def random_case(leaves: int, seed: int, blocks: int = 6, block_len=(40, 80)) -> PanMAT:
    """random_panmat: rotation, inversion, circular offsets, both strands, absent blocks."""
    rng = np.random.default_rng(seed)
    off, idx, root = random_tree(leaves, rng, max_children=4, unary=0.1)
    return random_panmat(rng, off, idx, root, names_for(off), blocks=blocks, block_len=block_len)


def star(tip_names, widths, seed=0, gaps=True) -> PanMAT:
    """A root with one tip per name and one block per entry of `widths` (the block's columns:
    bases + gap slots + the end sentinel), every block inserted at the root; each tip deletes a
    few bases and fills a gap slot, so sizes differ from tip to tip."""
    rng = np.random.default_rng(seed)
    n = len(tip_names)
    off = np.zeros(n + 2, np.int32)
    off[n + 1] = n
    pm = PanMAT(list(tip_names) + ["root"], off, np.arange(n, dtype=np.int32), n)
    lens, slot = [], []
    for b, w in enumerate(widths):
        assert w >= 2
        g = 2 if gaps and w >= 6 else 0   # two gap slots before position 1
        L = w - 1 - g
        lens.append(L)
        slot.append(g)
        pm.add_block(b, "".join(rng.choice(list("ACGT"), size=L)))
        if g:
            pm.add_gaps(b, [(1, g)])
        pm.add_block_mut(n, b, True, False)
    for v in range(n):
        for b, L in enumerate(lens):
            if (v + b) % 3 == 0:
                pm.add_nuc_mut(v, b, int(rng.integers(0, L)), -1, 5, [0])          # one base deleted
            if slot[b] and (v + b) % 4 == 1:
                pm.add_nuc_mut(v, b, 1, int(rng.integers(0, slot[b])), 4, [8])     # a gap slot filled
            if L > 8 and (v + b) % 5 == 2:
                pm.add_nuc_mut(v, b, L - 3, -1, 1, [0, 0, 0])                      # the last three deleted
    return pm
