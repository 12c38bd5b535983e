"""PanMATs for the VCF tests: one-block star trees whose aligned rows are given, and the
random block PanMATs (rotation, inversion, strands) of the replay tests."""
from __future__ import annotations

from collections import Counter

import numpy as np

from _panmat import random_panmat
from _trees import names_for, random_tree
from panman_amd.panmat import CODE, PanMAT

NSNPS, NSNPD = 3, 5   # NucMutationType: one-base substitution / deletion


def star_panmat(rows: dict[str, str], consensus: str) -> PanMAT:
    """A root with one tip per row; one block holding `consensus` (bases), every tip's aligned
    row made from it by one-base substitutions and deletions ('-')."""
    names = list(rows) + ["root"]
    n = len(rows)
    off = np.zeros(n + 2, np.int32)
    off[n + 1] = n
    pm = PanMAT(names, off, np.arange(n, dtype=np.int32), n)
    pm.add_block(0, consensus)
    pm.add_block_mut(n, 0, True, False)
    for v, row in enumerate(rows.values()):
        assert len(row) == len(consensus)
        for i, (c, ch) in enumerate(zip(consensus, row)):
            if ch == "-":
                pm.add_nuc_mut(v, 0, i, -1, NSNPD, [0])
            elif ch != c:
                pm.add_nuc_mut(v, 0, i, -1, NSNPS, [CODE[ch]])
    return pm


def random_case(leaves: int, seed: int) -> PanMAT:
    rng = np.random.default_rng(seed)
    off, idx, root = random_tree(leaves, rng, max_children=4, unary=0.1)
    return random_panmat(rng, off, idx, root, names_for(off), blocks=6)


def modal_reference(rows: dict[str, str]) -> str:
    """The first tip in byte order of the names whose row has the most common length."""
    length = Counter(len(r) for r in rows.values()).most_common(1)[0][0]
    return min((n for n in rows if len(rows[n]) == length), key=lambda s: s.encode())


def edge_rows(columns: int, tips: int, seed: int, ref_name: str = "ref"):
    """(rows, consensus) of one block of `columns` columns: the reference-to-be ("ref") has gaps
    (POS != column), every tip events across columns 69|70 and 2047|2048 where the block has
    them, an event open at the last column, and a few scattered ones."""
    rng = np.random.default_rng(seed)
    cons = "".join(rng.choice(list("ACGT"), size=columns))
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}

    def edit(row, i, kind):
        if 0 <= i < columns:
            row[i] = "-" if kind == 0 else other[cons[i]] if kind == 1 else cons[i]

    ref = list(cons)
    for i in (1, 5, 68, 69, 130, 2040, 2047, columns - 1):
        if tips % 2 or i != columns - 1:
            edit(ref, i, 0)
    rows = {ref_name: "".join(ref)}
    for k in range(tips):
        row = list(cons)
        for edge in (70, 2048):
            lo = edge - 1 - k % 3
            for i in range(lo, edge + 1 + (k // 3) % 3):
                edit(row, i, (i + k) % 3 if k % 7 else 1)
        edit(row, columns - 1, k % 2)
        if k % 4 == 0:
            edit(row, columns - 2, 0)
        for i in rng.integers(0, columns, size=3):
            edit(row, int(i), int(rng.integers(0, 2)))
        rows[f"t{k:03d}"] = "".join(row)
    return rows, cons
