"""PanMATs for the GFA tests: the hand cases that pin tests/_gfa_ref.py to src/gfa.cpp:3-500 (in
the from_fixture dict format, the expected text worked out by hand from the reference's code),
and wrappers around the MAF cases with rotation, sequence inversion and circular offsets cleared
(convertToGFA reads getSequenceFromReference(rotate = false); the FASTA it is compared with
must not apply them either)."""
from __future__ import annotations

import numpy as np

import _maf_cases
from _maf_cases import hand_panmat   # noqa: F401  (the hand cases are built the same way)
from panman_amd.panmat import PanMAT

B39 = "ACGT" * 9 + "ACG"    # 39 bases: with the end sentinel a block of 40 columns
B100 = "ACGT" * 25          # 100 bases: 101 columns, four chunks


def _case(blocks, block_muts, nuc_muts, gaps=()):
    return {"newick": "(t0,t1)r;", "blocks": blocks, "gaps": list(gaps), "block_muts": block_muts, "nuc_muts": nuc_muts,
            "rotation": {}, "inverted": {}, "circular": {}}


def _text(*lines, header=True):
    return ("H\tVN:Z:1.1\n" if header else "") + "".join(line + "\n" for line in lines)


# Mutation lists: [block, position, gap slot or -1, type, codes]; type 3 substitutes one base,
# type 4 fills one gap slot; codes A 1, C 2, G 4, T 8.
HAND = {
    # Forward chunks of a 40-column block: columns 0..31 and 32..39 (7 bases and the sentinel).
    # t0 turns base 35 (T) into A.  t0 makes nodes 0 and 1, t1 reuses 0 and makes 2.  Node 0 has
    # no incoming edge, so the merge loop stops at its first test; nothing merges.
    "A_two_tips_one_chunk": (
        _case([[0, B39]], {"r": [[0, 1, 0]]}, {"t0": [[0, 35, -1, 3, [1]]]}),
        _text("S\t1\t" + "ACGT" * 8, "S\t2\tACGAACG", "S\t3\tACGTACG",
              "L\t1\t+\t2\t+\t0M", "L\t1\t+\t3\t+\t0M",
              "P\tt0\t1+,2+\t*", "P\tt1\t1+,3+\t*")),
    # The same block on the reverse strand: the walk starts at column 39, so the first chunk is
    # columns 8..39 (31 bases and the sentinel, start (-1, 8, -1)) and the short one columns 0..7
    # (start (-1, 0, -1)); the texts stay in canonical order.  t0 turns base 2 (G) into T.
    "B_reverse_strand_40_columns": (
        _case([[0, B39]], {"r": [[0, 1, 1]]}, {"t0": [[0, 2, -1, 3, [8]]]}),
        _text("S\t1\t" + "ACGT" * 7 + "ACG", "S\t2\tACTTACGT", "S\t3\tACGTACGT",
              "L\t1\t-\t2\t-\t0M", "L\t1\t-\t3\t-\t0M",
              "P\tt0\t1-,2-\t*", "P\tt1\t1-,3-\t*")),
    # 32 gap slots in front of "ACGT": the first chunk is the gap slots alone.  In t1 it strips to
    # nothing: no node, no step.  t0 fills slot 5 with T: the node ((0, 0, 0), "T").  Node 0 has no
    # incoming edge and node 1 no outgoing one: nothing merges.
    "C_chunk_strips_to_nothing": (
        _case([[0, "ACGT"]], {"r": [[0, 1, 0]]}, {"t0": [[0, 0, 5, 4, [8]]]}, gaps=[[0, [[0, 32]]]]),
        _text("S\t1\tT", "S\t2\tACGT", "L\t1\t+\t2\t+\t0M", "P\tt0\t1+,2+\t*", "P\tt1\t2+\t*")),
    # Four chunks a b c d; t0 changes base 0, so it starts at a' (node 0) and t1 at a (node 4); b,
    # c, d are nodes 1, 2, 3 for both.  At u = b every test passes with dest = c (both have two
    # edges in and two out, the same tips): b becomes b + c, c is erased, b takes c's edges.  The
    # next round stops because G[d] is empty (inserted by that test) while GT[d] has two entries.
    # c's steps leave the paths; the texts number 1..4 in (id, strand) order: a', bc, d, a.
    "D_chain_merges": (
        _case([[0, B100]], {"r": [[0, 1, 0]]}, {"t0": [[0, 0, -1, 3, [2]]]}),
        _text("S\t1\tCCGT" + "ACGT" * 7, "S\t2\t" + "ACGT" * 16, "S\t3\tACGT", "S\t4\t" + "ACGT" * 8,
              "L\t1\t+\t2\t+\t0M", "L\t2\t+\t3\t+\t0M", "L\t4\t+\t2\t+\t0M",
              "P\tt0\t1+,2+,3+\t*", "P\tt1\t4+,2+,3+\t*")),
    # No nucleotide mutation: whole blocks.  t0's inversion of block 1 is "not an insertion" and
    # clears it; block 3 is never inserted and still gets its S line; no H line.
    "E_whole_blocks_with_an_inversion": (
        _case([[0, "ACG"], [1, "TT"], [2, "GGGG"], [3, "CA"]],
              {"r": [[0, 1, 0], [1, 1, 0], [2, 1, 0]], "t0": [[1, 0, 1]]}, {}),
        _text("S\t0\tACG", "S\t1\tTT", "S\t2\tGGGG", "S\t3\tCA",
              "L\t0\t+\t1\t+\t0M", "L\t0\t+\t2\t+\t0M", "L\t1\t+\t2\t+\t0M",
              "P\tt0\t0+,2+\t*", "P\tt1\t0+,1+,2+\t*", header=False)),
}


def _plain(pm: PanMAT) -> PanMAT:
    pm.rotation[:] = 0
    pm.inverted[:] = 0
    pm.circular[:] = -1
    return pm


def random_case(leaves: int, seed: int, blocks: int = 6, block_len=(40, 80)) -> PanMAT:
    """_maf_cases.random_case (both strands, absent blocks, gap slots, every mutation type)
    without rotation, sequence inversion and circular offsets."""
    return _plain(_maf_cases.random_case(leaves, seed, blocks=blocks, block_len=block_len))


def star(tip_names, widths, seed=0, gaps=True, reverse=()) -> PanMAT:
    """_maf_cases.star -- a root with one tip per name, one block per entry of `widths` (its
    columns, the end sentinel included), a few edits per tip -- with the blocks of `reverse`
    ((tip, block) pairs) inverted on their tip.  A width of 1 is a block without a base: its only
    column is the sentinel."""
    ones = [b for b, w in enumerate(widths) if w == 1]
    pm = _maf_cases.star(tip_names, [2 if w == 1 else w for w in widths], seed=seed, gaps=gaps)
    if ones:   # (no edit of such a block survives: its one base is gone)
        pm.blocks = [(b, [] if b in ones else words) for b, words in pm.blocks]
        pm.nuc_muts = [[m for m in lst if m[0] not in ones] for lst in pm.nuc_muts]
    for tip, block in reverse:
        pm.add_block_mut(tip, block, False, True)
    if not any(pm.nuc_muts):   # a mutation of a no-op type still selects the chunk branch (gfa.cpp:7-11)
        pm.add_nuc_mut(0, 0, 0, -1, 6, [0])
    return _plain(pm)


def names(n):
    return [f"t{k:03d}" for k in range(n)]
