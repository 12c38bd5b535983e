"""PanMATs for the amino-acid translation tests (tests/test_aa_ref.py on the CPU,
tests/test_gpu_aa.py and tests/test_cli_aa.py on the GPU): hand cases with their expected
results, the random cases and single-block stars for the kernels' edges.

The builders below `star` plant shapes at the constants of the kernels in pm_aa.hip (a ballot
round of 64 cells or 64 blocks in k_aa_locate, kAaChunk = 256 cells a round in k_aa_codons, four
waves a workgroup, the digits of an index); each has a check_* that proves from `locate`, `window`
and `codons` of tests/_aa_ref.py alone that the shapes are there.  tests/test_aa_cases.py runs
every check without a GPU, over the parameter lists at the end of this file."""
from __future__ import annotations

import re
from itertools import islice

import numpy as np

import _aa_ref
from _maf_ref import _parents, _path
from _panmat import random_panmat
from _trees import names_for, random_tree
from panman_amd.panmat import PanMAT

A, C, G, T, N = 1, 2, 4, 8, 15
NS, ND, NI, SNP, SNP_INS, SNP_DEL = 0, 1, 2, 3, 4, 5   # nucleotide mutation types


def tree(spec: dict, root: str) -> PanMAT:
    """spec: {parent name: [child names]}; nodes are numbered in order of first mention, root first."""
    names = [root]
    for parent, kids in spec.items():
        for n in [parent] + kids:
            if n not in names:
                names.append(n)
    off, idx = [0], []
    for n in names:
        idx += [names.index(k) for k in spec.get(n, [])]
        off.append(len(idx))
    return PanMAT(names, np.array(off, np.int32), np.array(idx, np.int32), 0)


def _snp(pm, node, block, pos, code, gap=-1):
    pm.add_nuc_mut(pm.index(node), block, pos, gap, SNP, [code])


def issue_case():
    """One block, no gaps; a SNP, a single-base deletion, a run deletion, an N, an unchanged child."""
    pm = tree({"r": ["a", "b", "c", "u"], "u": ["d"]}, "r")
    pm.add_block(0, "ATGGCCTAAGGGG")
    pm.add_block_mut(0, 0, True, False)
    _snp(pm, "a", 0, 4, A)
    pm.add_nuc_mut(pm.index("b"), 0, 3, -1, SNP_DEL, [0])
    pm.add_nuc_mut(pm.index("c"), 0, 3, -1, ND, [0, 0, 0])
    _snp(pm, "u", 0, 0, N)
    want = {"a": "S:1:Asp;", "b": "S:1:Pro;S:2:Lys;", "c": "I:3:Gly;D:1;", "u": "S:0:Trp;S:1:Pro;D:2;",
            "d": "S:0:Trp;S:1:Pro;D:2;"}
    return pm, 0, 9, want, 3


def slot_start_case():
    """start on gap slot 1 of position 2; position 5 has slots 0 and 1 filled: its slot 0 is left out."""
    pm = tree({"r": ["x", "y"]}, "r")
    pm.add_block(0, "ACGTACGTAC")
    pm.add_gaps(0, [(2, 2), (5, 2)])
    pm.add_block_mut(0, 0, True, False)
    pm.add_nuc_mut(0, 0, 2, 0, NI, [T, T])
    pm.add_nuc_mut(0, 0, 5, 0, NI, [G, G])
    _snp(pm, "x", 0, 3, A)            # TGT AGC -> TGA AGC
    _snp(pm, "y", 0, 5, A, gap=0)     # the slot the walk leaves out: no change
    return pm, 3, 12, {"x": "S:0:*;"}, 2


def slot_end_case():
    """start a main position; node e's end falls on a filled gap slot: its window is ERROR."""
    pm = tree({"r": ["e", "f"]}, "r")
    pm.add_block(0, "ATGGCCTAAGGG")
    pm.add_gaps(0, [(8, 1)])
    pm.add_block_mut(0, 0, True, False)
    pm.add_nuc_mut(pm.index("e"), 0, 8, 0, SNP_INS, [C])
    _snp(pm, "f", 0, 1, C)            # ATG -> ACG
    return pm, 0, 8, {"e": "D:0;D:1;", "f": "S:0:Thr;"}, 2


def reverse_case():
    """Block 0 on the reverse strand starts the window; node g also reverses block 1, whose walk
    then starts at block 0's last index: the sentinel, printed as a dash inside a codon."""
    pm = tree({"r": ["f", "g", "h"]}, "r")
    pm.add_block(0, "GGGCCC")
    pm.add_block(1, "ATGAAA")
    pm.add_block_mut(0, 0, True, True)
    pm.add_block_mut(0, 1, True, False)
    _snp(pm, "f", 0, 3, A)            # CCG -> CAG
    pm.add_block_mut(pm.index("g"), 1, False, True)
    _snp(pm, "h", 0, 2, T)            # CCG GGA -> CCT GGA: the same amino acids, no line
    return pm, 1, 10, {"f": "S:0:Gln;", "g": "S:2:Lys;"}, 3


def absent_case():
    """Node h lost block 1: seven dashes inside its window, and its own end lies further right."""
    pm = tree({"r": ["h", "i"]}, "r")
    pm.add_block(0, "ATGAAA")
    pm.add_block(1, "CCCGGG")
    pm.add_block(2, "TTTACGTCA")
    for b in range(3):
        pm.add_block_mut(0, b, True, False)
    pm.add_block_mut(pm.index("h"), 1, False, False)
    return pm, 0, 14, {"h": "I:4:Phe;I:4:Thr;D:2;D:3;"}, 4


def short_block0_case():
    """Block 1 on the reverse strand is longer than block 0: its walk starts at block 0's last
    index, inside it (defined, and not at its end)."""
    pm = tree({"r": ["k"]}, "r")
    pm.add_block(0, "ACG")
    pm.add_block(1, "TTTGGGCCC")
    pm.add_block_mut(0, 0, True, False)
    pm.add_block_mut(0, 1, True, True)
    _snp(pm, "k", 0, 0, G)
    return pm, 0, 10, {"k": "S:0:Ala;"}, 1


def unsupported_case():
    """Block 1 on the reverse strand is shorter than block 0: the reference indexes out of range."""
    pm = tree({"r": ["k"]}, "r")
    pm.add_block(0, "ACGTACGT")
    pm.add_block(1, "ACG")
    pm.add_block_mut(0, 0, True, False)
    pm.add_block_mut(0, 1, True, True)
    return pm, 0, 9


HAND = {"issue": issue_case, "slot_start": slot_start_case, "slot_end": slot_end_case, "reverse": reverse_case,
        "absent": absent_case, "short_block0": short_block0_case}


def text_of(pm, want: dict) -> str:
    """The text of `want` ({name: string}) in node-id order."""
    return "node_id\taa_mutations\n" + "".join(f"{n}\t{want[n]}\n" for n in pm.names if n in want)


def lengths(pm):
    """L of every node: the characters of its held blocks that are neither '-' nor 'x'."""
    parent = _parents(pm)
    max_id = max(b for b, _ in pm.blocks)
    is_block = {b for b, _ in pm.blocks}
    out = []
    for v in range(pm.num_nodes):
        s = _aa_ref.NodeState(pm, _path(pm, parent, v), max_id, is_block)
        out.append(sum((m not in "-x") + sum(ch not in "-x" for ch in sl)
                       for b, seq in enumerate(s.seq) if s.held[b] for m, sl in seq))
    return out


def random_case(leaves: int, k: int, seed: int, blocks: int = 6):
    """random_panmat with `blocks` blocks of k bases each (equal lengths keep every reverse-strand walk
    defined) and start < end below the smallest L of its nodes."""
    rng = np.random.default_rng(seed)
    off, idx, root = random_tree(leaves, rng, unary=0.1)
    pm = random_panmat(rng, off, idx, root, names_for(off), blocks=blocks, block_len=(k, k + 1))
    low = min(lengths(pm))
    assert low >= 2, (leaves, k, seed)
    start = int(rng.integers(0, low - 1))
    end = int(rng.integers(start + 1, low))
    return pm, start, end


RANDOM = [(1, 9, 1), (2, 9, 2), (30, 5, 3), (30, 17, 4), (30, 40, 5), (30, 40, 6), (2, 40, 7), (30, 64, 8)]


def star(names, length: int, seed: int, edits=()):
    """One block of `length` random bases under a root with the leaves `names`; every leaf gets
    a few SNPs, and `edits` adds (leaf name, position, type, codes) on top."""
    rng = np.random.default_rng(seed)
    pm = tree({"root": list(names)}, "root")
    pm.add_block(0, "".join(rng.choice(list("ACGT"), size=length)))
    pm.add_block_mut(0, 0, True, False)
    for n in names:
        for pos in sorted(set(rng.integers(0, length, size=max(2, length // 40)).tolist())):
            _snp(pm, n, 0, int(pos), int(rng.choice([A, C, G, T])))
    for name, pos, typ, codes in edits:
        pm.add_nuc_mut(pm.index(name), 0, pos, -1, typ, list(codes))
    return pm


# ---- shapes at the kernels' constants (pm_aa.hip) ------------------------------------------------

WAVE = 64        # cells of one ballot round of k_aa_locate's rank-select, blocks of one round of its block scan
ROUND = 256      # kAaChunk (pm_internal.h): cells of one round of k_aa_codons
WIDE_LEN = 300   # bases of every block of wide_case
_OTHER = {"A": C, "C": G, "G": T, "T": A}   # the code of a base that differs


def states(pm):
    """Every node's NodeState, in node-id order."""
    parent = _parents(pm)
    max_id = max(b for b, _ in pm.blocks)
    is_block = {b for b, _ in pm.blocks}
    return [_aa_ref.NodeState(pm, _path(pm, parent, v), max_id, is_block) for v in range(pm.num_nodes)]


def _real(ch) -> bool:
    return ch != "-" and ch != "x"


def _size(s, b) -> int:
    return sum(_real(m) + sum(_real(ch) for ch in sl) for m, sl in s.seq[b]) if s.held[b] else 0


def length_of(s) -> int:
    return sum(_size(s, b) for b in range(len(s.seq)))


def rank_in_block(s, g: int):
    """(block, the characters of that block the walk order of `locate` passes before coordinate g)."""
    total = length_of(s)
    if not g < total:
        g -= total
    b = _aa_ref.locate(s, g)[0]
    return b, g - sum(_size(s, i) for i in range(b))


def _column(seq, j, k) -> int:
    """The cell of (position j, slot k) in the forward order: per position its slots, then its main character."""
    return sum(len(sl) + 1 for _, sl in seq[:j]) + (k if k >= 0 else len(seq[j][1]))


def _reverse_cells(seq, top):
    """(position, slot) of a block's cells in the reverse walk's order from position `top` down."""
    for j in range(top, -1, -1):
        yield j, -1
        for k in range(len(seq[j][1]) - 1, -1, -1):
            yield j, k


def _first_cell(s, k0, i):
    """The first coordinate the window walk visits in block i when i is not its first block."""
    if s.forward[i]:
        return (i, 0, k0) if 0 <= k0 < len(s.seq[i][0][1]) else (i, 0, -1)
    return (i, len(s.seq[0]) - 1, -1)


def _index(s, start, cell):
    """The window index of a cell: what the walk from `start` emits before it (None: never reached)."""
    w = _aa_ref.window(s, start, cell)
    return None if w is None else len(w)


def wide_case(strands, ids, slots: bool):
    """Three blocks of WIDE_LEN bases (equal lengths keep every reverse walk defined) with the ids
    `ids`, inserted at the root with the strands `strands` ('+' / '-').  With `slots` every block has
    two gap slots at every fifth position, the root fills both at every tenth, and leaf "fill" one
    more (beyond the first block's cell 256).  Leaves: "same" (no mutation, no line), "lost" (loses
    the middle block), "flip_middle" and "flip_last_block" (invert a block's strand), "shift" (a one-base
    deletion early in the first block's walk: a frame shift), "snp"; and the internal node "inner"
    with two leaves, whose row comes from the derived tip of the replay."""
    assert len(strands) == len(ids) == 3
    rng = np.random.default_rng(300 + sum(1 << n for n, st in enumerate(strands) if st == "-"))
    kids = ["lost", "same", "flip_middle", "flip_last_block", "shift", "snp", "inner"] + (["fill"] if slots else [])
    pm = tree({"root": kids, "inner": ["in_a", "in_bb"]}, "root")
    seqs = []
    for b, strand in zip(ids, strands):
        seqs.append("".join(rng.choice(list("ACGT"), size=WIDE_LEN)))
        pm.add_block(b, seqs[-1])
        if slots:
            pm.add_gaps(b, [(p, 2) for p in range(0, WIDE_LEN, 5)])
        pm.add_block_mut(0, b, True, strand == "-")
        if slots:
            for p in range(0, WIDE_LEN, 10):
                pm.add_nuc_mut(0, b, p, 0, NI, [int(c) for c in rng.choice([A, C, G, T], size=2)])

    def snp(node, n, pos):
        _snp(pm, node, ids[n], pos, _OTHER[seqs[n][pos]])

    pm.add_block_mut(pm.index("lost"), ids[1], False, False)
    pm.add_block_mut(pm.index("flip_middle"), ids[1], False, True)
    pm.add_block_mut(pm.index("flip_last_block"), ids[2], False, True)
    pm.add_nuc_mut(pm.index("shift"), ids[0], 4 if strands[0] == "+" else WIDE_LEN - 4, -1, SNP_DEL, [0])
    snp("snp", 1, 150)
    snp("inner", 0, 100)
    snp("in_a", 2, 20)
    snp("in_bb", 1, 200)
    if slots:
        pm.add_nuc_mut(pm.index("fill"), ids[0], 255, 0, SNP_INS, [G])
    return pm


def wide_tags(pm, sts, start: int, end: int) -> set:
    """What one window of a wide_case reaches, from `locate`, `window` and `codons` alone:
      a_start64 / a_start256 / a_end64 / a_end256  the root's coordinate lies in a reverse block, 64 to 255 /
                  at least 256 of the block's characters into its walk (the second / a later than the fourth
                  ballot round of k_aa_locate's rank-select at the least)
      b_first / b_later  the root's walk takes more than ROUND cells of a reverse block as its first block
                  (from j0 down) / as a later one (from block 0's last index)
      c_fwd_* / c_rev_*  the root's start is slot 0, slot 1 or a main character of a forward / reverse block
      c_leftout_main / c_leftout_slot1  some node's start is a main character / a slot 1, and its walk of a
                  forward block leaves out a filled slot ROUND cells and more behind the block's first
                  walked cell, before the end
      d_rev256    some node has a codon with bases on both sides of cell ROUND of a reverse block's walk
      d_absent    "lost" has a codon that starts before its absent middle block and ends behind it
      e_holes     the root's window spans an id that holds no block
      f_wrap      both coordinates wrap on "lost" and neither does on the root."""
    tags = set()
    root = sts[pm.root]
    s0, e0 = _aa_ref.locate(root, start), _aa_ref.locate(root, end)
    for which, g, at in (("start", start, s0), ("end", end, e0)):
        if not root.forward[at[0]]:
            r = rank_in_block(root, g)[1]
            if r >= WAVE:
                tags.add(f"a_{which}{ROUND if r >= ROUND else WAVE}")
    tags.add(f"c_{'fwd' if root.forward[s0[0]] else 'rev'}_{'main' if s0[2] == -1 else 'slot%d' % s0[2]}")
    if any(not root.seq[i] for i in range(s0[0], e0[0] + 1)):
        tags.add("e_holes")
    lost = pm.index("lost")
    low = length_of(sts[lost])
    if low <= start < end < length_of(root):
        assert _aa_ref.locate(sts[lost], start) == _aa_ref.locate(sts[lost], start - low)
        assert _aa_ref.locate(sts[lost], end) == _aa_ref.locate(sts[lost], end - low)
        tags.add("f_wrap")
    for v, s in enumerate(sts):
        sv, ev = _aa_ref.locate(s, start), _aa_ref.locate(s, end)
        if sv is None or ev is None:
            continue
        w = _aa_ref.window(s, sv, ev)
        if w is None:
            continue
        _, cs, ce = _aa_ref.codons(w)
        k0 = sv[2]
        blocks = [i for i in range(sv[0], ev[0] + 1) if s.seq[i]]
        begin = [0 if i == sv[0] else _index(s, sv, _first_cell(s, k0, i)) for i in blocks] + [len(w)]
        for n, i in enumerate(blocks):
            seq = s.seq[i]
            if not s.forward[i]:
                if v == pm.root and begin[n + 1] - begin[n] > ROUND:
                    tags.add("b_first" if i == sv[0] else "b_later")
                cell = next(islice(_reverse_cells(seq, sv[1] if i == sv[0] else len(s.seq[0]) - 1), ROUND, None), None)
                at = None if cell is None else _index(s, sv, (i,) + cell)
                if at is not None and at < len(w) and any(a < at <= b for a, b in zip(cs, ce)):
                    tags.add("d_rev256")
            elif k0 in (-1, 1):
                first = _column(seq, sv[1], k0) if i == sv[0] else 0
                last = _column(seq, ev[1], ev[2]) if i == ev[0] else _column(seq, len(seq) - 1, -1) + 1
                out = [j for j, (_, sl) in enumerate(seq) for k, ch in enumerate(sl)
                       if s.held[i] and _real(ch) and (k0 == -1 or k < k0) and first + ROUND <= _column(seq, j, k) < last]
                if out:   # proven by the window: position j's main character follows the one before it too closely
                    j = out[0]
                    assert _index(s, sv, (i, j, -1)) - _index(s, sv, (i, j - 1, -1)) < 1 + len(seq[j][1])
                    tags.add("c_leftout_main" if k0 == -1 else "c_leftout_slot1")
            if v == lost and not s.held[i] and 0 < n < len(blocks) - 1:
                lo, hi = begin[n], begin[n + 1]
                if hi - lo >= WIDE_LEN and any(a < lo and b >= hi for a, b in zip(cs, ce)):
                    tags.add("d_absent")
    return tags


def wide_required(strands, ids, slots: bool) -> set:
    """The tags the windows of one wide_case must reach between them."""
    need = {"a_start64", "a_start256", "a_end64", "a_end256", "b_first", "b_later", "d_rev256", "d_absent", "f_wrap"}
    if slots:
        need |= {"c_rev_slot0", "c_rev_slot1", "c_rev_main", "c_leftout_main", "c_leftout_slot1"}
        if "+" in strands:
            need |= {"c_fwd_slot0", "c_fwd_slot1", "c_fwd_main"}
    if list(ids) != sorted(range(len(ids))):
        need.add("e_holes")
    return need


def check_wide_case(pm, strands, ids, slots: bool, windows):
    """The blocks, strands, lengths and leaves of wide_case, and the windows' tags; returns
    {window: tags}."""
    sts = states(pm)
    root = sts[pm.root]
    assert [b for b, _ in pm.blocks] == list(ids) and all(len(root.seq[b]) == WIDE_LEN + 1 for b in ids)
    assert [root.held[b] and root.forward[b] for b in ids] == [st == "+" for st in strands]
    assert all(root.held[b] for b in ids)
    per_block = WIDE_LEN + (2 * (WIDE_LEN // 10) if slots else 0)
    assert length_of(root) == 3 * per_block and min(length_of(s) for s in sts) == 2 * per_block
    assert length_of(sts[pm.index("lost")]) == 2 * per_block and not sts[pm.index("lost")].held[ids[1]]
    assert sts[pm.index("flip_middle")].forward[ids[1]] != root.forward[ids[1]]
    assert sts[pm.index("flip_last_block")].forward[ids[2]] != root.forward[ids[2]]
    assert length_of(sts[pm.index("shift")]) == 3 * per_block - 1
    assert length_of(sts[pm.index("fill")]) == 3 * per_block + 1 if slots else "fill" not in pm.names
    assert pm.child_offsets[pm.index("inner") + 1] - pm.child_offsets[pm.index("inner")] == 2
    if slots:
        cells = [len(sl) for _, sl in root.seq[ids[0]]]
        assert sum(cells) == 2 * (WIDE_LEN // 5) and sum(_real(ch) for _, sl in root.seq[ids[0]] for ch in sl) == 2 * (WIDE_LEN // 10)
    tags = {(start, end): wide_tags(pm, sts, start, end) for start, end in windows}
    reached = set().union(*tags.values())
    assert wide_required(strands, ids, slots) <= reached, sorted(wide_required(strands, ids, slots) - reached)
    return tags


def check_wide_errors(pm, strands, slots: bool, windows):
    """Every window is the root's "ERROR" (both coordinates located), and one of them because the
    end wraps in front of the start.  With slots and a forward block, one starts on a main
    character and ends on a filled slot of a forward block, ROUND cells and more behind the
    block's first walked cell -- a slot the walk leaves out."""
    root = states(pm)[pm.root]
    beyond = wraps = False
    for start, end in windows:
        s0, e0 = _aa_ref.locate(root, start), _aa_ref.locate(root, end)
        assert s0 is not None and e0 is not None and _aa_ref.window(root, s0, e0) is None, (start, end)
        wraps = wraps or start < length_of(root) <= end
        seq = root.seq[e0[0]]
        if s0[2] == -1 and e0[2] >= 0 and root.forward[e0[0]] and s0[0] <= e0[0]:
            assert _real(seq[e0[1]][1][e0[2]])
            first = _column(seq, s0[1], -1) if s0[0] == e0[0] else 0
            beyond = beyond or _column(seq, e0[1], e0[2]) - first >= ROUND
    assert wraps and (beyond or not (slots and "+" in strands))


def many_blocks_case():
    """129 blocks of 7 bases, every third on the reverse strand; "snps" with a SNP in blocks 62 to 65,
    127 and 128, "lost" without block 64, "shift" with a one-base deletion in block 0."""
    rng = np.random.default_rng(129)
    pm = tree({"root": ["snps", "lost", "shift"]}, "root")
    seqs = []
    for b in range(129):
        seqs.append("".join(rng.choice(list("ACGT"), size=7)))
        pm.add_block(b, seqs[-1])
        pm.add_block_mut(0, b, True, b % 3 == 2)
    for b in (62, 63, 64, 65, 127, 128):
        _snp(pm, "snps", b, b % 7, _OTHER[seqs[b][b % 7]])
    pm.add_block_mut(pm.index("lost"), 64, False, False)
    pm.add_nuc_mut(pm.index("shift"), 0, 2, -1, SNP_DEL, [0])
    return pm


def check_many_blocks_case(pm, windows):
    """Blocks 63 | 64 and 127 | 128 are the last lane of one round of k_aa_locate's block scan and
    the first of the next: a start and an end in each of 63, 64, 65, 127 and 128, located there by
    the reference, and a window over all blocks."""
    sts = states(pm)
    root = sts[pm.root]
    assert len(pm.blocks) == 129 and all(len(root.seq[b]) == 8 for b in range(129))
    assert [root.forward[b] for b in range(129)] == [b % 3 != 2 for b in range(129)] and all(root.held)
    assert not sts[pm.index("lost")].held[64] and length_of(sts[pm.index("shift")]) == 129 * 7 - 1
    first = {_aa_ref.locate(root, s)[0] for s, _ in windows}
    last = {_aa_ref.locate(root, e)[0] for _, e in windows}
    assert {63, 64, 65, 127, 128} <= first and {63, 64, 65, 127, 128} <= last
    assert any(_aa_ref.locate(root, s)[0] == 0 and _aa_ref.locate(root, e)[0] == 128 for s, e in windows)


def five_digit_case():
    """One block of 30,100 bases; "a" deletes base 9 (a frame shift: nearly every codon an S entry),
    "b" six bases near 29,000 (its last two codons start behind the root's last: I entries at 10,020)."""
    edits = [("a", 9, SNP_DEL, [0]), ("b", 29000, ND, [0] * 6)]
    return star(["a", "b", "c"], 30100, seed=5, edits=edits), 0, 30060


def check_five_digit_case(want):
    text, ref_codons, unlocated = want
    assert ref_codons == 10020 and unlocated == 0
    assert re.search(r"[\t;]S:1\d{4}:", text) and re.search(r";[ID]:1\d{4}[:;]", text)
    lines = text.split("\n")
    assert max(len(line) for line in lines) > 65536 and lines[1].startswith("a\t")


def many_nodes_case():
    """A star of 257 leaves (258 nodes: a last workgroup of k_aa_locate with two of its four waves) over
    one block of 40 bases; every leaf a SNP, every seventh a one-base deletion."""
    rng = np.random.default_rng(257)
    names = [f"n{k}" + "x" * (k % 5) for k in range(257)]
    pm = tree({"root": names}, "root")
    seq = "".join(rng.choice(list("ACGT"), size=40))
    pm.add_block(0, seq)
    pm.add_block_mut(0, 0, True, False)
    for k, n in enumerate(names):
        pos = (5 * k + 2) % 40
        _snp(pm, n, 0, pos, _OTHER[seq[pos]])
        if k % 7 == 0:
            pm.add_nuc_mut(pm.index(n), 0, (pos + 3 + k // 7) % 36, -1, SNP_DEL, [0])
    return pm, 1, 37


def check_many_nodes_case(pm):
    assert pm.num_nodes == 258 and pm.num_nodes % 4 != 0 and len(pm.leaves()) == 257
    assert all(len(m) in (1, 2) for v, m in enumerate(pm.nuc_muts) if v != pm.root)
    assert sum(len(m) == 2 for m in pm.nuc_muts) == 37


# The parameters of the GPU tests (tests/test_gpu_aa.py); tests/test_aa_cases.py runs every check
# over them without a GPU.  The windows depend on the strands and the slots, not on the ids; a
# block holds 360 characters on the root with slots and 300 without, so a reverse block's walk
# ranks 63 | 64 | 65 and 255 | 256 | 257 are the coordinates 63.., 423.., 783.. (363.., 663..) and
# 255.., 615.., 975.. (555.., 855..).
WIDE_STRANDS = ["+-+", "-+-", "---"]
WIDE_IDS = [(0, 1, 2), (0, 2, 5)]
WIDE_CASES = [(strands, ids, slots) for strands in WIDE_STRANDS for ids in WIDE_IDS for slots in (True, False)]
WIDE_WINDOWS = {
    ("+-+", True): [(63, 127), (64, 330), (65, 700), (255, 511), (256, 600), (5, 1070), (361, 420), (362, 700),
                    (0, 1079), (3, 423), (3, 1076), (73, 669), (260, 423), (260, 615), (361, 615), (383, 423), (423, 430),
                    (423, 850), (424, 431), (424, 1077), (425, 432), (615, 622), (616, 623), (617, 624), (718, 1009),
                    (720, 723), (722, 730), (725, 1000)],
    ("+-+", False): [(0, 899), (3, 364), (3, 896), (200, 363), (200, 556), (302, 607), (363, 370), (363, 730), (364, 371),
                     (364, 897), (365, 372), (555, 562), (555, 625), (556, 563), (556, 626), (557, 564), (557, 627),
                     (600, 603), (602, 610), (605, 820)],
    ("-+-", True): [(0, 64), (63, 127), (64, 330), (255, 511), (257, 1000), (5, 1070),
                    (0, 1079), (3, 783), (23, 63), (63, 70), (63, 490), (63, 1077), (64, 71), (64, 490), (65, 72), (255, 262),
                    (256, 263), (257, 264), (517, 864), (612, 1008), (620, 783), (720, 723), (721, 975), (722, 730),
                    (725, 1000), (783, 790), (784, 791), (785, 792), (898, 979), (975, 982), (976, 983), (977, 984)],
    ("-+-", False): [(0, 257), (0, 899), (3, 663), (63, 70), (63, 430), (63, 897), (64, 71), (64, 430), (65, 72), (255, 262),
                     (255, 325), (256, 263), (256, 326), (257, 264), (257, 327), (500, 663), (600, 603), (602, 610),
                     (605, 820), (663, 670), (664, 671), (665, 672), (855, 862), (856, 863), (857, 864)],
    ("---", True): [(0, 1079), (3, 424), (3, 783), (23, 63), (63, 70), (63, 490), (63, 1077), (64, 71), (64, 490), (65, 72),
                    (255, 262), (256, 263), (257, 264), (260, 423), (361, 615), (423, 430), (423, 850), (424, 431),
                    (424, 1077), (425, 432), (615, 622), (616, 623), (617, 624), (620, 783), (718, 986), (720, 723),
                    (722, 730), (725, 1000), (783, 790), (784, 791), (785, 792), (975, 982), (976, 983), (977, 984)],
    ("---", False): [(0, 257), (0, 899), (3, 364), (3, 663), (63, 70), (63, 430), (63, 897), (64, 71), (64, 430), (65, 72),
                     (200, 363), (255, 262), (255, 325), (256, 263), (256, 326), (257, 264), (257, 327), (363, 370),
                     (363, 730), (364, 371), (364, 897), (365, 372), (500, 663), (555, 562), (555, 625), (556, 563),
                     (556, 626), (557, 564), (557, 627), (600, 603), (602, 610), (605, 820), (663, 670), (664, 671),
                     (665, 672), (855, 862), (856, 863), (857, 864)],
}
WIDE_ERRORS = {   # the root's window is "ERROR": an end on a slot the walk leaves out, an end that wraps in front of the start
    ("+-+", True): [(346, 1032), (434, 1056), (372, 829), (571, 1045), (1035, 1105)],
    ("+-+", False): [(855, 925), (3, 901)],
    ("-+-", True): [(256, 600), (361, 420), (229, 421), (428, 648), (583, 708), (45, 468), (1035, 1105)],
    ("-+-", False): [(855, 925), (856, 926), (3, 901)],
    ("---", True): [(525, 527), (1035, 1105)],
    ("---", False): [(855, 925), (857, 927), (3, 901)],
}
MANY_BLOCKS_WINDOWS = [(439, 462), (448, 451), (890, 902), (3, 895), (434, 898), (0, 902), (441, 447), (443, 450),
                       (450, 456), (456, 460), (300, 445), (897, 901)]
