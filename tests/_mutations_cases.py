"""PanMATs for the mutation-printing tests (tests/test_mutations_ref.py and
tests/test_mutations_cases.py on the CPU, tests/test_gpu_mutations.py and tests/test_cli_mutations.py on
the GPU): hand cases with their expected lines, random cases and the shapes at the kernels' edges.

The builders below the hand cases plant shapes at the constants of pm_mutations.hip (kMutChunk = 256
columns per workgroup of the root map, kMutRound = 256 entries per round of k_mut_write, a wave of 64,
the digits of a coordinate); each has a check_* that proves from tests/_mutations_ref.py alone that
the shapes are there and that no case is Unsupported or skipped.  tests/test_mutations_cases.py runs
every check without a GPU, over the parameter lists at the end of this file."""
from __future__ import annotations

import numpy as np

import _mutations_ref
from _aa_cases import tree
from _maf_ref import _parents
from _panmat import random_panmat
from _trees import names_for, random_tree
from panman_amd.panmat import PanMAT

A, C, G, T, N = 1, 2, 4, 8, 15
NS, ND, NI, SNP, SNP_INS, SNP_DEL = 0, 1, 2, 3, 4, 5   # nucleotide mutation types
ROUND = 256   # kMutRound (pm_internal.h): entries per round of k_mut_write's workgroup
CHUNK = 256   # kMutChunk: columns per workgroup of the root map


# ---- hand cases: (PanMAT, {name: (substitutions, insertions, deletions)}, odd substitutions) ------------

def issue_case():
    """The issue's case: runs, a filled slot, a dropped NSNPD, a node without the block, an NSNPS over '-'."""
    pm = tree({"r": ["a", "b"], "a": ["c"]}, "r")
    pm.add_block(0, "ACGTACGTAC")
    pm.add_gaps(0, [(4, 2)])
    pm.add_block_mut(0, 0, True, False)
    a, b, c = pm.index("a"), pm.index("b"), pm.index("c")
    pm.add_nuc_mut(a, 0, 1, -1, NS, [G, T])
    pm.add_nuc_mut(a, 0, 4, 0, NI, [T, T])
    pm.add_nuc_mut(a, 0, 9, -1, SNP_DEL, [0])
    pm.add_nuc_mut(a, 0, 6, -1, ND, [0, 0])
    pm.add_nuc_mut(c, 0, 1, -1, SNP, [A])
    pm.add_nuc_mut(c, 0, 4, 0, ND, [0])
    pm.add_nuc_mut(c, 0, 6, -1, NS, [C])
    pm.add_nuc_mut(c, 0, 9, -1, SNP, [T])
    pm.add_block_mut(b, 0, False, False)
    pm.add_nuc_mut(b, 0, 0, -1, NS, [T])
    pm.add_nuc_mut(b, 0, 3, -1, NI, [A])
    want = {"a": (" > C2G > G3T", " > g5T > g5T", " > 7G > 8T"), "b": ("", " > 4A", ""), "c": (" > G2A > -10T", "", " > g5T")}
    return pm, want, 1


def reverse_root_case():
    """The root holds block 0 on the reverse strand with a filled slot: coordinates count down the
    columns (the sentinel first, a gap at coordinate 0), and the old base of a main position is the
    root's stored one."""
    pm = tree({"r": ["k"]}, "r")
    pm.add_block(0, "ACGT")
    pm.add_gaps(0, [(2, 1)])
    pm.add_block_mut(0, 0, True, True)
    pm.add_nuc_mut(0, 0, 2, 0, NI, [T])
    k = pm.index("k")
    pm.add_nuc_mut(k, 0, 0, -1, SNP, [C])     # walked last: coordinate 4
    pm.add_nuc_mut(k, 0, 3, -1, NS, [A])      # walked first after the sentinel: coordinate 0
    pm.add_nuc_mut(k, 0, 2, 0, ND, [0])       # the slot after G: coordinate 2
    pm.add_nuc_mut(k, 0, 4, -1, NI, [G])      # the sentinel: a gap at coordinate 0
    return pm, {"k": (" > A5C > T1A", " > g1G", " > 3T")}, 0


def absent_root_block_case():
    """The root does not hold block 1; m inserts it: one coordinate across the block and no g, also
    at its sentinel; m's own substitution reads the root's '-' and is skipped."""
    pm = tree({"r": ["m"], "m": ["n"]}, "r")
    pm.add_block(0, "ACG")
    pm.add_block(1, "TTTT")
    pm.add_block(2, "GG")
    pm.add_block_mut(0, 0, True, False)
    pm.add_block_mut(0, 2, True, False)
    m, n = pm.index("m"), pm.index("n")
    pm.add_block_mut(m, 1, True, False)
    pm.add_nuc_mut(m, 1, 2, -1, NS, [A])
    pm.add_nuc_mut(m, 1, 0, -1, NI, [G])
    pm.add_nuc_mut(n, 1, 1, -1, NS, [A, C])
    pm.add_nuc_mut(n, 1, 4, -1, ND, [0])
    pm.add_nuc_mut(n, 2, 1, -1, SNP, [C])     # block 2 starts at the same coordinate
    return pm, {"m": ("", " > 4G", ""), "n": (" > T4A > A4C > G5C", "", " > 4-")}, 0


def reverse_parent_case():
    """p inverts block 0 and changes position 1 to G; its child's substitution there prints the
    root's C as the old base (the quirk of :3835)."""
    pm = tree({"r": ["p"], "p": ["q"]}, "r")
    pm.add_block(0, "ACGT")
    pm.add_block_mut(0, 0, True, False)
    p, q = pm.index("p"), pm.index("q")
    pm.add_block_mut(p, 0, False, True)
    pm.add_nuc_mut(p, 0, 1, -1, SNP, [G])
    pm.add_nuc_mut(q, 0, 1, -1, SNP, [T])
    pm.add_nuc_mut(q, 0, 1, -1, ND, [0, 0])
    return pm, {"p": (" > C2G", "", ""), "q": (" > C2T", "", " > 2C > 3G")}, 0


def absent_parent_case():
    """d deletes block 0 and e inserts it again: against d every old base is '-', so e's run
    substitution is skipped and its deletion prints '-'."""
    pm = tree({"r": ["d"], "d": ["e"]}, "r")
    pm.add_block(0, "ACGT")
    pm.add_block_mut(0, 0, True, False)
    d, e = pm.index("d"), pm.index("e")
    pm.add_block_mut(d, 0, False, False)
    pm.add_block_mut(e, 0, True, False)
    pm.add_nuc_mut(e, 0, 0, -1, NS, [G, G])
    pm.add_nuc_mut(e, 0, 1, -1, ND, [0])
    return pm, {"d": ("", "", ""), "e": ("", "", " > 2-")}, 0


def dropped_case():
    """Single-base insertions and deletions make no entry."""
    pm = tree({"r": ["s"]}, "r")
    pm.add_block(0, "ACGT")
    pm.add_gaps(0, [(1, 1)])
    pm.add_block_mut(0, 0, True, False)
    s = pm.index("s")
    pm.add_nuc_mut(s, 0, 1, 0, SNP_INS, [G])
    pm.add_nuc_mut(s, 0, 2, -1, SNP_DEL, [0])
    return pm, {"s": ("", "", "")}, 0


def odd_case():
    """A single-base substitution over a base the parent deleted is kept and counted; a run
    substitution over it is skipped."""
    pm = tree({"r": ["f"], "f": ["g"]}, "r")
    pm.add_block(0, "ACGT")
    pm.add_block_mut(0, 0, True, False)
    f, g = pm.index("f"), pm.index("g")
    pm.add_nuc_mut(f, 0, 1, -1, ND, [0, 0])
    pm.add_nuc_mut(g, 0, 1, -1, SNP, [A])
    pm.add_nuc_mut(g, 0, 2, -1, NS, [T])
    return pm, {"f": ("", "", " > 2C > 3G"), "g": (" > -2A", "", "")}, 1


HAND = {"issue": issue_case, "reverse_root": reverse_root_case, "absent_root_block": absent_root_block_case,
        "reverse_parent": reverse_parent_case, "absent_parent": absent_parent_case, "dropped": dropped_case, "odd": odd_case}


def text_of(pm, want: dict) -> str:
    """The text of `want` ({name: three strings}; a node left out has three empty lines) in node-id order."""
    out = []
    for n in pm.names:
        s, i, d = want.get(n, ("", "", ""))
        out.append(f"Substitutions:\t{n}\t{s}\nInsertions:\t{n}\t{i}\nDeletions:\t{n}\t{d}\n")
    return "".join(out)


# ---- errors ------------------------------------------------------------------------------------------------

def unsupported_case():
    """u inverts block 1, which it does not hold: not held but flagged reverse."""
    pm = tree({"r": ["u"]}, "r")
    pm.add_block(0, "ACGT")
    pm.add_block(1, "GG")
    pm.add_block_mut(0, 0, True, False)
    pm.add_block_mut(pm.index("u"), 1, False, True)
    return pm


def secondary_case():
    pm, _, _ = odd_case()
    pm.add_nuc_mut(pm.index("g"), 0, 0, -1, SNP, [C], secondary=0)
    return pm


def beyond_block_case():
    """A run that ends past the sentinel."""
    pm, _, _ = odd_case()
    pm.add_nuc_mut(pm.index("g"), 0, 3, -1, NS, [A, A, A])
    return pm


def beyond_slots_case():
    """Slot 1 of a position with one slot."""
    pm, _, _ = dropped_case()
    pm.add_nuc_mut(pm.index("s"), 0, 1, 1, NI, [A])
    return pm


ARG_ERRORS = {"beyond_block": beyond_block_case, "beyond_slots": beyond_slots_case}
UNSUPPORTED = {"unheld_reverse": unsupported_case, "secondary": secondary_case}


# ---- tags: what a case's entries exercise -----------------------------------------------------------------

def tags_of(pm) -> set:
    """The kinds of entries and the skip rules a PanMAT exercises, read from the restatement's own
    pieces: S / I / D entries with and without g, on slots and main positions, a skipped run
    substitution by each rule, dropped single-base types, a kept odd substitution, the reverse quirk."""
    ref = _mutations_ref
    lists = ref._Lists(pm) if getattr(pm, "_arrays", None) is not None else pm
    entries, odd = ref.node_entry_lists(lists)
    parent = _parents(lists)
    max_id = max(b for b, _ in lists.blocks)
    is_block = {b for b, _ in lists.blocks}
    states = {}

    def state(v):
        if v not in states:
            states[v] = ref.NodeState(lists, ref._path(lists, parent, v), max_id, is_block)
        return states[v]

    tags = set()
    root = state(lists.root)
    for b in is_block:
        tags.add(("root", "held" if root.held[b] else "absent", "forward" if root.forward[b] else "reverse"))
    for v, es in enumerate(entries):
        for kind, _, old, _, gap in es:
            tags.add((kind, "g" if gap else "plain"))
            if kind == "D" and old == "-":
                tags.add("D over -")
        if v == lists.root:
            continue
        par = state(parent[v])
        me = state(v)
        for b, _, pos, g, info, _ in lists.nuc_muts[v]:
            typ, length = info & 7, info >> 4
            tags.add(("type", typ, "slot" if g != -1 else "main"))
            if typ in (SNP_INS, SNP_DEL):
                tags.add("dropped")
            if typ in (NS, SNP) and not me.held[b]:
                tags.add("S skipped: not held")
            if typ == NS and me.held[b]:
                for j in range(length):
                    cell = (b, pos, g + j) if g != -1 else (b, pos + j, -1)
                    if ref.seq_char(par, root, *cell) in "-x":
                        tags.add("S skipped: old -")
            if typ in (NS, ND, SNP) and g == -1 and par.held[b] and not par.forward[b]:
                tags.add("old from the root")
            if typ in (NS, ND, SNP) and not par.held[b]:
                tags.add("parent not held")
    if odd:
        tags.add("odd")
    return tags


# ---- random cases ------------------------------------------------------------------------------------------

def random_case(leaves, seed, blocks=6, block_len=(5, 40)):
    """A random PanMAT with every mutation type, block insertions, deletions and inversions.  An
    inversion of a block its node does not hold is Unsupported: such block mutations are dropped."""
    rng = np.random.default_rng(seed)
    off, idx, root = random_tree(leaves, rng, unary=0.1)
    pm = random_panmat(rng, off, idx, root, names_for(off), blocks=blocks, block_len=block_len, options=False)
    parent = _parents(pm)
    order = [pm.root]
    for v in order:
        order += [int(pm.child_index[e]) for e in range(pm.child_offsets[v], pm.child_offsets[v + 1])]
    held = {}
    for v in order:
        h = set(held[parent[v]]) if v != pm.root else set()
        kept = []
        for b, insertion, inversion in pm.block_muts[v]:
            if insertion:
                h.add(b)
            elif inversion:
                if b not in h:
                    continue
            else:
                h.discard(b)
            kept.append((b, insertion, inversion))
        pm.block_muts[v] = kept
        held[v] = h
    return pm


RANDOM = [(12, 1), (20, 2), (30, 3), (40, 4)]
RANDOM_TAGS = {("S", "plain"), ("S", "g"), ("I", "plain"), ("I", "g"), ("D", "plain"), ("D", "g"), "D over -", "dropped",
               "S skipped: not held", "S skipped: old -", "old from the root", "parent not held", "odd",
               ("root", "held", "forward"), ("root", "held", "reverse"), ("root", "absent", "forward")}


def check_random_cases():
    """Every random case runs (none Unsupported, none an ArgError) and between them they hold every
    kind of entry and every skip rule."""
    tags = set()
    for leaves, seed in RANDOM:
        pm = random_case(leaves, seed)
        text, _ = _mutations_ref.print_mutations(pm)
        assert text.count("\n") == 3 * pm.num_nodes
        tags |= tags_of(pm)
    missing = RANDOM_TAGS - tags
    assert not missing, missing
    for typ in range(6):
        assert ("type", typ, "main") in tags and ("type", typ, "slot") in tags, typ


# ---- entries per node: the rounds of k_mut_write -------------------------------------------------------

ENTRY_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 2 * ROUND + 5]


def _star(names, length, seed, slots=()):
    """One forward block of `length` random bases (slots: (position, count) pairs) under a root
    `r` with the leaves `names`."""
    rng = np.random.default_rng(seed)
    pm = tree({"r": list(names)}, "r")
    seq = "".join(rng.choice(list("ACGT"), size=length))
    pm.add_block(0, seq)
    if slots:
        pm.add_gaps(0, list(slots))
    pm.add_block_mut(0, 0, True, False)
    return pm, seq


def _other(ch, k=0):
    return [c for c in (A, C, G, T) if "-ACMGRSVT"[c] != ch][k % 3]


def entry_count_case():
    """Node e<n> has exactly n entries, all substitutions, single bases and runs of up to six mixed;
    the nodes between them have none."""
    names = []
    for n in ENTRY_COUNTS:
        names += [f"e{n}", f"z{n}"]
    pm, seq = _star(names, 700, seed=5)
    for n in ENTRY_COUNTS:
        v, at, k = pm.index(f"e{n}"), 0, 0
        while at < n:
            run = min(n - at, 1 + k % 6)
            if run == 1 and k % 2:
                pm.add_nuc_mut(v, 0, at, -1, SNP, [_other(seq[at])])
            else:
                pm.add_nuc_mut(v, 0, at, -1, NS, [_other(seq[at + j], j) for j in range(run)])
            at += run
            k += 1
    return pm


def check_entry_count_case():
    pm = entry_count_case()
    entries, odd = _mutations_ref.node_entry_lists(pm)
    assert odd == 0
    for n in ENTRY_COUNTS:
        assert len(entries[pm.index(f"e{n}")]) == n and not entries[pm.index(f"z{n}")]
        assert all(kind == "S" for kind, *_ in entries[pm.index(f"e{n}")])


def long_text_case():
    """Twelve leaves with 690 substitutions each: a text longer than a pipe's 64 KiB buffer."""
    names = [f"leaf{k}" for k in range(12)]
    pm, seq = _star(names, 700, seed=11)
    for k, nm in enumerate(names):
        for at in range(0, 690, 6):
            pm.add_nuc_mut(pm.index(nm), 0, at, -1, NS, [_other(seq[at + j], j + k) for j in range(6)])
    return pm


def check_long_text_case():
    text, odd = _mutations_ref.print_mutations(long_text_case())
    assert len(text) > 1 << 16 and odd == 0


def straddle_case():
    """Node w: 253 single substitutions, then a run of six insertions into slots that crosses the
    round's end (entries 253..258), deletions after it; its S, I and D lines all span two rounds of
    entries.  Nodes i, d and s hold entries of one section only, between nodes with none."""
    pm, seq = _star(["n0", "w", "n1", "i", "n2", "d", "n3", "s", "n4"], 600, seed=6, slots=[(300, 6), (310, 3)])
    w = pm.index("w")
    for at in range(253):
        pm.add_nuc_mut(w, 0, at, -1, SNP, [_other(seq[at])])
    pm.add_nuc_mut(w, 0, 300, 0, NI, [A, C, G, T, A, C])
    pm.add_nuc_mut(w, 0, 400, -1, ND, [0] * 6)
    pm.add_nuc_mut(w, 0, 310, 0, NI, [T, T, T])
    pm.add_nuc_mut(w, 0, 500, -1, NS, [_other(seq[500 + j]) for j in range(4)])
    pm.add_nuc_mut(pm.index("i"), 0, 310, 1, NI, [G, G])
    pm.add_nuc_mut(pm.index("d"), 0, 7, -1, ND, [0, 0, 0])
    pm.add_nuc_mut(pm.index("s"), 0, 9, -1, SNP, [_other(seq[9])])
    return pm


def check_straddle_case():
    pm = straddle_case()
    entries, _ = _mutations_ref.node_entry_lists(pm)
    kinds = [kind for kind, *_ in entries[pm.index("w")]]
    assert kinds[ROUND - 3:ROUND + 3] == ["I"] * 6 and kinds[ROUND - 4] == "S" and kinds[ROUND + 3] == "D"
    assert {"S", "I", "D"} == set(kinds[ROUND:]) and len(kinds) == 253 + 6 + 6 + 3 + 4
    for name, only in (("i", "I"), ("d", "D"), ("s", "S")):
        assert {kind for kind, *_ in entries[pm.index(name)]} == {only}
    for name in ("n0", "n1", "n2", "n3", "n4"):
        assert not entries[pm.index(name)]


# ---- coordinates: the digits --------------------------------------------------------------------------------

DIGIT_EDGES = [9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000]


def digits_case():
    """One block of 100,001 bases under three nodes: substitutions, insertions (into the sentinel's
    slot and over deleted bases) and deletions printed at 9/10 ... 99999/100000 and at 100001."""
    pm, seq = _star(["x", "y", "z"], 100001, seed=7)
    x, y, z = pm.index("x"), pm.index("y"), pm.index("z")
    for c in DIGIT_EDGES:
        pm.add_nuc_mut(x, 0, c - 1, -1, SNP, [_other(seq[c - 1])])
        pm.add_nuc_mut(y, 0, c - 1, -1, ND, [0])
        pm.add_nuc_mut(z, 0, c - 1, -1, NI, [N])
    pm.add_nuc_mut(x, 0, 100000, -1, NS, [_other(seq[100000])])
    pm.add_nuc_mut(z, 0, 100001, -1, NI, [A])      # the sentinel: g, one past the last base
    return pm, seq


def check_digits_case():
    pm, seq = digits_case()
    text, _ = _mutations_ref.print_mutations(pm)
    lines = text.split("\n")
    for c in DIGIT_EDGES:
        assert f" > {seq[c - 1]}{c}" in lines[3 * pm.index("x")]
        assert f" > {c}{seq[c - 1]}" in lines[3 * pm.index("y") + 2]
        assert f" > {c}N" in lines[3 * pm.index("z") + 1]
    assert lines[3 * pm.index("z") + 1].endswith(" > g100002A") and f" > {seq[100000]}100001" in lines[3 * pm.index("x")]


# ---- the root map: chunk edges in both directions, 130 blocks, 258 nodes, names --------------------------

ROOT_WIDTHS = [63, 64, 65, 257]


def root_map_case(seed=8):
    """130 blocks under 258 nodes with names of 1 to 40 bytes.  The first sixteen blocks have 63, 64,
    65 and 257 columns each in four forms -- held forward with filled and empty slots, held reverse
    with filled and empty slots, absent from the root (a child inserts it), absent and reverse at the
    child -- so that block and chunk edges of the root map fall at every offset; the rest are short.
    Every non-root node edits the first and last position, and a slot, of several blocks."""
    rng = np.random.default_rng(seed)
    n = 258
    def name(v):   # the id in letters, padded to 1 + v % 40 bytes
        code = chr(ord("A") + v % 26) + (chr(ord("A") + v // 26) if v >= 26 else "")
        return code + "_" * (1 + v % 40 - len(code))

    names = ["r"] + [name(v) for v in range(1, n)]
    assert len(set(names)) == n
    off, idx = [0], []
    for v in range(n):   # node v's children: 2 v + 1, 2 v + 2 (a complete binary tree)
        idx += [k for k in (2 * v + 1, 2 * v + 2) if k < n]
        off.append(len(idx))
    pm = PanMAT(names, np.array(off, np.int32), np.array(idx, np.int32), 0)
    shapes = []   # (block, bases, slots {position: count}, form)
    b = 0
    forms = ["forward", "reverse", "absent", "absent_reverse"]
    for i, width in enumerate(ROOT_WIDTHS):
        for form in forms[i:] + forms[:i]:                     # (so that each form meets a chunk edge)
            slots = {2: 3, width // 2: 2}                      # 5 slot columns, the sentinel one more
            bases = width - 6
            shapes.append((b, bases, slots, form))
            b += 1
    while b < 130:
        shapes.append((b, int(rng.integers(3, 9)), {1: 1} if b % 3 == 0 else {}, "forward" if b % 5 else "reverse"))
        b += 1
    seqs = {}
    for b, bases, slots, form in shapes:
        seqs[b] = "".join(rng.choice(list("ACGT"), size=bases))
        pm.add_block(b, seqs[b])
        if slots:
            pm.add_gaps(b, sorted(slots.items()))
        if form in ("forward", "reverse"):
            pm.add_block_mut(0, b, True, form == "reverse")
            for pos, cnt in slots.items():                      # the first of a position's slots filled, the others empty
                pm.add_nuc_mut(0, b, pos, 0, SNP_INS, [G])
        else:
            pm.add_block_mut(1, b, True, form == "absent_reverse")   # node 1 and its subtree hold it
    for v in range(1, n):
        for k in range(3):
            b, bases, slots, form = shapes[(7 * v + 5 * k) % len(shapes)]
            pos = [0, bases - 1, bases][k]                      # first base, last base, the sentinel
            if k == 2:
                pm.add_nuc_mut(v, b, pos, -1, NI, [_other("A", v)])
            elif v % 2:
                pm.add_nuc_mut(v, b, pos, -1, SNP, [_other(seqs[b][pos], v)])
            else:
                pm.add_nuc_mut(v, b, pos, -1, ND, [0])
            if slots:
                p0 = sorted(slots)[v % len(slots)]
                pm.add_nuc_mut(v, b, p0, slots[p0] - 1, NI, [T])   # the position's last slot
                pm.add_nuc_mut(v, b, p0, 0 if v % 3 else slots[p0] - 1, ND, [0])   # slot 0 is filled at the root where it holds the block
    return pm, shapes


def check_root_map_case():
    pm, shapes = root_map_case()
    assert pm.num_nodes == 258 and len(pm.blocks) == 130
    assert {len(nm) for nm in pm.names} == set(range(1, 41))
    lists = pm
    ref = _mutations_ref
    root = ref.NodeState(lists, [0], 129, set(range(130)))
    widths = {}
    for b, bases, slots, form in shapes[:16]:
        widths.setdefault(sum(1 + len(s) for _, s in root.seq[b]), set()).add(
            (root.held[b], root.forward[b], any(ch != "-" for _, s in root.seq[b] for ch in s)))
    assert sorted(widths) == ROOT_WIDTHS
    for w in ROOT_WIDTHS:   # held forward and held reverse with filled slots (and empty ones beside them), absent
        assert widths[w] == {(True, True, True), (True, False, True), (False, True, False)}, widths[w]
    tags = tags_of(pm)
    assert {("S", "plain"), ("I", "plain"), ("I", "g"), ("D", "plain"), ("D", "g"), "D over -", "old from the root",
            "parent not held", ("root", "held", "forward"), ("root", "held", "reverse"), ("root", "absent", "forward")} <= tags
    text, _ = ref.print_mutations(pm)
    assert text.count("\n") == 3 * 258
    # a chunk edge of the root map falls inside a forward, a reverse and an absent block
    at, inside = 0, set()
    for b, bases, slots, form in shapes:
        w = sum(1 + len(s) for _, s in root.seq[b])
        if at // CHUNK != (at + w - 1) // CHUNK:
            inside.add(form)
        at += w
    assert {"forward", "reverse", "absent", "absent_reverse"} <= inside, inside
