"""PanMATs for the UShER export tests (tests/test_usher_ref.py and tests/test_usher_cases.py on the CPU,
tests/test_gpu_usher.py and tests/test_cli_usher.py on the GPU): hand cases with their bytes written
out, and the shapes at the kernels' edges.

The builders plant shapes at the constants of pm_usher.hip (kUsherRound = 256 entries per round of
k_usher_write, a wave of 64, the varint steps of a position and of a node's length L); each has a
check_* that proves from tests/_usher_ref.py alone that the shapes are there.
tests/test_usher_cases.py runs every check without a GPU.  The entry-count, straddle, long-text,
258-node and random PanMATs are those of tests/_mutations_cases.py: kMutRound is 256 as well."""
from __future__ import annotations

import numpy as np

import _usher_ref
from _aa_cases import tree
from _mutations_cases import (ENTRY_COUNTS, _other, _star, beyond_block_case, beyond_slots_case, entry_count_case,
                              long_text_case, random_case, root_map_case, secondary_case, straddle_case)

A, C, G, T, R, N = 1, 2, 4, 8, 5, 15
NS, ND, NI, SNP, SNP_INS, SNP_DEL = 0, 1, 2, 3, 4, 5   # nucleotide mutation types
ROUND = 256   # kUsherRound (pm_internal.h)


def hx(text: str) -> bytes:
    return bytes.fromhex(text)


# ---- hand cases: (PanMAT, the bytes) ------------------------------------------------------------------------
# Block 0 is "ACGT" with two gap slots before position 2, so its cells and positions (getCoordMap,
# src/panman2usher.cpp:37-48) are: A 1, C 2, slot 3, slot 4, G 5, T 6, the sentinel 7.
# Nodes come in pre-order r, a, b (getNodeDFS :289, :540-542); an empty node is 12 00.

NEWICK3 = b"\x0a\x22(a:1.000000,b:1.000000)r:0.000000;"                  # 34 bytes of text
NEWICK4 = b"\x0a\x2e((c:1.000000)a:1.000000,b:1.000000)r:0.000000;"      # 46 bytes of text


def _three():
    pm = tree({"r": ["a", "b"]}, "r")
    pm.add_block(0, "ACGT")
    pm.add_gaps(0, [(2, 2)])
    pm.add_block_mut(0, 0, True, False)
    return pm, pm.index("a"), pm.index("b")


def substitution_case():
    """NS of one base over the consensus C (:354-385): position 2, ref C = 2, par C = 2, mut_nuc {G} = {2}."""
    pm, a, _ = _three()
    pm.add_nuc_mut(a, 0, 1, -1, NS, [G])
    return pm, NEWICK3 + hx("1200") + hx("120b 0a09 0802 1002 1802 220102") + hx("1200")


def slot_insertion_case():
    """NI of two bases into the empty slots (:389-403): ref and par are code('-') = 0, so both fields are absent."""
    pm, a, _ = _three()
    pm.add_nuc_mut(a, 0, 2, 0, NI, [T, T])
    return pm, NEWICK3 + hx("1200") + hx("120e 0a05 0803 220103 0a05 0804 220103") + hx("1200")


def deletion_run_case():
    """ND of two bases (:436-449): newVal stays '-' (:344), whose code 0 reads as N: mut_nuc 0, 1, 2, 3."""
    pm, a, _ = _three()
    pm.add_nuc_mut(a, 0, 0, -1, ND, [0, 0])
    return pm, (NEWICK3 + hx("1200") + hx("121c 0a0c 0801 1001 1801 220400010203 0a0c 0802 1002 1802 220400010203")
                + hx("1200"))


def iupac_and_zero_case():
    """NS with the codes R = 5 (bits 0 and 2) and 0 ('-', whose code 0 reads as N, get_nuc :161-212)."""
    pm, a, _ = _three()
    pm.add_nuc_mut(a, 0, 0, -1, NS, [R, 0])
    return pm, NEWICK3 + hx("1200") + hx("121a 0a0a 0801 1001 1801 22020002 0a0c 0802 1002 1802 220400010203") + hx("1200")


def sentinel_case():
    """NSNPI at the sentinel (:496-507): position 7, ref and par code('x') = 0."""
    pm, a, _ = _three()
    pm.add_nuc_mut(a, 0, 4, -1, SNP_INS, [A])
    return pm, NEWICK3 + hx("1200") + hx("1207 0a05 0807 220100") + hx("1200")


def type_six_case():
    """A mutation of type 6 meets no branch of :346-537: an empty list."""
    pm, a, _ = _three()
    pm.add_nuc_mut_raw(a, 0, 1, -1, (1 << 4) | 6, G << 20)
    return pm, NEWICK3 + hx("1200") + hx("1200") + hx("1200")


def root_list_case():
    """The root's own NSNPS of T to A at position 6 (par from the pseudo-root), seen as par by both children:
    a deletes it (NSNPD, :523-534), b substitutes it."""
    pm, a, b = _three()
    pm.add_nuc_mut(0, 0, 3, -1, SNP, [A])
    pm.add_nuc_mut(a, 0, 3, -1, SNP_DEL, [0])
    pm.add_nuc_mut(b, 0, 3, -1, SNP, [C])
    return pm, (NEWICK3 + hx("120b 0a09 0806 1008 1808 220100") + hx("120e 0a0c 0806 1008 1801 220400010203")
                + hx("120b 0a09 0806 1008 1801 220101"))


def rewritten_cell_case():
    """a writes position 1 twice (A to G, then G to T: the second par is the first's new base, :374-376); its
    child c deletes the T; b, visited after a's subtree was undone (:553-560), sees the A again.  Pre-order
    r, a, c, b differs from the id order r, a, b, c."""
    pm = tree({"r": ["a", "b"], "a": ["c"]}, "r")
    pm.add_block(0, "ACGT")
    pm.add_block_mut(0, 0, True, False)
    a, b, c = pm.index("a"), pm.index("b"), pm.index("c")
    pm.add_nuc_mut(a, 0, 0, -1, SNP, [G])
    pm.add_nuc_mut(a, 0, 0, -1, NS, [T])
    pm.add_nuc_mut(c, 0, 0, -1, ND, [0])
    pm.add_nuc_mut(b, 0, 0, -1, SNP, [C])
    return pm, (NEWICK4 + hx("1200") + hx("1216 0a09 0801 1001 1801 220102 0a09 0801 1001 1804 220103")
                + hx("120e 0a0c 0801 1001 1808 220400010203") + hx("120b 0a09 0801 1001 1801 220101"))


def block_mutations_case():
    """The substitution case with a second block that a deletes and b inverts, and block 0 deleted at a:
    block mutations are tracked (:294-333) and never read, so a's mutation of the block it does not hold
    is written all the same.  Block 1 "GG" adds the cells 8, 9, 10."""
    pm, a, b = _three()
    pm.add_block(1, "GG")
    pm.add_block_mut(0, 1, True, True)
    pm.add_block_mut(a, 0, False, False)
    pm.add_block_mut(a, 1, False, False)
    pm.add_block_mut(b, 1, False, True)
    pm.add_nuc_mut(a, 0, 1, -1, NS, [G])
    pm.add_nuc_mut(b, 1, 1, -1, SNP, [T])
    return pm, NEWICK3 + hx("1200") + hx("120b 0a09 0802 1002 1802 220102") + hx("120b 0a09 0809 1004 1804 220103")


def single_node_case():
    """A tree of its root alone: the newick is the bare identifier without ';' (getNewickString,
    src/panman.cpp:1930-1933), and the root's NSNPS reads its par from the pseudo-root."""
    pm = tree({"r": []}, "r")
    pm.add_block(0, "ACGT")
    pm.add_block_mut(0, 0, True, False)
    pm.add_nuc_mut(0, 0, 0, -1, SNP, [G])
    return pm, hx("0a01 72") + hx("120b 0a09 0801 1001 1801 220102")


HAND = {"single_node": single_node_case, "substitution": substitution_case, "slot_insertion": slot_insertion_case, "deletion_run": deletion_run_case,
        "iupac_and_zero": iupac_and_zero_case, "sentinel": sentinel_case, "type_six": type_six_case,
        "root_list": root_list_case, "rewritten_cell": rewritten_cell_case, "block_mutations": block_mutations_case}


def without_block_mutations(pm):
    """The same PanMAT with every block mutation dropped (list-built PanMATs only)."""
    for v in range(pm.num_nodes):
        pm.block_muts[v] = []
    return pm


# ---- errors ------------------------------------------------------------------------------------------------

ARG_ERRORS = {"beyond_block": beyond_block_case, "beyond_slots": beyond_slots_case}
UNSUPPORTED = {"secondary": secondary_case}

# ---- random cases: those of the mutation-printing tests (block insertions, deletions, inversions, all six types)

RANDOM = [(20, 2), (30, 3), (40, 4)]


def check_random_cases():
    types = set()
    for leaves, seed in RANDOM:
        pm = random_case(leaves, seed)
        assert any(pm.block_muts[v] for v in range(pm.num_nodes) if v != pm.root)
        assert all(sec == -1 for muts in pm.nuc_muts for _, sec, *_ in muts)
        types |= {info & 7 for muts in pm.nuc_muts for *_, info, _ in muts}
        data, count = _usher_ref.to_usher(pm)
        text, nodes = _usher_ref.decode(data)
        assert len(nodes) == pm.num_nodes and sum(map(len, nodes)) == count > 0
        assert _usher_ref.to_usher(without_block_mutations(random_case(leaves, seed)))[0] == data
    assert {0, 1, 2, 3, 4, 5} <= types


def _preorder(pm):
    order, stack = [], [pm.root]
    while stack:
        v = stack.pop()
        order.append(v)
        stack += [int(pm.child_index[e]) for e in range(pm.child_offsets[v + 1] - 1, pm.child_offsets[v] - 1, -1)]
    return order


def records_of(pm, name):
    """The records of the node called `name`."""
    return _usher_ref.node_lists(pm)[_preorder(pm).index(pm.index(name))]


def check_entry_count_case():
    pm = entry_count_case()
    assert ENTRY_COUNTS == [0, 1, 63, 64, 65, 255, 256, 257, 2 * ROUND + 5]
    for n in ENTRY_COUNTS:
        assert len(records_of(pm, f"e{n}")) == n and not records_of(pm, f"z{n}")


def check_straddle_case():
    """Entries 253..258 of node w are one run of six insertions into slots: it crosses the round's end."""
    pm = straddle_case()
    recs = records_of(pm, "w")
    assert len(recs) == 253 + 6 + 6 + 3 + 4
    run = recs[ROUND - 3:ROUND + 3]
    assert all(ref == 0 and par == 0 for _, ref, par, _ in run) and [p for p, *_ in run] == list(range(run[0][0], run[0][0] + 6))
    assert recs[ROUND - 4][1] != 0


def check_long_case():
    data, count = _usher_ref.to_usher(long_text_case())
    assert len(data) > 1 << 16 and count == 12 * 690


def check_permuted_case():
    """258 nodes in a complete binary tree numbered level by level, 130 blocks, names of 1 to 40 bytes, block
    insertions, deletions and inversions: pre-order differs from id order."""
    pm, _ = root_map_case()
    assert pm.num_nodes == 258 and len(pm.blocks) == 130
    order = _preorder(pm)
    assert order != sorted(order) and sorted(order) == list(range(258))
    lists = _usher_ref.node_lists(pm)
    assert sum(1 for m in lists if m) >= 257
    assert any(inversion for muts in pm.block_muts for _, _, inversion in muts)


# ---- positions on both sides of the varint steps ----------------------------------------------------------

POSITION_EDGES = [127, 128, 16383, 16384]
WIDE = 16390   # bases of block 0: positions 1 .. 16391 (the sentinel), then block 1


def position_case():
    """Block 0 of 16,390 bases and block 1 of ten: single-base mutations at positions 127, 128, 16383 and
    16384, at block 0's sentinel and in block 1 (positions past 16391), over two nodes."""
    rng = np.random.default_rng(21)
    pm = tree({"r": ["p", "q"]}, "r")
    seq = "".join(rng.choice(list("ACGT"), size=WIDE))
    pm.add_block(0, seq)
    pm.add_block(1, "ACGTACGTAC")
    pm.add_block_mut(0, 0, True, False)
    pm.add_block_mut(0, 1, True, False)
    p, q = pm.index("p"), pm.index("q")
    for at in POSITION_EDGES:
        pm.add_nuc_mut(p, 0, at - 1, -1, SNP, [_other(seq[at - 1])])
        pm.add_nuc_mut(q, 0, at - 1, -1, SNP_DEL, [0])
    pm.add_nuc_mut(p, 0, WIDE, -1, NI, [A])                 # the sentinel: position 16391
    pm.add_nuc_mut(p, 1, 0, -1, NS, [T, T, T])              # positions 16392 ..
    pm.add_nuc_mut(q, 1, 9, -1, NS, [G, G])                 # ... 16401 and block 1's sentinel, 16402
    return pm


def check_position_case():
    pm = position_case()
    p, q = records_of(pm, "p"), records_of(pm, "q")
    assert [r[0] for r in p] == POSITION_EDGES + [WIDE + 1, WIDE + 2, WIDE + 3, WIDE + 4]
    assert [r[0] for r in q] == POSITION_EDGES + [WIDE + 11, WIDE + 12]
    assert q[-1][1] == 0 and p[4][1] == 0                   # the sentinels: ref 0


# ---- a node's length L on both sides of its varint steps --------------------------------------------------

LIST_LENGTHS = [127, 128, 16383, 16384]


def _mix(total, small):
    """(x, y): x records of `small` bytes and y of small + 1 make `total` bytes, y the least possible."""
    for y in range(small):
        if (total - y * (small + 1)) % small == 0 and total >= y * (small + 1):
            return (total - y * (small + 1)) // small, y
    raise AssertionError((total, small))


def list_length_case():
    """Node l<L>'s list body is exactly L bytes.  A single-base substitution over a base is 11 bytes wrapped
    at a position below 128 and 12 from 128 on (0a len 08 position 10 ref 18 par 22 01 bit); with a new code of
    two bits (R) it is one byte more.  x plain and y two-bit records with x * s + y * (s + 1) = L are chosen
    here on the CPU: L = 127 and 128 below position 128, L = 16383 and 16384 (about 1365 records) from 128 on."""
    pm, seq = _star([f"l{n}" for n in LIST_LENGTHS] + ["none"], 1700, seed=22)
    for total in LIST_LENGTHS:
        v = pm.index(f"l{total}")
        small, first = (11, 0) if total < 1000 else (12, 127)
        x, y = _mix(total, small)
        for k in range(x + y):
            at = first + k
            two_bits = k >= x
            code = R if two_bits else _other(seq[at])
            pm.add_nuc_mut(v, 0, at, -1, SNP, [code])
    return pm


def check_list_length_case():
    pm = list_length_case()
    for total in LIST_LENGTHS:
        recs = records_of(pm, f"l{total}")
        body = b"".join(_usher_ref.f_bytes(1, _usher_ref.encode_mut(*r)) for r in recs)
        assert len(body) == total, (total, len(body))
        assert total < 1000 or 1300 < len(recs) < 1500
    assert not records_of(pm, "none")


# ---- codes, runs and rewritten cells ----------------------------------------------------------------------

def codes_case():
    """Node m: all 16 codes as substitution runs over bases (ref and par non-zero) and as insertion runs into
    16 empty slots (ref and par zero); a substitution run that ends at the sentinel; node d deletes slots that
    m's sibling s filled (par non-zero over ref zero)."""
    pm, seq = _star(["m", "s"], 40, seed=23, slots=[(20, 16)])
    pm = _with_child(pm, "s", "d")
    m, s, d = pm.index("m"), pm.index("s"), pm.index("d")
    for lo, hi in ((0, 6), (6, 12), (12, 16)):
        pm.add_nuc_mut(m, 0, lo, -1, NS, list(range(lo, hi)))
        pm.add_nuc_mut(m, 0, 20, lo, NI, list(range(lo, hi)))
    pm.add_nuc_mut(m, 0, 38, -1, NS, [_other(seq[38]), _other(seq[39]), A])   # positions 38, 39 and the sentinel 40
    pm.add_nuc_mut(s, 0, 20, 3, NI, [A, C, G])
    pm.add_nuc_mut(d, 0, 20, 2, ND, [0, 0, 0, 0, 0])                          # slots 2 .. 6: over '-', A, C, G, '-'
    return pm


def _with_child(pm, parent, child):
    """`pm`'s tree with one more leaf under `parent` (before any mutation is added)."""
    kids = {n: [pm.names[int(pm.child_index[e])] for e in range(pm.child_offsets[v], pm.child_offsets[v + 1])]
            for v, n in enumerate(pm.names)}
    kids[parent] = kids[parent] + [child]
    out = tree({n: k for n, k in kids.items() if k}, pm.names[pm.root])
    out.blocks, out.gaps = pm.blocks, pm.gaps
    out.block_muts[out.root] = list(pm.block_muts[pm.root])
    return out


def check_codes_case():
    pm = codes_case()
    m = records_of(pm, "m")
    over_bases = [r for r in m if r[1] and r[2]]
    into_slots = [r for r in m if not r[1] and not r[2]]
    sets = lambda recs: {sum(1 << k for k in bits) for _, _, _, bits in recs}
    assert sets(over_bases) == set(range(1, 16)) and sets(into_slots[:16]) == set(range(1, 16))
    assert sum(1 for r in over_bases[:16] if r[3] == [0, 1, 2, 3]) == 2          # the codes 0 and 15
    char, position = _usher_ref.pseudo_root(pm)
    assert m[-1][0] == position[0, 40, -1] and m[-1][1] == 0 and m[-1][2] == 0   # the run ends at the sentinel
    d = records_of(pm, "d")
    assert [(ref, par) for _, ref, par, _ in d] == [(0, 0), (0, A), (0, C), (0, G), (0, 0)]


def rewrite_case():
    """Cells written again within one list, among nodes that write every cell once:
    u   SNP at 5, then an NS run 4..6 covering it, then an ND run 5..7: position 6 is written three times
    v   (u's child) a deletion at 20, then an insertion there; and at 5, which its parent u left '-', an
        insertion and then a substitution: the cell is also written by the parent
    w   a slot filled, substituted and deleted in one list; x, y, z and the 30 leaves k0.. write no cell twice."""
    names = ["u", "x", "w", "y", "z"] + [f"k{i}" for i in range(30)]
    pm, seq = _star(names, 60, seed=24, slots=[(10, 2)])
    pm = _with_child(pm, "u", "v")
    u, v, w = pm.index("u"), pm.index("v"), pm.index("w")
    pm.add_nuc_mut(u, 0, 5, -1, SNP, [_other(seq[5])])
    pm.add_nuc_mut(u, 0, 4, -1, NS, [_other(seq[4], 1), _other(seq[5], 1), _other(seq[6], 1)])
    pm.add_nuc_mut(u, 0, 5, -1, ND, [0, 0, 0])
    pm.add_nuc_mut(v, 0, 20, -1, SNP_DEL, [0])
    pm.add_nuc_mut(v, 0, 20, -1, SNP_INS, [N])
    pm.add_nuc_mut(v, 0, 5, -1, SNP_INS, [N])
    pm.add_nuc_mut(v, 0, 5, -1, SNP, [A])
    pm.add_nuc_mut(v, 0, 30, -1, SNP, [_other(seq[30])])
    pm.add_nuc_mut(w, 0, 10, 1, SNP_INS, [G])
    pm.add_nuc_mut(w, 0, 10, 0, NS, [A, T])
    pm.add_nuc_mut(w, 0, 10, 1, SNP_DEL, [0])
    for i, name in enumerate(["x", "y", "z"] + [f"k{i}" for i in range(30)]):
        n = pm.index(name)
        pm.add_nuc_mut(n, 0, i, -1, NS, [_other(seq[i + j], i) for j in range(3)])
        pm.add_nuc_mut(n, 0, 5 + i, -1, SNP_DEL, [0])
    return pm


def check_rewrite_case():
    pm = rewrite_case()
    code = {c: k for k, c in enumerate("-ACMGRSVTWYHKDBN")}
    seq = _star(["q"], 60, seed=24)[1]
    u = records_of(pm, "u")
    at6 = [r for r in u if r[0] == 6]
    assert len(at6) == 3 and at6[0][2] == code[seq[5]] and at6[1][2] == _other(seq[5]) and at6[2][2] == _other(seq[5], 1)
    v = records_of(pm, "v")
    assert [(r[0], r[2]) for r in v] == [(23, code[seq[20]]), (23, 0), (6, 0), (6, N), (33, code[seq[30]])]   # (two slots lie before base 10) u left '-' at 6
    w = records_of(pm, "w")
    slot1 = [r for r in w if r[0] == w[0][0]]
    assert [(ref, par) for _, ref, par, _ in slot1] == [(0, 0), (0, G), (0, T)]
    for name in ["x", "y", "z", "k0", "k29"]:
        recs = records_of(pm, name)
        assert recs and len({r[0] for r in recs}) == len(recs)


def one_node_batches_case():
    """Seven nodes, the root among them, of 60 records each: more than half of a 4096-byte batch, so every
    batch holds one node."""
    names = [f"t{i}" for i in range(6)]
    pm, seq = _star(names, 100, seed=25)
    for k, v in enumerate([0] + [pm.index(n) for n in names]):
        for at in range(0, 60, 6):
            pm.add_nuc_mut(v, 0, at + k, -1, NS, [_other(seq[at + k + j], j + k) for j in range(6)])
    return pm


def check_one_node_batches_case():
    lists = _usher_ref.node_lists(one_node_batches_case())
    assert [len(m) for m in lists] == [60] * 7
