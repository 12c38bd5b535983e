"""PanMATs for the reroot tests: the hand cases that pin the oracle's restatement (oracle/pm_oracle.cpp,
reroot_dump) and pm_reroot to src/reroot.cpp:4-262 -- in the from_fixture dict format with branch lengths in
the Newick text, the expected dump worked out by hand from the reference's code -- and builders for the edges
of pm_reroot's kernels and host steps (topology, block states, column counts, NucMut runs, column chunks).
Every builder states the property that makes it an edge case; check() asserts it on a dump.

What the derivations below use of the reference:

  transform / transformHelper (src/panman.cpp:5831-5906).  With the tip's parent the root, only the tip's
  length changes, to 0 (:5873-5876).  Otherwise a new root "node_<internal nodes + 1>" (:5890, newInternalNodeId
  src/panman.hpp:793) takes the tip (length 0) and the tip's old parent, which takes the tip's old length; every
  node on the way up takes its old parent as its last child, the parent getting the node's old length.  Both go
  through `size_t oldBranchLen` (:5855, :5888), so a moved length loses its fraction.  The old root stays when
  it keeps two children or more (:5833-5835); with one it is deleted and that child moves up (:5837-5841).

  States (src/reroot.cpp:59-78, :176-186, :202-212): a block is 1 absent, 2 forward, 4 reversed; a character is
  1 << code ('-' and 'x' 1, A 2, C 4, G 16, T 256).  The forward pass (src/fitchSankoff.cpp:30-56, :224-245)
  gives a node the AND of its children's states or, when that is empty, the OR.  The backward pass (:96-129,
  :247-270) forces the root to the new root's own state; any other node takes its parent's state when it holds
  it and its lowest set bit otherwise.  A node whose state differs from its parent's gets a mutation
  (:131-171, :272-308): parent 1 an insertion (NI 2; a block: BI, inverted when the state is 4), own state 1 a
  deletion (ND 1; a block: BD), anything else a substitution (NS 0; a block: BD with the inversion flag).  The
  root's parent state is 1 for a block (src/reroot.cpp:82, :116) and for a gap slot (:190), and
  1 << code(consensus) for a main position (:216), the consensus ending in '-' (:165).

  Runs (src/reroot.cpp:226-262, NucMut(vector<tuple6>, start, end) src/panman.hpp:154-189): per node the sorted
  main tuples, then the sorted gap tuples; a run ends after 6 codes, at another block or type, at a position
  that is not the next one (main) or at another position or a slot that is not the next one (gap).  A record is
  block, position, slot or -1, (length << 4) + type, and the codes from bit 20 down, four bits each.

Dump lines (tests/_panmat.py tree_dump): the Newick text, then per node in name order "B block insertion
inversion" sorted by block and "N block position slot info codes" in list order."""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

from _panmat import from_fixture
from _trees import CODE, parse_newick
from panman_amd.panmat import PanMAT


def newick_lengths(text: str, default: float = 0.0) -> np.ndarray:
    """The branch lengths of a Newick text in the node order of _trees.parse_newick and
    _panmat._parse_labelled (pre-order); a node without one gets `default`."""
    text = text.strip().rstrip(";")
    lens, stack, last, i = [], [], None, 0
    while i < len(text):
        c = text[i]
        if c == "(":
            stack.append(len(lens))
            lens.append(default)
            last = None
            i += 1
        elif c == ",":
            last = None
            i += 1
        elif c == ")":
            last = stack.pop()
            i += 1
        elif c == ":":
            j = i + 1
            while j < len(text) and text[j] not in ",()":
                j += 1
            lens[last] = float(text[i + 1:j])
            i = j
        else:
            j = i
            while j < len(text) and text[j] not in ",():":
                j += 1
            if last is None:      # a tip's name (a label behind ')' names the node just closed)
                last = len(lens)
                lens.append(default)
            i = j
    return np.array(lens, np.float32)


def _case(newick, blocks, block_muts, nuc_muts=None, gaps=()):
    return {"newick": newick, "blocks": blocks, "gaps": list(gaps), "block_muts": block_muts, "nuc_muts": nuc_muts or {},
            "rotation": {}, "inverted": {}, "circular": {}}


def hand_panmat(case: dict) -> PanMAT:
    pm = from_fixture(case)
    pm.branch_length = newick_lengths(case["newick"])
    return pm


def _dump(newick, *lines):
    return "newick\t" + newick + "\n" + "".join(line.replace(" ", "\t") + "\n" for line in lines)


# Mutation lists: [block, position, gap slot or -1, type, codes]; type 3 substitutes one base, 4 inserts one
# (a gap slot, or the end sentinel), 5 deletes one; codes A 1, C 2, G 4, T 8.  parse_newick names the internal
# nodes node_1, node_2, ... in the order of their '('.
HAND = {
    # node_1 = root (node_2, c), node_2 = (a, b).  a leaves node_2; oldBranchLen = (size_t)1.5 = 1.  node_3 is
    # the new root.  transformHelper(node_2): it leaves node_1, oldBranchLen = (size_t)3.25 = 3;
    # transformHelper(node_1) finds one child left, c: c's length is 0, node_1 is deleted, c returned.  node_2
    # takes c with length 3, node_3 takes node_2 with length 1.  b never moved: 2.75.  All three tips hold block
    # 0 forward with its consensus: every state is 2, the root differs from its parent state 1: BI, forward.
    "A_fractional_lengths_two_child_root": (
        _case("((a:1.5,b:2.75):3.25,c:4.5);", [[0, "A"]], {"node_1": [[0, 1, 0]]}), "a",
        _dump("(a:0.000000,(b:2.750000,c:3.000000)node_2:1.000000)node_3:0.000000;",
              "node_3 B 0 1 0")),
    # node_1 = root (node_2, c, e) with length 9.5, node_2 = (node_3, d), node_3 = (a, b).  a: (size_t)1.5 = 1.
    # node_3 leaves node_2 with (size_t)3.75 = 3, node_2 leaves node_1 with (size_t)0.875 = 0; node_1 keeps c
    # and e, so it stays, its length set to 0 (:5834).  node_2 takes node_1 with length 0, node_3 takes node_2
    # with 3, the new root node_4 takes node_3 with 1.
    "B_fractional_lengths_three_child_root": (
        _case("(((a:1.5,b:2.5):3.75,d:0.5):0.875,c:4.5,e:2.25):9.5;", [[0, "A"]], {"node_1": [[0, 1, 0]]}), "a",
        _dump("(a:0.000000,(b:2.500000,(d:0.500000,(c:4.500000,e:2.250000)node_1:0.000000)node_2:3.000000)node_3:1.000000)"
              "node_4:0.000000;",
              "node_4 B 0 1 0")),
    # c hangs under the root: only c's length changes (:5873-5876); node_1 keeps its 0.5.  The mutations are
    # still made anew with node_1 forced to c's characters "AC".  Column 0: a 2, b 16 (G), c 2; node_2 = 2 | 16
    # = 18, node_1 forced to 2 = its parent state (consensus A); node_2 holds 2 and takes it, a too, b does not:
    # 16, a substitution, code 4.
    "C_parent_is_the_root": (
        _case("((a:1.5,b:2.75):3.25,c:4.5):0.5;", [[0, "AC"]], {"node_1": [[0, 1, 0]]}, {"b": [[0, 0, -1, 3, [4]]]}), "c",
        _dump("((a:1.500000,b:2.750000)node_2:3.250000,c:0.000000)node_1:0.500000;",
              "b N 0 0 -1 16 400000",
              "node_1 B 0 1 0")),
    # node_1 = root (node_2, c, d), node_2 = (node_3) unary, node_3 = (a, b).  a: (size_t)2.5 = 2.  node_3 leaves
    # node_2 (no child left) with (size_t)0.75 = 0, node_2 leaves node_1 with (size_t)5.5 = 5, node_1 keeps c, d
    # and stays.  node_2 = (node_1:5), node_3 = (b, node_2:0), node_4 = (a, node_3:2).  Column 0: a 2, b 2, c 4,
    # d 16.  node_1 = 20, node_2 = 20 (one child), node_3 = 2 | 20 = 22.  Down: node_3 holds 2; node_2 does not,
    # lowest bit 4; node_1 and c take 4; d 16.  node_2: NS C, d: NS G.
    "D_unary_node_on_the_chain": (
        _case("(((a:2.5,b:1.25):0.75):5.5,c:1,d:2);", [[0, "A"]], {"node_1": [[0, 1, 0]]},
              {"c": [[0, 0, -1, 3, [2]]], "d": [[0, 0, -1, 3, [4]]]}), "a",
        _dump("(a:0.000000,(b:1.250000,((c:1.000000,d:2.000000)node_1:5.000000)node_2:0.000000)node_3:2.000000)node_4:0.000000;",
              "d N 0 0 -1 16 400000",
              "node_2 N 0 0 -1 16 200000",
              "node_4 B 0 1 0")),
    # node_1 = root (node_2, b, c), node_2 = (a) unary.  a leaves node_2, which has no child left, with
    # (size_t)2.5 = 2; node_2 leaves node_1 with (size_t)3.5 = 3 and takes it as its only child.  Column 0: a 2,
    # b 4, c 2: node_1 = 6 = node_2; both hold 2 and take it; b 4: NS C.
    "E_unary_parent_of_the_leaf": (
        _case("((a:2.5):3.5,b:1.75,c:1);", [[0, "A"]], {"node_1": [[0, 1, 0]]}, {"b": [[0, 0, -1, 3, [2]]]}), "a",
        _dump("(a:0.000000,((b:1.750000,c:1.000000)node_1:3.000000)node_2:2.000000)node_3:0.000000;",
              "b N 0 0 -1 16 200000",
              "node_3 B 0 1 0")),
    # New tree node_3 = (a, node_2 = (b, c)); consensus ACGTA, one gap slot before position 0, three before 2.
    #   a = A G - T C, sentinel T, slots (2,0) A, (2,1) G;  b = A C G C C, sentinel T, slots (2,1) G, (2,2) C;
    #   c = A C G G C, slot (2,1) G.
    # Main positions, parent state of node_3 = the consensus:
    #   1 (C 4): a 16, b = c = 4.  node_3 is forced to 16 -- free, it would take 4 and a would mutate.  node_3
    #     NS G, node_2 (4, does not hold 16) NS C.
    #   2 (G 16): only a lacks it.  node_3 forced to 1: ND; node_2 16 under a parent 1: NI G.
    #   3 (T 256): a 256, b 4, c 16.  node_2 = 4 | 16 does not hold 256: the lowest bit, 4, breaks the tie.
    #     node_2 NS C, b takes 4, c NS G.
    #   4 (A 2): every tip C: node_3 is 4, its parent state 2: the consensus alone makes NS C.
    #   5 (sentinel, parent state 1 << code('-') = 1): a 256, b 256, c 1 ('x').  node_3 256 under 1: NI T, not a
    #     substitution.  node_2 = 257 holds 256; c does not: 1, ND.
    # Gap slots, parent state 1:  (0,0) nobody: nothing.  (2,0) only a: node_3 2: NI A; node_2 1: ND.
    #   (2,1) every tip G: node_3 NI G.  (2,2) only b: node_2 = 4 | 1 holds node_3's 1; b 4: NI C.
    # node_3's main tuples at 1 NS, 2 ND, 4 NS, 5 NI never join (type, type, position, type); its gap tuples
    # (2,0) and (2,1) are one NI run of 2: info (2 << 4) + 2, codes 1, 4.  node_2's 1 NS, 2 NI, 3 NS stay apart.
    "F_one_block_three_tips": (
        _case("((a:1,b:1):1,c:1);", [[0, "ACGTA"]], {"node_1": [[0, 1, 0]]},
              {"a": [[0, 1, -1, 3, [4]], [0, 2, -1, 5, [0]], [0, 4, -1, 3, [2]], [0, 5, -1, 4, [8]], [0, 2, 0, 4, [1]],
                     [0, 2, 1, 4, [4]]],
               "b": [[0, 3, -1, 3, [2]], [0, 4, -1, 3, [2]], [0, 5, -1, 4, [8]], [0, 2, 1, 4, [4]], [0, 2, 2, 4, [2]]],
               "c": [[0, 3, -1, 3, [4]], [0, 4, -1, 3, [2]], [0, 2, 1, 4, [4]]]},
              gaps=[[0, [[0, 1], [2, 3]]]]), "a",
        _dump("(a:0.000000,(b:1.000000,c:1.000000)node_2:1.000000)node_3:0.000000;",
              "b N 0 2 2 18 200000",
              "c N 0 3 -1 16 400000",
              "c N 0 5 -1 17 000000",
              "node_2 N 0 1 -1 16 200000",
              "node_2 N 0 2 -1 18 400000",
              "node_2 N 0 3 -1 16 200000",
              "node_2 N 0 2 0 17 000000",
              "node_3 B 0 1 0",
              "node_3 N 0 1 -1 16 400000",
              "node_3 N 0 2 -1 17 000000",
              "node_3 N 0 4 -1 16 200000",
              "node_3 N 0 5 -1 18 800000",
              "node_3 N 0 2 0 34 140000")),
    # New tree node_3 = (a, node_2 = (b, c)).  The old root inserts blocks 0 and 1 forward and block 2
    # reversed, a deletes block 0, b turns block 2 (forward again), c deletes block 1.
    #   block 0: a 1, b 2, c 2.  node_3 forced to 1 = its parent state; node_2 2 under 1: BI, state 2: forward.
    #   block 1: a 2, b 2, c 1.  node_3 2: BI forward; node_2 = 3 holds 2; c 1 under 2: BD.
    #   block 2: a 4, b 2, c 4.  node_3 4 under 1: BI, state 4: inverted; node_2 = 6 holds 4; b 2 under 4,
    #     neither is 1: BD with the inversion flag.
    # c's substitution in block 1 is skipped, c lacks the block (getSequenceFromReference): c has its consensus
    # there.  b's T at base 0 of block 2 (consensus G): a 16, b 256, c 16; node_2 holds 16; b NS T.
    "G_block_states": (
        _case("((a:1,b:1):1,c:1);", [[0, "AC"], [1, "TT"], [2, "GG"]],
              {"node_1": [[0, 1, 0], [1, 1, 0], [2, 1, 1]], "a": [[0, 0, 0]], "b": [[2, 0, 1]], "c": [[1, 0, 0]]},
              {"c": [[1, 0, -1, 3, [1]]], "b": [[2, 0, -1, 3, [8]]]}), "a",
        _dump("(a:0.000000,(b:1.000000,c:1.000000)node_2:1.000000)node_3:0.000000;",
              "b B 2 0 1",
              "b N 2 0 -1 16 800000",
              "c B 1 0 0",
              "node_2 B 0 1 0",
              "node_3 B 1 1 0",
              "node_3 B 2 1 1")),
}


# ---- builders ---------------------------------------------------------------------------------------------

class Case(NamedTuple):
    pm: PanMAT
    leaf: str
    check: Callable[[str], None]       # asserts the builder's property on a dump of this case
    columns: int | None = None         # the promised count of canonical columns


class Block(NamedTuple):
    id: int
    cons: str
    slots: dict      # position (0 .. len(cons), the last one the sentinel's) -> gap slots before it


class Held(NamedTuple):
    """How a tip holds a block: strand '+' / '-' (None: not at all), its characters that differ from the
    consensus ({position: char}, '-' deletes) and its filled gap slots ({(position, slot): char})."""
    strand: str | None = "+"
    main: dict = {}
    gap: dict = {}


def tips_panmat(newick: str, blocks: list[Block], tips: dict, root_inserts=None) -> PanMAT:
    """The PanMAT over `newick` (with branch lengths) whose root inserts the blocks of `root_inserts` (default:
    all) forward and whose tips `tips[name][block id]` (default Held()) differ from that by their own
    mutations: one record per character."""
    names, off, idx, root = parse_newick(newick)
    pm = PanMAT(names, off, idx, root)
    pm.branch_length = newick_lengths(newick)
    assert len(pm.branch_length) == len(names)
    at_root = {b.id for b in blocks} if root_inserts is None else set(root_inserts)
    for b in blocks:
        pm.add_block(b.id, b.cons)
        if b.slots:
            pm.add_gaps(b.id, sorted(b.slots.items()))
        if b.id in at_root:
            pm.add_block_mut(root, b.id, True, False)
    for v in pm.leaves():
        for b in blocks:
            h = tips.get(names[v], {}).get(b.id, Held())
            if h.strand is None:
                if b.id in at_root:
                    pm.add_block_mut(v, b.id, False, False)
                continue
            if b.id not in at_root:
                pm.add_block_mut(v, b.id, True, h.strand == "-")
            elif h.strand == "-":
                pm.add_block_mut(v, b.id, False, True)
            for pos, ch in sorted(h.main.items()):
                assert 0 <= pos < len(b.cons) and ch != b.cons[pos]
                pm.add_nuc_mut(v, b.id, pos, -1, 5 if ch == "-" else 3, [CODE[ch]])
            for (pos, slot), ch in sorted(h.gap.items()):
                assert slot < b.slots[pos] and ch != "-"
                pm.add_nuc_mut(v, b.id, pos, slot, 4, [CODE[ch]])
    return pm


def columns_of(blocks: list[Block]) -> dict:
    """(block id, position, slot or -1) -> canonical column: the blocks in id order, before every position
    (the sentinel's included) its gap slots."""
    col, at = {}, 0
    for b in sorted(blocks, key=lambda b: b.id):
        for pos in range(len(b.cons) + 1):
            for w in range(b.slots.get(pos, 0)):
                col[(b.id, pos, w)] = at
                at += 1
            col[(b.id, pos, -1)] = at
            at += 1
    return col


def n_lines(dump: str, node: str):
    """The N lines of `node` in list order: (block, position, slot, length, type)."""
    out = []
    for line in dump.splitlines()[1:]:
        f = line.split("\t")
        if f[0] == node and f[1] == "N":
            out.append((int(f[2]), int(f[3]), int(f[4]), int(f[5]) >> 4, int(f[5]) & 15))
    return out


def b_lines(dump: str):
    return {tuple(line.split("\t")[3:5]) for line in dump.splitlines()[1:] if line.split("\t")[1] == "B"}


def _no_check(dump):
    assert not dump.startswith("#error"), dump


# -- topology

_T0 = Block(0, "ACGTACGTAC", {3: 2})
_T1 = Block(1, "TTGCA", {})


def _random_tips(names, blocks, seed, states=True):
    """A few substitutions, deletions and filled slots per tip; block 1, if any, absent or reversed in some."""
    rng = np.random.default_rng(seed)
    tips = {}
    for n in names:
        held = {}
        for b in blocks:
            strand = "+"
            if states and b.id:
                strand = [None, "-", "+", "+", "+", "+"][int(rng.integers(6))]
            main = {}
            for pos in np.flatnonzero(rng.random(len(b.cons)) < 0.15):
                main[int(pos)] = str(rng.choice([c for c in "ACGT-" if c != b.cons[pos]]))
            gap = {(p, w): str(rng.choice(list("ACGT"))) for p, k in b.slots.items() for w in range(k) if rng.random() < 0.25}
            held[b.id] = Held(strand, main, gap)
        tips[n] = held
    return tips


def _moved_lengths_check(pm: PanMAT, leaf: str):
    """The tip's old length has a fraction and arrives at its old parent without it (when the parent is the
    root nothing moves, and the tip's length becomes 0)."""
    v = pm.index(leaf)
    parent = {int(c): p for p in range(pm.num_nodes) for c in pm.child_index[pm.child_offsets[p]:pm.child_offsets[p + 1]]}
    par, old = parent[v], float(pm.branch_length[v])

    def check(dump):
        from _panmat import _parse_labelled
        assert not dump.startswith("#error"), dump
        text = dump.splitlines()[0][7:]
        names, _, _ = _parse_labelled(text)
        lens = dict(zip(names, newick_lengths(text).tolist()))
        assert lens[leaf] == 0
        if par != pm.root:
            assert old != int(old) and lens[pm.names[par]] == int(old), (old, lens[pm.names[par]])
        else:
            assert any(float(x) != int(x) for x in pm.branch_length)
    return check


def caterpillar_newick(depth: int) -> str:
    """(t0,(t1,(... (t<depth-1>,t<depth>)))): `depth` internal nodes, fractional lengths everywhere."""
    def tip(k):
        return f"t{k}:{k % 5 + 1.375}"
    s = f"({tip(depth - 1)},{tip(depth)})"
    for k in range(depth - 2, -1, -1):
        s = f"({tip(k)},{s}:{k % 3 + 0.625})"
    return s + ";"


def caterpillar(depth: int, deepest: bool) -> Case:
    """A caterpillar of `depth` internal nodes rerooted at its deepest tip or at the tip next to the root;
    19 columns (depth 300: at most 40)."""
    text = caterpillar_newick(depth)
    names = [f"t{k}" for k in range(depth + 1)]
    pm = tips_panmat(text, [_T0, _T1], _random_tips(names, [_T0, _T1], 1000 + depth))
    leaf = names[depth] if deepest else "t0"
    return Case(pm, leaf, _moved_lengths_check(pm, leaf), 19)


# twelve tips; out-degrees 1 (t5's parent, and the node above (t8,t9,t10), which lies on their chain), 2, 3
# (the root) and 4
MIXED_NEWICK = ("((t0:1.5,t1:2.25,(t2:0.5,t3:1.75):2.5,t4:3.125):1.25,"
                "((t5:2.75):1.5,t6:0.25,(t7:4.5,((t8:1.125,t9:2.875,t10:0.625):3.75):6.5):0.875):2.375,t11:5.5):0.5;")
MIXED_TIPS = [f"t{k}" for k in range(12)]


def mixed_pm() -> PanMAT:
    return tips_panmat(MIXED_NEWICK, [_T0, _T1], _random_tips(MIXED_TIPS, [_T0, _T1], 77))


def mixed(tip: int) -> Case:
    pm = mixed_pm()
    return Case(pm, f"t{tip}", _moved_lengths_check(pm, f"t{tip}"), 19)


def polytomy(n: int) -> Case:
    """`n` tips under one node below a root of degree 3, rerooted at one of them."""
    names = [f"p{k}" for k in range(n)]
    text = "((" + ",".join(f"{p}:{k % 4 + 0.75}" for k, p in enumerate(names)) + "):2.5,q0:1.25,q1:3.5);"
    pm = tips_panmat(text, [_T0, _T1], _random_tips(names + ["q0", "q1"], [_T0, _T1], 2000 + n))
    leaf = names[n // 2]
    return Case(pm, leaf, _moved_lengths_check(pm, leaf), 19)


def unary_root() -> tuple[PanMAT, str]:
    """transformHelper reads children[0] of an empty list (src/panman.cpp:5837): both sides refuse."""
    return tips_panmat("((a:1.5,b:2.5):1.25);", [Block(0, "TTGCA", {})], {"b": {0: Held("+", {0: "A"})}}), "a"


# -- blocks

# (a, b, c, d) per block: None absent, '+' forward, '-' reversed; a is the new root
_PATTERNS = [
    ("-", "+", "+", "+"),        # the new root alone reversed
    ("+", "-", "-", "-"),        # the converse
    (None, None, None, None),    # nobody holds it
    ("+", None, None, None),     # only the new root holds it
    (None, "+", "-", "+"),       # the new root lacks it
    ("+", "+", None, "-"),
    ("-", None, "-", "+"),
]
BLOCK_COUNTS = (1, 2, 3, 16, 17)


def block_states(count: int, ids=None) -> Case:
    """((a,b),(c,d)) rerooted at a, `count` blocks of three bases whose states cycle through _PATTERNS
    (bcodes packs two per byte: an odd count leaves half a byte); b changes a base of every block it holds."""
    ids = list(range(count)) if ids is None else list(ids)
    blocks = [Block(i, "ACG", {}) for i in ids]
    tips = {n: {} for n in "abcd"}
    for k, b in enumerate(blocks):
        for n, strand in zip("abcd", _PATTERNS[(k + count) % len(_PATTERNS)]):
            tips[n][b.id] = Held(strand, {k % 3: "T"} if n == "b" and strand else {})
    # the root inserts the blocks at least two tips hold
    at_root = [b.id for b in blocks if sum(tips[n][b.id].strand is not None for n in "abcd") >= 2]
    pm = tips_panmat("((a:1.5,b:2.25):3.75,(c:0.5,d:1.25):2.5);", blocks, tips, at_root)

    def check(dump):
        assert not dump.startswith("#error"), dump
        if count >= len(_PATTERNS):   # BI, BI inverted, BD, BD with the inversion flag
            assert b_lines(dump) == {("1", "0"), ("1", "1"), ("0", "0"), ("0", "1")}
    return Case(pm, "a", check, 4 * count)


def block_ids_0_2() -> tuple[PanMAT, str]:
    """No block has id 1: "Block with id 1 -1 not found!" (src/reroot.cpp:160-163)."""
    return block_states(2, ids=(0, 2)).pm, "a"


# -- columns

COLUMN_COUNTS = (2, 3, 31, 32, 33, 511, 512, 513)
_TREES = {3: ("((a:1.5,b:0.75):2.25,c:1);", "abc"), 5: ("((a:1.5,b:0.75):2.25,(c:1,(d:3.5,e:0.125):1.5):2);", "abcde")}


def columns(total: int, tips: int) -> Case:
    """One block of `total` canonical columns (k_rows_to_codes: one thread per two columns and row, 256 per
    workgroup; an odd count leaves half a byte), from 31 up four of them gap slots: one before base 0, two
    before base 1, one before the sentinel."""
    slots = {0: 1, 1: 2, total - 5: 1} if total >= 31 else {}
    length = total - 1 - sum(slots.values())
    rng = np.random.default_rng(total)
    b = Block(0, "".join(rng.choice(list("ACGT"), size=length)), slots)
    text, names = _TREES[tips]
    pm = tips_panmat(text, [b], _random_tips(list(names), [b], 3000 + total + tips))
    assert len(columns_of([b])) == total
    return Case(pm, "a", _no_check, total)


_IUPAC = "ACMGRSVTWYHKDBN"


def iupac() -> Case:
    """All 15 codes in the consensus, in every tip and so in the new root: tip k holds the consensus rotated
    by k + 1, so no column agrees with the consensus or between two tips; block 1 has them agree."""
    blocks = [Block(0, _IUPAC, {}), Block(1, _IUPAC[::-1], {})]
    tips = {n: {0: Held("+", {p: _IUPAC[(p + k + 1) % 15] for p in range(15)})} for k, n in enumerate("abc")}
    pm = tips_panmat(_TREES[3][0], blocks, tips)

    def check(dump):
        assert not dump.startswith("#error"), dump
        codes = set("".join(f[6] for f in (line.split("\t") for line in dump.splitlines()[1:]) if f[1] == "N"))
        assert codes >= set("123456789abcdef")
    return Case(pm, "a", check, 32)


def gap_slots() -> Case:
    """Slots before base 0, base 2, base 3 and the sentinel of ACGT.  (0,0) and (4,0): every tip fills them;
    (2,0): only the new root a; (2,1): nobody; (3,0): only b; (4,1): a and c with different bases."""
    b = Block(0, "ACGT", {0: 1, 2: 2, 3: 1, 4: 2})
    tips = {"a": {0: Held("+", {}, {(0, 0): "G", (4, 0): "T", (2, 0): "C", (4, 1): "A"})},
            "b": {0: Held("+", {}, {(0, 0): "G", (4, 0): "T", (3, 0): "A"})},
            "c": {0: Held("+", {}, {(0, 0): "G", (4, 0): "T", (4, 1): "G"})}}
    pm = tips_panmat(_TREES[3][0], [b], tips)

    def check(dump):
        # a gap slot's root parent state is a gap: what every tip fills is an insertion at the new root node_3
        # (a main column every tip agrees on with the consensus is none); (2,0) is deleted again below it
        assert n_lines(dump, "node_3") == [(0, 0, 0, 1, 2), (0, 2, 0, 1, 2), (0, 4, 0, 2, 2)]
        assert n_lines(dump, "node_2") == [(0, 2, 0, 1, 1), (0, 4, 1, 1, 1)]
        assert n_lines(dump, "b") == [(0, 3, 0, 1, 2)] and n_lines(dump, "c") == [(0, 4, 1, 1, 2)]
    return Case(pm, "a", check, 11)


# -- runs and chunks

def _next(ch):
    return "ACGT"[("ACGT".index(ch) + 1) % 4]


_R0 = Block(0, "ACGT" * 19, {})                        # 76 bases: columns 0 .. 76
_R1 = Block(1, "TGCA" * 22 + "TG", {})                 # 90 bases: columns 77 .. 167
_R2 = Block(2, "GATTACAGATTA", {4: 7, 8: 6, 9: 2, 10: 2})   # 12 bases, 17 slots: columns 168 .. 197
RUN_BLOCKS = [_R0, _R1, _R2]
RUN_COLUMNS = 198
# b's substituted bases of block 0: runs of 5, 6, 7, 12 and 13; the last one lies in columns 60 .. 72 and its first
# record in 60 .. 65, across the chunk edges 63 (chunks of 7) and 64 (chunks of 64)
_B_RUNS = [(2, 5), (9, 6), (17, 7), (26, 12), (60, 13)]
CHUNK_SIZES = (1, 2, 7, 64, RUN_COLUMNS - 1, RUN_COLUMNS, RUN_COLUMNS + 1)


def runs() -> Case:
    """((a,b),c) rerooted at a; a keeps the consensus, so what b or c alone changes is a mutation of that tip.
      b, block 0: substituted runs of 5, 6, 7, 12 and 13 bases -> records of [5, 6, 6, 1, 6, 6, 6, 6, 1].
      c, blocks 0 / 1: the last two bases of block 0 and the first two of block 1 substituted: cut, not joined.
      c, block 1: bases 3 .. 5 substituted, 6 .. 8 deleted: the type changes in the middle.
      c, block 2: the last base (column 196 of 198) substituted: a record in the last chunk of sizes 2 and 7.
      b, block 2: bases 2 .. 6 substituted, passing base 4 and its 7 slots: one record of 5 (the main tuples are
        grouped on their own); all 7 slots of base 4 filled: [6, 1]; all 6 of base 8: [6]; the last slot of base
        9 and the first of base 10: two records; and so b has both kinds, main records first."""
    def sub(blk, ps):
        return {p: _next(blk.cons[p]) for p in ps}
    b0 = [p for start, n in _B_RUNS for p in range(start, start + n)]
    b_gap = {(4, w): "ACGTACG"[w] for w in range(7)}
    b_gap.update({(8, w): "TGCATG"[w] for w in range(6)})
    b_gap.update({(9, 1): "C", (10, 0): "A"})
    c1 = sub(_R1, [0, 1, 3, 4, 5])
    c1.update({6: "-", 7: "-", 8: "-"})
    tips = {"b": {0: Held("+", sub(_R0, b0)), 2: Held("+", sub(_R2, range(2, 7)), b_gap)},
            "c": {0: Held("+", sub(_R0, [74, 75])), 1: Held("+", c1), 2: Held("+", sub(_R2, [11]))}}
    pm = tips_panmat(_TREES[3][0], RUN_BLOCKS, tips)
    assert len(columns_of(RUN_BLOCKS)) == RUN_COLUMNS

    def check(dump):
        b, c = n_lines(dump, "b"), n_lines(dump, "c")
        assert [r[3] for r in b if r[0] == 0] == [5, 6, 6, 1, 6, 6, 6, 6, 1]
        assert all(r[4] == 0 for r in b if r[2] == -1)
        assert c == [(0, 74, -1, 2, 0), (1, 0, -1, 2, 0), (1, 3, -1, 3, 0), (1, 6, -1, 3, 1), (2, 11, -1, 1, 0)]
        assert [r for r in b if r[0] == 2] == [(2, 2, -1, 5, 0), (2, 4, 0, 6, 2), (2, 4, 6, 1, 2), (2, 8, 0, 6, 2),
                                              (2, 9, 1, 1, 2), (2, 10, 0, 1, 2)]
        kinds = [r[2] != -1 for r in b]
        assert kinds == sorted(kinds) and kinds[0] is False and kinds[-1] is True
        col = columns_of(RUN_BLOCKS)
        for size in (7, 64):   # a record whose bases lie in two chunks
            assert any(col[(blk, pos, -1)] // size != col[(blk, pos + n - 1, -1)] // size
                       for blk, pos, slot, n, _ in b + c if slot == -1), size
        assert RUN_COLUMNS % 7 != 0   # chunks of 7: the last one is shorter
    return Case(pm, "a", check, RUN_COLUMNS)


EDGE: dict[str, Callable[[], Case]] = {}
for _d in (1, 2, 3, 64, 65, 300):
    EDGE[f"caterpillar_{_d}_deepest"] = (lambda d=_d: caterpillar(d, True))
    EDGE[f"caterpillar_{_d}_next_to_root"] = (lambda d=_d: caterpillar(d, False))
for _k in range(12):
    EDGE[f"mixed_degrees_t{_k}"] = (lambda k=_k: mixed(k))
for _n in (65, 257):
    EDGE[f"polytomy_{_n}"] = (lambda n=_n: polytomy(n))
for _n in BLOCK_COUNTS:
    EDGE[f"blocks_{_n}"] = (lambda n=_n: block_states(n))
for _t in (3, 5):
    for _c in COLUMN_COUNTS:
        EDGE[f"columns_{_c}_tips_{_t}"] = (lambda c=_c, t=_t: columns(c, t))
EDGE["iupac"] = iupac
EDGE["gap_slots"] = gap_slots
EDGE["runs"] = runs
