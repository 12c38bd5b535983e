"""A plain-Python restatement of Tree::extractAminoAcidTranslations (src/aaTrans.cpp:185-304),
of getNucleotideSequenceFromBlockCoordinates / getAminoAcidSequence (aaTrans.cpp:3-183) and of
globalCoordinateToBlockCoordinate with circular offset 0 (src/panman.cpp:5726-5798), working
from a list-built PanMAT alone.

Every node's sequence comes from its own path walk (`_maf_ref.block_state`, `block_sequence`),
with rotation, sequence inversion and circular offset playing no part (rotate = false).  The
deviations pm_aa documents: lines are in node-id order (the reference iterates a
tbb::concurrent_unordered_map); a root window that ends "ERROR" raises (the reference goes on
and reports every codon as an insertion at 0); a reverse-strand block inside the window whose
walk the reference starts out of range (it reads block id 0's length) raises Unsupported."""
from __future__ import annotations

from _maf_ref import _Lists, _parents, _path, block_sequence, block_state

# the standard genetic code: the 64 codons in TCAG order, one letter each, and the names
_ORDER = "TCAG"
_LETTERS = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
_NAMES = {"A": "Ala", "R": "Arg", "N": "Asn", "D": "Asp", "C": "Cys", "Q": "Gln", "E": "Glu", "G": "Gly", "H": "His",
          "I": "Ile", "L": "Leu", "K": "Lys", "M": "Met", "F": "Phe", "P": "Pro", "S": "Ser", "T": "Thr", "W": "Trp",
          "Y": "Tyr", "V": "Val", "*": "*"}
CODON_TABLE = {a + b + c: _NAMES[_LETTERS[16 * i + 4 * j + k]]
               for i, a in enumerate(_ORDER) for j, b in enumerate(_ORDER) for k, c in enumerate(_ORDER)}


class ArgError(ValueError):
    """PM_ERR_ARG: end <= start, the root not located, the root's window 'ERROR'."""


class Unsupported(ValueError):
    """PM_ERR_UNSUPPORTED: secondary blocks; a reverse walk the reference starts out of range."""


class NodeState:
    """One node's sequence_t, blockExists and blockStrand over ids 0..max_id."""

    def __init__(self, pm, path, max_id, is_block):
        self.seq = [[] for _ in range(max_id + 1)]       # ids that hold no block: no position
        self.held = [False] * (max_id + 1)
        self.forward = [True] * (max_id + 1)
        for b in is_block:
            self.seq[b] = block_sequence(pm, path, b)
            ex, st = block_state(pm, path, b)
            self.held[b] = ex
            self.forward[b] = st if ex else True          # an absent block counts as forward


def locate(s: NodeState, g: int):
    """globalCoordinateToBlockCoordinate(g, circularOffset = 0): (block, position, slot) with
    slot -1 for a main character, or None."""
    def real(ch):
        return ch != "-" and ch != "x"

    length = 0
    for b, seq in enumerate(s.seq):
        if s.held[b]:
            for main, slots in seq:
                length += sum(real(ch) for ch in slots) + real(main)
    if not g < length:
        g -= length
    ctr = 0
    for b, seq in enumerate(s.seq):
        if not s.held[b]:
            continue
        if s.forward[b]:
            for j, (main, slots) in enumerate(seq):
                for k, ch in enumerate(slots):
                    if real(ch):
                        if ctr == g:
                            return (b, j, k)
                        ctr += 1
                if real(main):
                    if ctr == g:
                        return (b, j, -1)
                    ctr += 1
        else:
            for j in range(len(seq) - 1, -1, -1):
                main, slots = seq[j]
                if real(main):
                    if ctr == g:
                        return (b, j, -1)
                    ctr += 1
                for k in range(len(slots) - 1, -1, -1):
                    if real(slots[k]):
                        if ctr == g:
                            return (b, j, k)
                        ctr += 1
    return None


def window(s: NodeState, start, end):
    """getNucleotideSequenceFromBlockCoordinates: the characters from `start` up to `end`
    (exclusive), or None for "ERROR"."""
    b0, j0, k0 = start
    out = []
    for i in range(b0, end[0] + 1):
        seq = s.seq[i]
        if s.forward[i]:
            for j in range(j0 if i == b0 else 0, len(seq)):
                main, slots = seq[j]
                # the slot loop always starts at get<3>(start): no slot at all when it is -1
                if k0 != -1:
                    for k in range(k0, len(slots)):
                        if (i, j, k) == end:
                            return "".join(out)
                        out.append(slots[k] if s.held[i] else "-")
                if (i, j, -1) == end:
                    return "".join(out)
                out.append(main if s.held[i] else "-")
        else:
            if i == b0:
                top = j0
            else:
                top = len(s.seq[0]) - 1                   # the reference reads sequence[0]
                if top < 0 or top >= len(seq):
                    raise Unsupported("reverse-strand walk starts outside its block")
            for j in range(top, -1, -1):
                main, slots = seq[j]
                if (i, j, -1) == end:
                    return "".join(out)
                out.append(main if s.held[i] else "-")
                first = k0 if (i == b0 and j == j0) else len(slots) - 1
                for k in range(first, -1, -1):
                    if (i, j, k) == end:
                        return "".join(out)
                    out.append(slots[k] if s.held[i] else "-")
    return None


def codons(w):
    """getAminoAcidSequence: (amino acids, starts, ends) of a window; an "ERROR" window has none."""
    if w is None:
        return [], [], []
    w = "".join(ch if ch in "ACGT" else "-" for ch in w)
    aas, starts, ends = [], [], []
    cur = ""
    for i, ch in enumerate(w):
        if ch != "-":
            if not cur:
                starts.append(i)
            cur += ch
        if len(cur) == 3:
            ends.append(i)
            aas.append(CODON_TABLE[cur])
            cur = ""
    while len(starts) > len(ends):
        starts.pop()
    return aas, starts, ends


def merge(ref_starts, ref_ends, alt_starts):
    """The two-pointer loop of aaTrans.cpp:259-285: (matches, insertions, deletions) as
    (ref index, alt index) pairs, (ref index, alt index) pairs and ref indices."""
    matches, insertions, deletions = [], [], []
    ref_itr = alt_itr = 0
    while alt_itr < len(alt_starts) and ref_itr < len(ref_starts):
        if alt_starts[alt_itr] > ref_ends[ref_itr]:
            deletions.append(ref_itr)
            ref_itr += 1
        elif alt_starts[alt_itr] < ref_starts[ref_itr]:
            insertions.append((ref_itr, alt_itr))
            alt_itr += 1
        else:
            matches.append((ref_itr, alt_itr))
            alt_itr += 1
            ref_itr += 1
    while alt_itr < len(alt_starts):
        insertions.append((ref_itr, alt_itr))
        alt_itr += 1
    while ref_itr < len(ref_starts):
        deletions.append(ref_itr)
        ref_itr += 1
    return matches, insertions, deletions


def merge_order_free(ref_starts, ref_ends, alt_starts):
    """The same three lists without a carried pointer (the form the kernels use): q(a) = the
    root codons that end before a starts; a matches q(a) iff it starts at or after that codon's
    start and is the first of the node's codons with that q to do so."""
    from bisect import bisect_left
    n = len(ref_starts)
    matches, insertions = [], []
    matched = [False] * n
    prev_in = False   # the previous codon had the same q and lay inside the interval
    prev_q = -1
    for a, st in enumerate(alt_starts):
        q = bisect_left(ref_ends, st)
        inside = q < n and st >= ref_starts[q]
        if inside and not (prev_q == q and prev_in):
            matches.append((q, a))
            matched[q] = True
        else:
            insertions.append((q + 1 if inside else q, a))
        prev_q, prev_in = q, inside
    return matches, insertions, [q for q in range(n) if not matched[q]]


def node_string(ref, alt) -> str:
    ref_aa, ref_starts, ref_ends = ref
    alt_aa, alt_starts, _ = alt
    matches, insertions, deletions = merge(ref_starts, ref_ends, alt_starts)
    out = [f"S:{q}:{alt_aa[a]};" for q, a in matches if ref_aa[q] != alt_aa[a]]
    out += [f"I:{q}:{alt_aa[a]};" for q, a in insertions]
    out += [f"D:{q};" for q in deletions]
    return "".join(out)


def aa(pm, start: int, end: int):
    """(text, ref_codons, unlocated)."""
    if getattr(pm, "_arrays", None) is not None:
        pm = _Lists(pm)
    if end <= start:
        raise ArgError("End coordinate must be greater than start")
    if any(secondary != -1 for muts in pm.nuc_muts for _, secondary, *_ in muts):
        raise Unsupported("secondary blocks")
    parent = _parents(pm)
    max_id = max(b for b, _ in pm.blocks)
    is_block = {b for b, _ in pm.blocks}

    def state(v):
        return NodeState(pm, _path(pm, parent, v), max_id, is_block)

    root = state(pm.root)
    s, e = locate(root, start), locate(root, end)
    if s is None or e is None:
        raise ArgError("coordinates out of range")
    w = window(root, s, e)
    if w is None:
        raise ArgError("root window")
    ref = codons(w)
    if not ref[0]:
        return "", 0, 0
    unlocated = 0
    lines = ["node_id\taa_mutations\n"]
    for v in range(pm.num_nodes):
        st = root if v == pm.root else state(v)
        s, e = locate(st, start), locate(st, end)
        if s is None or e is None:
            unlocated += 1
            continue
        string = node_string(ref, codons(window(st, s, e)))
        if string:
            lines.append(f"{pm.names[v]}\t{string}\n")
    return "".join(lines), len(ref[0]), unlocated
