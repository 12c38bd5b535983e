"""A plain-Python restatement of Tree::printMutationsNew(std::ostream&) (src/panman.cpp:3699-4057;
the --printMutations command without --input-file, src/panmanUtils.cpp:1008-1071), working from a
list-built PanMAT alone.

Every node's sequence comes from its own path walk as getSequenceFromReference(rotate = false)
builds it (src/panman.cpp:4676-4972): all block mutations of the path first, then the nucleotide
mutations of the blocks the node holds at the end only, so a block it does not hold keeps its
consensus and its empty gap slots (`_maf_ref.block_sequence` over an empty path).  The reference's
maps keyed by (block, position, slot) are dictionaries here; its seqChar map, which has an entry for
every cell of every node, is the function `seq_char` of one cell.

The deviations pm_print_mutations documents: nodes are printed in node-id order (the reference
iterates a tbb::concurrent_unordered_map); the stdout notices are not printed, the kept NSNPS
entries over a '-' are counted instead; a secondary block, a block that some node does not hold yet
flags reverse, and a mutation on an id that holds no block raise Unsupported; a mutation element
(of types 0 to 5) whose cell does not exist raises ArgError, where the reference would
default-insert into its maps."""
from __future__ import annotations

from _maf_ref import NUC, _Lists, _parents, _path, block_sequence, block_state


class ArgError(ValueError):
    """PM_ERR_ARG: a mutation whose cell does not exist."""


class Unsupported(ValueError):
    """PM_ERR_UNSUPPORTED: secondary blocks; a block not held but flagged reverse."""


def real(ch):
    return ch != "-" and ch != "x"


class NodeState:
    """One node's sequence_t, blockExists and blockStrand over ids 0..max_id."""

    def __init__(self, pm, path, max_id, is_block):
        self.seq = [[] for _ in range(max_id + 1)]       # ids that hold no block: no position
        self.held = [False] * (max_id + 1)
        self.forward = [True] * (max_id + 1)
        for b in is_block:
            ex, st = block_state(pm, path, b)
            self.held[b], self.forward[b] = ex, st
            self.seq[b] = block_sequence(pm, path if ex else [], b)   # :4827-4835


def root_map(root: NodeState):
    """:3725-3806: (coord, gap) of every cell (block, position, slot), slot -1 the main character."""
    coord, gap = {}, {}
    ctr = 0
    for i, seq in enumerate(root.seq):
        def visit(j, k, ch):
            nonlocal ctr
            coord[i, j, k] = ctr
            if not root.held[i]:
                gap[i, j, k] = False
            elif real(ch):
                gap[i, j, k] = False
                ctr += 1
            else:
                gap[i, j, k] = True

        if root.forward[i]:
            for j, (main, slots) in enumerate(seq):
                for k, ch in enumerate(slots):
                    visit(j, k, ch)
                visit(j, -1, main)
        else:
            for j in range(len(seq) - 1, -1, -1):
                main, slots = seq[j]
                visit(j, -1, main)
                for k in range(len(slots) - 1, -1, -1):
                    visit(j, k, slots[k])
    return coord, gap


def seq_char(s: NodeState, root: NodeState, i, j, k):
    """seqChar[(u, i, j, k)] (:3810-3849)."""
    main, slots = s.seq[i][j]
    if k != -1:
        return slots[k] if real(slots[k]) else "-"
    if s.forward[i]:
        return main if real(main) and s.held[i] else "-"
    return root.seq[i][j][0] if real(main) else "-"      # :3835, the root's stored character


def node_entries(pm, v, path, parent_state, root, coord, gap):
    """:3859-4022: the entries (kind, coord, old, new, gap) of node v != root, and the kept NSNPS
    entries whose old character is no base."""
    present = list(root.held)
    for node in path[1:]:
        for b, insertion, inversion in pm.block_muts[node]:
            if b >= len(present):
                continue
            if insertion:
                present[b] = True
            elif not inversion:
                present[b] = False
    out, odd = [], 0
    for b, _, pos, g, info, nucs in pm.nuc_muts[v]:
        typ, length = info & 7, info >> 4

        def cell(j):
            return (b, pos, g + j) if g != -1 else (b, pos + j, -1)

        def code(j):
            return NUC[(nucs >> (4 * (5 - j))) & 15]

        def old(j):
            return seq_char(parent_state, root, *cell(j))

        if typ == 0:
            for j in range(length):
                if present[b]:
                    o = old(j)
                    if o == "-" or o == "x":
                        continue
                    out.append(("S", coord[cell(j)], o, code(j), gap[cell(j)]))
        elif typ == 2:
            for j in range(length):
                out.append(("I", coord[cell(j)], "-", code(j), gap[cell(j)]))
        elif typ == 1:
            for j in range(length):
                out.append(("D", coord[cell(j)], old(j), "-", gap[cell(j)]))
        elif typ == 3:
            if present[b]:
                o = old(0)
                if o == "-" or o == "x":
                    odd += 1                              # "NOT ACTUALLY A SUBSTITUTION"
                out.append(("S", coord[cell(0)], o, code(0), gap[cell(0)]))
        # NSNPI, NSNPD and above: no entry (:3913, :3987)
    return out, odd


def node_lines(name, entries) -> str:
    """:4025-4055."""
    out = [f"Substitutions:\t{name}\t"]
    out += [f" > {'g' if g else ''}{o}{c + 1}{n}" for kind, c, o, n, g in entries if kind == "S"]
    out.append(f"\nInsertions:\t{name}\t")
    out += [f" > {'g' if g else ''}{c + 1}{n}" for kind, c, o, n, g in entries if kind == "I"]
    out.append(f"\nDeletions:\t{name}\t")
    out += [f" > {'g' if g else ''}{c + 1}{o}" for kind, c, o, n, g in entries if kind == "D"]
    out.append("\n")
    return "".join(out)


def node_entry_lists(pm):
    """Per node its entries, and the odd substitutions in total (the cases' checks read these)."""
    if getattr(pm, "_arrays", None) is not None:
        pm = _Lists(pm)
    if any(secondary != -1 for muts in pm.nuc_muts for _, secondary, *_ in muts):
        raise Unsupported("secondary blocks")
    parent = _parents(pm)
    max_id = max(b for b, _ in pm.blocks)
    is_block = {b for b, _ in pm.blocks}
    layout = {b: block_sequence(pm, [], b) for b in is_block}   # the cells: the same for every node
    for muts in pm.nuc_muts:
        for b, _, pos, g, info, _ in muts:
            typ, length = info & 7, info >> 4
            if typ > 5:
                continue
            if b not in is_block:
                raise Unsupported("mutation on a missing block")
            for j in range(1 if typ >= 3 else length):
                p = pos if g != -1 else pos + j
                if p < 0 or p >= len(layout[b]) or g < -1 or (g != -1 and g + j >= len(layout[b][p][1])):
                    raise ArgError("mutation outside its block")
    paths = [_path(pm, parent, v) for v in range(pm.num_nodes)]
    states = [NodeState(pm, paths[v], max_id, is_block) for v in range(pm.num_nodes)]
    root = states[pm.root]
    coord, gap = root_map(root)
    for s in states:
        if any(not h and not f for h, f in zip(s.held, s.forward)):
            raise Unsupported("a block not held but flagged reverse")
    entries, odd = [], 0
    for v in range(pm.num_nodes):
        if v == pm.root:
            entries.append([])
            continue
        e, o = node_entries(pm, v, paths[v], states[parent[v]], root, coord, gap)
        entries.append(e)
        odd += o
    return entries, odd


def print_mutations(pm):
    """(text, odd_substitutions)."""
    entries, odd = node_entry_lists(pm)
    return "".join(node_lines(pm.names[v], e) for v, e in enumerate(entries)), odd
