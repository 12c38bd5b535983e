"""A plain-Python restatement of Tree::convertToGFA (src/gfa.cpp:3-500), both branches, working
from a list-built PanMAT alone, and of the way back: the sequences a GFA text spells.

The reference runs the tips under tbb::parallel_for_each and prints from concurrent containers;
the orders it leaves to the scheduler are fixed here as pm_gfa documents them: node ids as if the
tips ran one after the other in tip (node-id) order, "P" lines in tip order, the "L" lines of the
whole-block branch in ascending (from, to) order.  Everything else -- the std::map / std::set walks
of the compaction, the merge loop that inserts into the maps it walks, the && of gfa.cpp:379, the
start tuples of the two strands that collide for block 0 -- is restated as it is written."""
from __future__ import annotations

import bisect

from _maf_ref import COMPLEMENT, NUC, _Lists, _parents, _path, block_sequence, block_state

NODE_LEN = 32
SIZE_MAX = 2 ** 64 - 1   # a size_t holding -1


class _Map:
    """std::map: operator[] inserts a default; a walk sees keys inserted ahead of it."""

    def __init__(self):
        self.d = {}
        self.keys = []

    def at(self, k):   # operator[]
        if k not in self.d:
            self.d[k] = []
            bisect.insort(self.keys, k)
        return self.d[k]

    def walk(self):
        i = 0
        while i < len(self.keys):
            k = self.keys[i]
            yield k
            i = bisect.bisect_right(self.keys, k)


def _columns(seq):
    """The block's columns in canonical order as (character, position, gap slot or -1)."""
    cols = []
    for j, (main, slots) in enumerate(seq):
        cols += [(ch, j, k) for k, ch in enumerate(slots)]
        cols.append((main, j, -1))
    return cols


def _strip(chunk):
    return "".join(ch for ch, _, _ in chunk if ch not in "-x")   # stripGaps, panman.cpp:5445-5453


def _tip_steps(pm, path, blocks, nodes):
    """One tip's walk (gfa.cpp:144-304): [(node id, strand)]; new (start, string) keys join `nodes`."""
    steps = []
    for b in blocks:
        exists, forward = block_state(pm, path, b)
        if not exists:
            continue
        cols = _columns(block_sequence(pm, path, b))
        if forward:
            walk = cols
        else:
            walk = cols[::-1]
        for c0 in range(0, len(walk), NODE_LEN):
            chunk = walk[c0:c0 + NODE_LEN]
            if forward:
                _, j, k = chunk[0]   # the first column
                start = (b, j, SIZE_MAX if k == -1 else k)
            else:
                _, j, k = chunk[-1]   # the last visited column
                start = (-b - 1, j, SIZE_MAX) if k == -1 else (-b, j, k)
                chunk = chunk[::-1]   # reversed back: canonical order, not complemented
            text = _strip(chunk)
            if not text:
                continue
            key = (start, text)
            if key not in nodes:
                nodes[key] = (len(nodes), forward)
            steps.append((nodes[key][0], forward))
    return steps


def _chunk_graph(pm, parent, tips, blocks, notes):
    nodes = {}   # allSequenceNodes: (start, string) -> (id, strand of the tip that made it)
    paths = {t: _tip_steps(pm, _path(pm, parent, t), blocks, nodes) for t in tips}
    name = {t: pm.names[t].encode() for t in tips}
    finals = {made: key[1] for key, made in nodes.items()}   # finalNodes
    if notes is not None:
        notes["creator"] = {i: strand for i, strand in nodes.values()}
        notes["paths"] = {t: list(steps) for t, steps in paths.items()}
        notes["loose"] = set()
    G, GT = _Map(), _Map()
    for t in tips:
        steps = paths[t]
        for i in range(1, len(steps)):
            G.at(steps[i - 1]).append((name[t], steps[i]))
            GT.at(steps[i]).append((name[t], steps[i - 1]))
    for m in (G, GT):
        for k in m.keys:
            m.d[k].sort()
    for u in G.walk():   # :343-409
        if u not in finals:
            continue
        while True:
            out = G.d[u]
            if len(out) != len(GT.at(u)) or not out:
                break
            check = True
            for j in range(len(out)):
                if out[j][0] != GT.at(u)[j][0]:
                    check = False
                    break
                elif j > 0 and out[j][1] != out[j - 1][1]:
                    check = False
                    break
            if not check:
                break
            dest = out[0][1]
            if len(out) != len(GT.at(dest)):
                break
            if u[1] != dest[1]:
                break
            loose = False
            for j in range(len(out)):
                if out[j][0] != GT.at(dest)[j][0] and GT.at(dest)[j][1] != u:   # :379
                    check = False
                    break
                if out[j][0] != GT.at(dest)[j][0] or GT.at(dest)[j][1] != u:
                    loose = True   # an || would have stopped here
            if len(G.at(dest)) != len(GT.at(dest)):
                break
            for j in range(len(GT.at(dest))):
                if G.at(dest)[j][0] != GT.at(dest)[j][0]:
                    check = False
                    break
            if not check:
                break
            if loose and notes is not None:
                notes["loose"] |= {u, dest}
            tail = finals.get(dest, "")   # operator[] inserts an empty text, erased below
            finals[u] = finals[u] + tail if u[1] else tail + finals[u]
            finals.pop(dest, None)
            G.d[u] = [] if dest == u else list(G.at(dest))
    text_id = {}   # sequenceToId: the last node in finals order with a text wins
    for ctr, k in enumerate(sorted(finals), 1):
        text_id[finals[k]] = ctr
    old_new = {k[0]: text_id[finals[k]] for k in sorted(finals)}
    edges = set()
    for u in G.keys:
        if u in finals:
            for _, v in G.d[u]:
                if v in finals:
                    edges.add(((old_new.get(u[0], 0), u[1]), (old_new.get(v[0], 0), v[1])))
    sequential = {}
    for k in sorted(finals):
        sequential.setdefault(old_new[k[0]], len(sequential) + 1)
    out = ["H\tVN:Z:1.1\n"]
    done = set()
    for k in sorted(finals):
        if old_new[k[0]] not in done:
            done.add(old_new[k[0]])
            out.append(f"S\t{sequential[old_new[k[0]]]}\t{finals[k]}\n")
    sign = {True: "+", False: "-"}
    for (a, sa), (b, sb) in sorted(edges):
        out.append(f"L\t{sequential[a]}\t{sign[sa]}\t{sequential[b]}\t{sign[sb]}\t0M\n")
    for t in tips:
        kept = [f"{sequential[old_new[i]]}{sign[s]}" for i, s in paths[t] if (i, s) in finals]
        out.append(f"P\t{pm.names[t]}\t{','.join(kept)}\t*\n")
    return "".join(out)


def _whole_blocks(pm, parent, tips):
    """gfa.cpp:13-118."""
    segment = {}
    for b, words in pm.blocks:
        text = ""
        for w in words:
            for k in range(8):
                code = (int(w) >> (4 * (7 - k))) & 15
                if code == 0:
                    break   # ends the word, not the block
                text += NUC[code]
        segment[b] = text   # nodes[(primary, -1)]: the last block of an id wins
    rank = {b: i for i, b in enumerate(sorted(segment))}
    slots = len(pm.blocks) + 1
    paths, links = {}, set()
    for t in tips:
        present = [False] * slots
        for node in _path(pm, parent, t):
            for b, insertion, _ in pm.block_muts[node]:
                present[b] = bool(insertion)   # :66-78: anything but BI clears, an inversion too
        paths[t] = [i for i in range(slots) if present[i]]
        links |= set(zip(paths[t], paths[t][1:]))
    out = [f"S\t{rank[b]}\t{segment[b]}\n" for b in sorted(segment)]
    out += [f"L\t{rank.get(a, 0)}\t+\t{rank.get(b, 0)}\t+\t0M\n" for a, b in sorted(links)]   # nodeIds[...]: missing reads 0
    for t in tips:
        out.append(f"P\t{pm.names[t]}\t{','.join(f'{rank.get(i, 0)}+' for i in paths[t])}\t*\n")
    return "".join(out)


def gfa(pm, notes=None) -> str:
    """The GFA text.  `notes` (a dict) receives, for the chunk branch, what a test needs to name
    the reference rule that breaks a tip's path: "creator" (node id -> strand), "paths" (tip ->
    steps before the path filter) and "loose" (nodes of merges an || at :379 would have refused)."""
    if getattr(pm, "_arrays", None) is not None:
        pm = _Lists(pm)
    parent = _parents(pm)
    tips = pm.leaves()
    if not any(pm.nuc_muts[v] for v in range(pm.num_nodes)):
        return _whole_blocks(pm, parent, tips)
    blocks = sorted({b for b, _ in pm.blocks})
    return _chunk_graph(pm, parent, tips, blocks, notes)


def gfa_to_sequences(text: str) -> dict[str, str]:
    """Per "P" line the concatenation of its segments' texts; a '-' step reversed and complemented."""
    segment, out = {}, {}
    for line in text.split("\n"):
        f = line.split("\t")
        if f[0] == "S":
            segment[f[1]] = f[2]
        elif f[0] == "P":
            seq = ""
            for step in (f[2].split(",") if f[2] else []):
                s = segment[step[:-1]]
                seq += s if step[-1] == "+" else "".join(COMPLEMENT.get(ch, "N") for ch in reversed(s))
            out[f[1]] = seq
    return out
