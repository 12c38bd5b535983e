"""A plain-Python restatement of Tree::printMAF (src/maf.cpp:68-188) and of
generateSequencesFromMAF (src/maf.cpp:4-66), working from a list-built PanMAT alone.

Every (tip, block) text comes from its own path walk, as getBlockSequenceFromReference does
(src/panman.cpp:3070-3261); the starts come from the tip's print order
(getSequenceFromReference(rotate = true), src/panman.cpp:4974-4999).  One deviation, the one
pm_maf documents: inside a block the lines are in tip (node-id) order, where the reference
iterates a tbb::concurrent_unordered_map."""
from __future__ import annotations

NUC = "-ACMGRSVTWYHKDBN"
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K",
              "B": "V", "D": "H", "H": "D", "V": "B"}   # getComplementCharacter: anything else -> 'N'


def _parents(pm):
    parent = [-1] * pm.num_nodes
    for v in range(pm.num_nodes):
        for e in range(pm.child_offsets[v], pm.child_offsets[v + 1]):
            parent[int(pm.child_index[e])] = v
    return parent


def _path(pm, parent, tip):
    """Root first."""
    path = [tip]
    while path[-1] != pm.root:
        path.append(parent[path[-1]])
    return path[::-1]


def block_state(pm, path, block):
    """(exists, strand) of one block at the end of the path (panman.cpp:3097-3124)."""
    exists, strand = False, True
    for node in path:
        for b, insertion, inversion in pm.block_muts[node]:
            if b != block:
                continue
            if insertion:
                exists, strand = True, not inversion
            elif inversion:
                strand = not strand
            else:
                exists, strand = False, True
    return exists, strand


def block_sequence(pm, path, block):
    """The block's [main, gap slots] positions after the path's mutations (panman.cpp:3130-3260)."""
    seq = []
    for b, words in pm.blocks:
        if b != block:
            continue
        end = False
        for w in words:
            for k in range(8):
                code = (w >> (4 * (7 - k))) & 15
                if code == 0:
                    end = True
                    break
                seq.append([NUC[code], []])
            if end:
                break
        seq.append(["x", []])
    for b, slots in pm.gaps:
        if b != block:
            continue
        for pos, length in slots:
            cur = seq[pos][1]
            seq[pos][1] = cur[:length] + ["-"] * (length - len(cur))
    for node in path:
        for primary, secondary, pos, gap, info, nucs in pm.nuc_muts[node]:
            if primary != block or secondary != -1:
                continue
            typ, length = info & 7, info >> 4
            if typ > 5:
                continue
            if typ >= 3:
                length = 1
            for j in range(length):
                ch = "-" if typ in (1, 5) else NUC[(nucs >> (4 * (5 - j))) & 15]
                if gap != -1:
                    seq[pos][1][gap + j] = ch
                else:
                    seq[pos + j][0] = ch
    return seq


def block_text(seq):
    """maf.cpp:163-177: per position the gap slots, then the main character; 'x' as '-'."""
    out = []
    for main, slots in seq:
        out += ["-" if ch == "x" else ch for ch in slots]
        out.append("-" if main == "x" else main)
    return "".join(out)


def print_order(pm, tip, exists, max_id):
    """Block ids in the tip's print order (panman.cpp:4974-4999, maf.cpp:93-103)."""
    ids = list(range(max_id + 1))
    rot = int(pm.rotation[tip])
    if rot != 0:
        ctr, at = -1, 0
        for i in ids:
            if exists[i]:
                ctr += 1
            if ctr == rot:
                at = i
                break
        ids = ids[at:] + ids[:at]
    if pm.inverted[tip]:
        ids.reverse()
    return ids


class _Lists:
    """The list form of a PanMAT held as flat arrays (PanmanFile.to_panmat)."""

    def __init__(self, pm):
        a = pm._arrays
        self.names, self.root, self.num_nodes = pm.names, pm.root, pm.num_nodes
        self.child_offsets, self.child_index, self.leaves = pm.child_offsets, pm.child_index, pm.leaves
        self.rotation, self.inverted, self.circular = pm.rotation, pm.inverted, pm.circular
        so, go = a["block_seq_offsets"], a["gap_offsets"]
        self.blocks = [(int(b), [int(w) for w in a["block_seq"][so[i]:so[i + 1]]])
                       for i, b in enumerate(a["block_primary"])]
        self.gaps = [(int(b), [(int(a["gap_position"][k]), int(a["gap_length"][k])) for k in range(go[i], go[i + 1])])
                     for i, b in enumerate(a["gap_primary"])]
        bo, no = a["block_mut_offsets"], a["nuc_mut_offsets"]
        self.block_muts = [[(int(a["block_mut_primary"][k]), int(a["block_mut_info"][k]), int(a["block_mut_inversion"][k]))
                            for k in range(bo[v], bo[v + 1])] for v in range(self.num_nodes)]
        self.nuc_muts = [[(int(a["nuc_mut_primary"][k]), int(a["nuc_mut_secondary"][k]), int(a["nuc_mut_position"][k]),
                           int(a["nuc_mut_gap_position"][k]), int(a["nuc_mut_info"][k]), int(a["nuc_mut_nucs"][k]))
                          for k in range(no[v], no[v + 1])] for v in range(self.num_nodes)]


def maf(pm) -> str:
    if getattr(pm, "_arrays", None) is not None:
        pm = _Lists(pm)
    parent = _parents(pm)
    max_id = max(b for b, _ in pm.blocks)
    is_block = {b for b, _ in pm.blocks}
    tips = pm.leaves()
    text, strand, start, src = {}, {}, {}, {}
    for t in tips:
        path = _path(pm, parent, t)
        exists = [False] * (max_id + 1)
        for b in is_block:
            ex, st = block_state(pm, path, b)
            if ex:
                exists[b] = True
                strand[t, b] = st
                text[t, b] = block_text(block_sequence(pm, path, b))
        ctr = 0
        for b in print_order(pm, t, exists, max_id):
            if exists[b]:
                start[t, b] = ctr
                ctr += len(text[t, b].replace("-", ""))
        src[t] = ctr
        offset = int(pm.circular[t])
        if offset >= 0:   # maf.cpp:125-136: one conditional add
            for b in range(max_id + 1):
                if exists[b]:
                    start[t, b] -= offset
                    if start[t, b] < 0:
                        start[t, b] += ctr
    groups = {}
    for b, words in pm.blocks:
        groups.setdefault(tuple(int(w) & 0xFFFFFFFF for w in words), []).append(b)
    out = ["##maf version=1\n"]
    for key in sorted(groups):   # tuples of unsigned words: lexicographic, a proper prefix first
        out.append("a\n")
        for b in groups[key]:
            for t in tips:
                if (t, b) in text:
                    size = len(text[t, b].replace("-", ""))
                    out.append(f"s\t{pm.names[t]}\t{start[t, b]}\t{size}\t{'+' if strand[t, b] else '-'}\t{src[t]}\t"
                               f"{text[t, b]}\n")
        out.append("\n")
    return "".join(out)


def maf_to_sequences(text: str) -> dict[str, str]:
    """generateSequencesFromMAF (maf.cpp:4-66): per name the 's' lines by start, gaps stripped,
    '-' strand blocks complemented and reversed, concatenated, rotated by the first start when
    it is non-zero.  A size-0 block adds nothing (and is left out of the positions, where the
    reference lets the last line at a start win)."""
    by_name = {}
    for line in text.split("\n"):
        if len(line) > 2 and line[:2] == "s\t":
            words = line.split("\t")
            assert len(words) == 7, line
            forward = words[4] == "+"
            s = "".join(ch if forward else COMPLEMENT.get(ch, "N") for ch in words[6] if ch != "-")
            if not forward:
                s = s[::-1]
            assert len(s) == int(words[3]), line
            positions = by_name.setdefault(words[1], {})
            if s:
                assert int(words[2]) not in positions, line
                positions[int(words[2])] = s
    out = {}
    for name, positions in by_name.items():
        expected, end, full = 0, 0, ""
        for pos in sorted(positions):
            if expected == 0 and pos != expected:
                expected = end = pos
            assert pos == expected, (name, pos, expected)
            full += positions[pos]
            expected += len(positions[pos])
        out[name] = full[len(full) - end:] + full[:len(full) - end]
    return out
