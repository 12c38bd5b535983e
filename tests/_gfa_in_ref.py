"""Python restatement of the reference's GFA construction up to the block-state matrix:
parse (src/panman.cpp:729-753), block order (GfaGraph::GfaGraph, :6060-6142, with chain_align,
src/chaining.cpp: the range tree's build :71-84, its pre-order query :89-103, find_chain's barrier
loop :105-150, chaining :153-232, build_consensus :235-283) and the two-pointer walk of every path
against the final order (:6144-6193, states :784-797).  The per-node block mutations then come from
the oracle's block Fitch over that matrix (oracle.csr_columns, algo = MODE_BLOCK_FITCH).

Two places of the reference depend on library internals; `Ambiguous` is raised instead of guessing:
  * a path that repeats a segment of the consensus gives points with equal x, and the range tree's
    std::sort by x alone (:75) leaves their order unspecified;
  * a maximum of the final score loop (:214-220) that is not unique is resolved by the iteration
    order of an unordered_map.
UNAMBIGUOUS_SEEDS lists seeds of random_gfa on which neither happens (checked on the CPU by
tests/test_gfa_in_ref.py)."""
from __future__ import annotations

import numpy as np

from _trees import parse_newick, random_tree, to_newick

MODE_BLOCK_FITCH = 2
K = 4000
MATCH = 50
ORIGIN = (-1, -1)


class Ambiguous(Exception):
    pass


# ---- parse -----------------------------------------------------------------------------------------

def parse(text: str):
    """(nodes, paths): paths = [(name, [(segment, forward)])] in byte order of the names."""
    nodes, paths = {}, {}
    for line in text.split("\n"):
        f = line.split("\t")
        if f[0] == "S":
            nodes[f[1]] = f[2]
        elif f[0] == "P":
            paths[f[1]] = [(v[:-1], v[-1] == "+") for v in (f[2].split(",") if f[2] else [])]
    return nodes, sorted(paths.items(), key=lambda kv: kv[0].encode())


# ---- src/chaining.cpp ------------------------------------------------------------------------------

class _Node:
    __slots__ = ("point", "left", "right")


def _construct(pts, start, end):
    """constructRangeTree: the slice sorted by x (it already is: the points come sorted by (x, y)
    and hold distinct x), the median the node, the halves its subtrees."""
    if start > end:
        return None
    n = _Node()
    mid = (start + end) // 2
    n.point = pts[mid]
    n.left = _construct(pts, start, mid - 1)
    n.right = _construct(pts, mid + 1, end)
    return n


def _query(n, lo, hi, out):
    """queryRange: pre-order -- the node, its left subtree, its right subtree."""
    if n is None:
        return
    x, y = n.point
    if lo[0] <= x <= hi[0] and lo[1] <= y <= hi[1]:
        out.append(n.point)
    if n.left is not None and lo[0] <= x:
        _query(n.left, lo, hi, out)
    if n.right is not None and hi[0] >= x:
        _query(n.right, lo, hi, out)


def _find_chain(root, point, score):
    if point == (0, 0):
        score[point] = (MATCH, ORIGIN)
        return
    result = []
    _query(root, (max(point[0] - K, 0), max(point[1] - K, 0)), (point[0] - 1, point[1] - 1), result)
    best, best_node = 10, ORIGIN
    xb = yb = -1   # the barrier
    for p in reversed(result):
        if p[0] <= xb and p[1] <= yb:
            continue
        cost = -(point[0] - p[0] + point[1] - p[1])
        if cost + score[p][0] + MATCH > best:
            best = cost + score[p][0] + MATCH
            best_node = p
        if xb < p[0]:
            xb = p[0] - 1
        if yb < p[1]:
            yb = p[1] - 1
    score[point] = (best, best_node)


def chaining(cons, sample):
    """The chain, best point first; also returns the best score (for the hand cases)."""
    pts = sorted((i, j) for i, c in enumerate(cons) for j, s in enumerate(sample) if c == s)
    if len({p[0] for p in pts}) != len(pts):
        raise Ambiguous("a path repeats a segment of the consensus: equal-x points")
    if not pts:
        return [], None
    root = _construct(pts, 0, len(pts) - 1)
    score = {p: (-1, ORIGIN) for p in pts}
    for p in pts:
        _find_chain(root, p, score)
    best = max(v[0] for v in score.values())
    seeds = [p for p in pts if score[p][0] == best]
    if len(seeds) != 1:
        raise Ambiguous(f"the best score {best} is reached at {seeds}")
    chain, seed = [], seeds[0]
    while True:
        chain.append(seed)
        seed = score[seed][1]
        if seed == ORIGIN:
            break
    return chain, (best, seeds[0])


def build_consensus(chain, cons, sample, int_cons, counter):
    """-> (cons_new, int_cons_new, int_sample, new ids -> names); counter = [numBlocks]."""
    cons_new, int_cons_new, int_sample, named = [], [], [], {}
    pc = ps = -1

    def fresh(j):
        cons_new.append(sample[j])
        int_sample.append(counter[0])
        named[counter[0]] = sample[j]
        int_cons_new.append(counter[0])
        counter[0] += 1

    for cc, sc in reversed(chain):
        for j in range(pc + 1, cc):
            cons_new.append(cons[j])
            int_cons_new.append(int_cons[j])
        for j in range(ps + 1, sc):
            fresh(j)
        cons_new.append(cons[cc])
        int_sample.append(int_cons[cc])
        int_cons_new.append(int_cons[cc])
        pc, ps = cc, sc
    for j in range(pc + 1, len(cons)):
        cons_new.append(cons[j])
        int_cons_new.append(int_cons[j])
    for j in range(ps + 1, len(sample)):
        fresh(j)
    return cons_new, int_cons_new, int_sample, named


# ---- GfaGraph ----------------------------------------------------------------------------------------

def block_order(paths):
    """-> (segment name per block in final order, block ids per path step)."""
    counter = [0]
    names, cons, int_cons, int_seqs = {}, [], [], []
    for k, (_, steps) in enumerate(paths):
        sample = [s for s, _ in steps]
        if k == 0:
            for s in sample:
                cons.append(s)
                names[counter[0]] = s
                int_cons.append(counter[0])
                counter[0] += 1
            int_seqs.append(list(int_cons))
            continue
        chain, _ = chaining(cons, sample)
        cons, int_cons, int_sample, named = build_consensus(chain, cons, sample, int_cons, counter)
        names.update(named)
        int_seqs.append(int_sample)
    order = {b: i for i, b in enumerate(int_cons)}
    return [names[b] for b in int_cons], [[order[b] for b in seq] for seq in int_seqs]


def aligned_codes(total: int, seq, strands):
    """getAlignedSequences + getAlignedStrandSequences as block states: 0 absent, 1 forward,
    2 reverse.  The walk as written: p1 over the blocks, p2 over the path."""
    row = np.zeros(total, np.uint8)
    p1 = p2 = 0
    while p1 < total and p2 < len(seq):
        if p1 == seq[p2]:
            row[p1] = 1 if strands[p2] else 2
            p2 += 1
        p1 += 1
    return row


class Built:
    """blocks: the sequence per block; names / off / idx / root: the tree (pre-order node ids,
    the reference's node names); rows: path name -> aligned states; node_row / codes: the matrix
    of the leaves' rows as the oracle takes it."""

    def records(self, oracle):
        """{(node name, block, blockMutInfo, inversion)} of the oracle's block Fitch."""
        if not self.blocks:
            return set()
        _, recs = oracle.csr_columns(self.off, self.idx, self.root, self.names, self.codes, self.node_row,
                                     np.zeros(len(self.blocks), np.uint8), None, algo=MODE_BLOCK_FITCH)
        return {(self.names[int(r[0])], int(r[1]), int(r[2]), int(r[3])) for r in recs}


def build(text: str, newick: str) -> Built:
    nodes, paths = parse(text)
    seg_of_block, int_seqs = block_order(paths)
    b = Built()
    b.blocks = [nodes[s] for s in seg_of_block]
    b.rows = {name: aligned_codes(len(b.blocks), seq, [fw for _, fw in steps])
              for (name, steps), seq in zip(paths, int_seqs)}
    b.names, b.off, b.idx, b.root = parse_newick(newick.split("\n")[0])
    b.node_row = np.full(len(b.names), -1, np.int32)
    rows = []
    for v, name in enumerate(b.names):
        if b.off[v] == b.off[v + 1] and name in b.rows:
            b.node_row[v] = len(rows)
            rows.append(b.rows[name])
    b.codes = np.array(rows, np.uint8).reshape(len(rows), len(b.blocks))
    return b


def panmat_records(pm) -> set:
    """The same set from a built PanMAT (PanmanFile.to_panmat)."""
    a = pm._arrays
    off = a["block_mut_offsets"]
    out = set()
    for v in range(pm.num_nodes):
        for k in range(int(off[v]), int(off[v + 1])):
            out.add((pm.names[v], int(a["block_mut_primary"][k]), int(a["block_mut_info"][k]),
                     int(a["block_mut_inversion"][k])))
    return out


def panmat_blocks(pm) -> list[str]:
    """Every block's sequence, decoded (8 codes per word, MSB first, code 0 ends)."""
    a = pm._arrays
    chars = "-ACMGRSVTWYHKDBN"
    out = []
    for i in range(len(a["block_primary"])):
        assert int(a["block_primary"][i]) == i
        s = ""
        for w in a["block_seq"][int(a["block_seq_offsets"][i]):int(a["block_seq_offsets"][i + 1])]:
            for j in range(8):
                c = (int(w) >> (4 * (7 - j))) & 15
                if c:
                    s += chars[c]
        out.append(s)
    return out


# ---- random inputs -------------------------------------------------------------------------------------

def random_gfa(seed: int, repeats: bool = False):
    """(GFA text, Newick): 5-40 segments of ACGT, 8-30 leaves whose paths are the base order with
    deletions, reverse steps and moved runs; polytomies on odd seeds; a leaf or two without a path
    and a path no leaf names.  `repeats` also repeats a segment inside some paths (Ambiguous)."""
    rng = np.random.default_rng(7000 + seed)
    nseg = int(rng.integers(5, 41))
    leaves = int(rng.integers(8, 31))
    segs = {f"s{k + 1}": "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 13)))) for k in range(nseg)}
    base = list(segs)
    off, idx, root = random_tree(leaves, rng, max_children=4 if seed % 2 else 2, unary=0.0)
    names = [f"t{v:03d}" if off[v] == off[v + 1] else "" for v in range(len(off) - 1)]
    lines = ["H\tVN:Z:1.0"] + [f"S\t{k}\t{v}" for k, v in segs.items()]
    no_path = set(rng.choice(leaves, size=int(rng.integers(0, 3)), replace=False).tolist())
    for t in list(range(leaves)) + ["extra"]:
        if t in no_path:
            continue
        steps = [s for s in base if rng.random() >= 0.15] or [base[0]]
        if rng.random() < 0.3 and len(steps) >= 4:   # a moved run
            a = int(rng.integers(0, len(steps) - 1))
            b = int(rng.integers(a + 1, min(len(steps), a + 6) + 1))
            run, rest = steps[a:b], steps[:a] + steps[b:]
            at = int(rng.integers(0, len(rest) + 1))
            steps = rest[:at] + run + rest[at:]
        if repeats and rng.random() < 0.5:
            at = int(rng.integers(0, len(steps) + 1))
            steps = steps[:at] + [steps[int(rng.integers(0, len(steps)))]] + steps[at:]
        strands = ["-" if rng.random() < 0.15 else "+" for _ in steps]
        name = t if isinstance(t, str) else names[t]
        lines.append(f"P\t{name}\t" + ",".join(s + d for s, d in zip(steps, strands)) + "\t*")
        if rng.random() < 0.3:
            lines.append(f"L\t{steps[0]}\t+\t{steps[-1]}\t+\t0M")
    lines.insert(int(rng.integers(1, len(lines))), "")   # a blank line
    return "\n".join(lines) + "\n", to_newick(off, idx, root, names)


# seeds of random_gfa(seed) on which build() does not raise Ambiguous
UNAMBIGUOUS_SEEDS = [2, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15]
AMBIGUOUS_SEEDS = [0, 1, 3, 9]   # the best score is reached twice
