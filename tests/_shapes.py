"""Deterministic edge-case trees and mixed-class columns (host only, numpy).

Every generator returns (off, idx, root) in the CSR form of _trees.random_tree, leaf ids first.
The shapes are built around the engine's planner and launcher limits (pm_plan.cpp,
pm_cluster.cpp): out-degree classes <= 3 | 4-15 | 16-255 | > 255, the sweeps' 64 nodes per
cluster, 32 heights per band and 4 LDS slots, and the compressed records' three word classes
(consensus, simple, complex)."""
from __future__ import annotations

import numpy as np

# child kinds of a feature node, in cycle order
KINDS = ("leaf", "cherry", "single", "s2", "s3", "rec")

MAIN_DEGREES = (1, 2, 3, 4, 15, 16, 63, 64, 65, 66, 255)
# (every feature node of the second tree has >= 4 children, six of them so that the first two
# slots still see every kind)
WIDE_DEGREES = (4, 5, 256, 257, 300, 6)

WORD = 32          # sites per record word
TILE_WORDS = 64    # words per tile


class _Builder:
    def __init__(self):
        self.kids = []

    def leaf(self):
        self.kids.append(None)
        return len(self.kids) - 1

    def node(self, children):
        self.kids.append(list(children))
        return len(self.kids) - 1

    def cherry(self):
        return self.node([self.leaf(), self.leaf()])

    def kind(self, name, variant=0):
        if name == "leaf":
            return self.leaf()
        if name == "cherry":
            return self.cherry()
        if name == "single":
            return self.node([self.leaf()])
        if name == "s2":
            return self.node([self.cherry(), self.leaf()])
        if name == "s3":
            return self.node([self.cherry(), self.cherry()])
        # a materialised internal child: a binary subtree of 5, 6 or 7 leaves
        cur = self.node([self.node([self.cherry(), self.cherry()]), self.leaf()])
        for _ in range(variant % 3):
            cur = self.node([cur, self.leaf()])
        return cur

    def chain(self, length):
        """`length` materialised nodes one above the other: a three-leaf node (out-degree 3 is
        never evaluated inline), then (chain, cherry) nodes."""
        cur = self.node([self.leaf(), self.leaf(), self.leaf()])
        for _ in range(length - 1):
            cur = self.node([cur, self.cherry()])
        return cur

    def csr(self, root):
        """Leaves renumbered first (creation order), internal nodes after them."""
        n = len(self.kids)
        new = np.zeros(n, np.int64)
        leaves = [v for v in range(n) if self.kids[v] is None]
        inner = [v for v in range(n) if self.kids[v] is not None]
        new[leaves] = np.arange(len(leaves))
        new[inner] = len(leaves) + np.arange(len(inner))
        off = np.zeros(n + 1, np.int32)
        idx = []
        for k, v in enumerate(inner):
            idx += [int(new[c]) for c in self.kids[v]]
            off[len(leaves) + k + 1] = len(idx)
        off[: len(leaves) + 1] = 0
        return off, np.array(idx, np.int32), int(new[root])


def edge_tree(degrees=MAIN_DEGREES, depth_pad=40, unary_every=0):
    """A caterpillar spine with one feature node per entry of `degrees` hanging off it.

    Feature node i has degrees[i] children whose kinds cycle through KINDS starting at kind i,
    so the first two child slots (the ones with up slots / push_sub) take every kind in turn
    across the feature nodes.  (The engine moves a node's heaviest internal child to slot 0 on
    upload; slot 1 keeps the kind given here unless it was the heaviest.)  Between feature nodes
    the spine has two plain nodes (a leaf, then a cherry beside the spine child); `depth_pad`
    plain spine nodes follow the last feature node, so the top bands are pure chains and the
    default plan sweeps them.  unary_every = k > 0 puts a unary node above every k-th spine
    node."""
    b = _Builder()
    spine = 0
    cur = b.node([b.leaf(), b.leaf(), b.leaf()])

    def up(side):
        nonlocal cur, spine
        cur = b.node([cur, side])
        spine += 1
        if unary_every > 0 and spine % unary_every == 0:
            cur = b.node([cur])

    for i, deg in enumerate(degrees):
        # (five-leaf subtrees only under the widest nodes: the tree stays near 4 000 nodes)
        feature = b.node([b.kind(KINDS[(i + j) % len(KINDS)], variant=0 if deg > 255 else i + j)
                          for j in range(deg)])
        up(feature)
        up(b.leaf())
        up(b.cherry())
    for k in range(depth_pad):
        up(b.leaf() if k % 2 else b.cherry())
    return b.csr(cur)


def ladder(heights):
    """A pure chain of exactly `heights` materialised heights: a three-leaf node at height 1,
    then (chain, cherry) nodes up to the root.  Every level of the post-order holds one node, so
    the planner's bands are cut by kClBandHeights alone: ceil(heights / 32) bands."""
    b = _Builder()
    return b.csr(b.chain(heights))


def fat_cluster(nodes, five_live=False):
    """A subtree of exactly `nodes` materialised nodes, balanced over four chains:
    root = (X, Y), X = (chain, chain), Y = (chain, chain), the chains' lengths differing by at
    most one (the longer ones under X).  It spans under 32 heights and needs three LDS slots,
    so up to kClMaxSteps = 64 nodes it is one cluster.

    five_live: instead a node with five chains of three nodes each as children (five record
    children of equal height, all live at the node's step: one more than kClSlots) under a
    binary root."""
    b = _Builder()
    if five_live:
        p = b.node([b.chain(3) for _ in range(5)])
        return b.csr(b.node([p, b.cherry()]))
    rem = nodes - 3
    lens = [rem // 4 + (1 if k < rem % 4 else 0) for k in range(4)]
    x = b.node([b.chain(lens[0]), b.chain(lens[1])])
    y = b.node([b.chain(lens[2]), b.chain(lens[3])])
    return b.csr(b.node([x, y]))


def star_with_sibling(width):
    """root = (star, sib): a star of `width` leaves beside sib = (S2, S3), whose two children
    the subtree form evaluates inline (so the tree has S-shaped nodes and, with every leaf
    present, runs in the subtree form)."""
    b = _Builder()
    star = b.node([b.leaf() for _ in range(width)])
    sib = b.node([b.kind("s2"), b.kind("s3")])
    return b.csr(b.node([star, sib]))


# mixed_columns' committed rates: per tile of 64 words, QUIET words stay at the consensus in
# every leaf, UNIFORM words hold one non-consensus code per site in every leaf, RANDOM words
# are uniformly random codes; the other words evolve down the tree at one of EDGE_RATES changes
# per edge and site.  SINGLE_SITES sites per tile (in evolving words) are uniformly random too.
QUIET_PER_TILE = 14
UNIFORM_PER_TILE = 12
RANDOM_PER_TILE = 6
SINGLE_SITES = 8
CLADE_NODES = 12   # (two clade sites per tile for each of the widest nodes of >= 4 children)
EDGE_RATES = (0.0005, 0.003, 0.02)


def mixed_columns(rng, off, idx, root, sites, with_forced=False):
    """Leaf codes [leaves, sites] (every leaf present, rows in leaf-id order) and the consensus,
    mixing the three record word classes inside every tile, with clade and hole sites at the
    widest nodes (below); with_forced adds a forced root vector.  Returns (codes, cons) or
    (codes, cons, forced)."""
    n = off.shape[0] - 1
    leaves = int((np.diff(off) == 0).sum())
    words = (sites + WORD - 1) // WORD
    cons = rng.choice(np.array([0, 1, 2, 4, 8], np.uint8), size=sites, p=[0.04, 0.24, 0.24, 0.24, 0.24])
    # word classes: 0 quiet, 1 uniform, 2 random, 3 + k evolving at EDGE_RATES[k]
    cls = np.zeros(words, np.int64)
    for t0 in range(0, words, TILE_WORDS):
        deck = [0] * QUIET_PER_TILE + [1] * UNIFORM_PER_TILE + [2] * RANDOM_PER_TILE
        deck += [3 + k % len(EDGE_RATES) for k in range(TILE_WORDS - len(deck))]
        deck = rng.permutation(np.array(deck))
        m = min(TILE_WORDS, words - t0)
        cls[t0:t0 + m] = deck[:m]
    if words % TILE_WORDS == 1:
        cls[-1] = 3   # a ragged tile of one word: an evolving one
    site_cls = np.repeat(cls, WORD)[:sites]
    rate = np.zeros(sites)
    for k, r in enumerate(EDGE_RATES):
        rate[site_cls == 3 + k] = r
    # evolve down the tree from the consensus
    bases = np.array([1, 2, 4, 8], np.uint8)
    state = np.zeros((n, sites), np.uint8)
    state[root] = cons
    stack = [root]
    while stack:
        u = stack.pop()
        for c in idx[off[u]:off[u + 1]]:
            hit = rng.random(sites) < rate
            row = state[u].copy()
            row[hit] = bases[rng.integers(0, 4, size=int(hit.sum()))]
            state[c] = row
            stack.append(int(c))
    codes = np.ascontiguousarray(state[:leaves])
    for w in np.flatnonzero(cls == 1):
        s0, s1 = w * WORD, min(sites, (w + 1) * WORD)
        free = np.array([c for c in range(16) if c not in set(cons[s0:s1].tolist())], np.uint8)
        if w % 2:   # one code for the whole word
            codes[:, s0:s1] = free[rng.integers(0, free.size)]
        else:       # a code per site
            codes[:, s0:s1] = free[rng.integers(0, free.size, size=s1 - s0)][None, :]
    for w in np.flatnonzero(cls == 2):
        s0, s1 = w * WORD, min(sites, (w + 1) * WORD)
        codes[:, s0:s1] = rng.integers(0, 16, size=(leaves, s1 - s0))
    evolving = np.flatnonzero(site_cls >= 3)
    for t0 in range(0, sites, TILE_WORDS * WORD):
        pool = evolving[(evolving >= t0) & (evolving < t0 + TILE_WORDS * WORD)]
        for s in rng.choice(pool, size=min(SINGLE_SITES, pool.size), replace=False):
            codes[:, s] = rng.integers(0, 16, size=leaves)
    # clade sites: under each of the CLADE_NODES widest nodes every leaf holds one code and
    # every other leaf the consensus, so at that node one code's count is exactly its out-degree
    # while its parent's state differs (a set that came out wrong there changes the records); at
    # a second site the node's first child holds another code (the count one short)
    deg = np.diff(off)
    wide = [int(v) for v in np.argsort(-deg, kind="stable")[:CLADE_NODES] if deg[v] >= 4]
    used = []
    for t0 in range(0, sites, TILE_WORDS * WORD):
        pool = evolving[(evolving >= t0) & (evolving < t0 + TILE_WORDS * WORD)]
        picks = rng.choice(pool, size=min(2 * len(wide), pool.size), replace=False)
        used += picks.tolist()
        for k, s in enumerate(picks):
            v = wide[k // 2]
            a, b = rng.choice(bases[bases != cons[s]], size=2, replace=False)
            codes[:, s] = cons[s]
            codes[_leaves_under(off, idx, v), s] = a
            if k % 2:
                codes[_leaves_under(off, idx, int(idx[off[v]])), s] = b
    # hole sites (first tile, as many as its evolving sites allow): for each child j of each of
    # those nodes, the node's other children hold one code and child j, like every leaf outside,
    # the consensus -- Fitch's state for the node is then the consensus only if child j was
    # folded in (it alone empties the intersection), so a child skipped at any position of the
    # node's child loop changes the records of all the others
    pool = np.setdiff1d(evolving[evolving < TILE_WORDS * WORD], np.array(used, np.int64))
    holes = [(v, j) for v in wide for j in range(int(deg[v]))]
    for (v, j), s in zip(holes, rng.permutation(pool)):
        codes[:, s] = cons[s]
        codes[_leaves_under(off, idx, v), s] = rng.choice(bases[bases != cons[s]])
        codes[_leaves_under(off, idx, int(idx[off[v] + j])), s] = cons[s]
    if with_forced:
        return codes, cons, rng.integers(0, 16, size=sites).astype(np.uint8)
    return codes, cons


def _leaves_under(off, idx, v):
    out, stack = [], [v]
    while stack:
        u = stack.pop()
        if off[u] == off[u + 1]:
            out.append(u)
        stack += [int(c) for c in idx[off[u]:off[u + 1]]]
    return np.array(out, np.int64)


def leaf_rows(off):
    """node_row for leaves_upload / the oracle: leaf i (ids first) is row i, every leaf present."""
    n = off.shape[0] - 1
    leaves = int((np.diff(off) == 0).sum())
    node_row = np.full(n, -1, np.int32)
    node_row[:leaves] = np.arange(leaves, dtype=np.int32)
    return node_row
