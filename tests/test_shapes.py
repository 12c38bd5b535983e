"""The generators of _shapes.py give what test_gpu_paths.py relies on: every requested degree,
every child kind in the first two child slots and beyond them, unary nodes, the three record
word classes in every tile, and the score identity the GPU tests use (CPU only)."""
import numpy as np
import pytest

import _shapes
from _shapes import KINDS, MAIN_DEGREES, TILE_WORDS, WIDE_DEGREES, WORD
from _trees import names_for


def _kids(off, idx, v):
    return [int(c) for c in idx[off[v]:off[v + 1]]]


def _kind(off, idx, v):
    """The kind of child v, from the tree alone."""
    k = _kids(off, idx, v)
    leaf = [off[c] == off[c + 1] for c in k]
    if not k:
        return "leaf"
    if len(k) == 1 and leaf[0]:
        return "single"
    if len(k) == 2 and all(leaf):
        return "cherry"
    if len(k) == 2:
        cherries = sum(_kind(off, idx, c) == "cherry" for c in k)
        if cherries + sum(leaf) == 2 and cherries >= 1:
            return "s2" if cherries == 1 else "s3"
    return "rec"


def _check_tree(off, idx, root):
    """np.diff(off) consistent, a single root, every node reachable (exactly once)."""
    n = off.shape[0] - 1
    deg = np.diff(off)
    assert off[0] == 0 and (deg >= 0).all() and off[-1] == idx.shape[0] == n - 1
    assert idx.min() >= 0 and idx.max() < n
    assert np.unique(idx).shape[0] == n - 1 and root not in set(idx.tolist())
    leaves = int((deg == 0).sum())
    assert (deg[:leaves] == 0).all() and (deg[leaves:] > 0).all()   # leaf ids first
    seen, stack = 0, [root]
    while stack:
        v = stack.pop()
        seen += 1
        stack += _kids(off, idx, v)
    assert seen == n


def _heights(off, idx, root):
    n = off.shape[0] - 1
    h = np.zeros(n, np.int64)
    order, stack = [], [root]
    while stack:
        v = stack.pop()
        order.append(v)
        stack += _kids(off, idx, v)
    for v in reversed(order):
        k = _kids(off, idx, v)
        h[v] = 1 + max(h[c] for c in k) if k else 0
    return h


def _materialised(off, idx, root):
    """Internal nodes the subtree form keeps: not a one- or two-leaf leaf-parent, not an S2 / S3
    node under a parent of out-degree <= 2 (pm_plan.cpp: leaf_parent_like, sshape_of)."""
    n = off.shape[0] - 1
    parent = np.full(n, -1, np.int64)
    for v in range(n):
        for c in _kids(off, idx, v):
            parent[c] = v
    out = []
    for v in range(n):
        if off[v] == off[v + 1]:
            continue
        kind = _kind(off, idx, v)
        if v != root and (kind in ("single", "cherry") or
                          (kind in ("s2", "s3") and off[parent[v] + 1] - off[parent[v]] <= 2)):
            continue
        out.append(v)
    return out


@pytest.mark.parametrize("degrees,unary_every", [(MAIN_DEGREES, 7), (MAIN_DEGREES, 0), (WIDE_DEGREES, 0)])
def test_edge_tree_census(degrees, unary_every):
    off, idx, root = _shapes.edge_tree(degrees, unary_every=unary_every)
    _check_tree(off, idx, root)
    n = off.shape[0] - 1
    assert n <= 4200, n
    deg = np.diff(off)
    for d in degrees:
        assert (deg == d).any(), d
    first, later = set(), set()
    for v in np.flatnonzero(deg >= 4):
        kinds = [_kind(off, idx, c) for c in _kids(off, idx, v)]
        first |= set(kinds[:2])
        later |= set(kinds[2:])
    assert first == set(KINDS) and later == set(KINDS), (first, later)
    # unary nodes above internal nodes (inside the spine), beyond the one-leaf leaf-parents
    unary_inner = [v for v in np.flatnonzero(deg == 1) if off[idx[off[v]]] != off[idx[off[v]] + 1]]
    if unary_every:
        assert len(unary_inner) >= 5
    else:
        assert len(unary_inner) <= 1   # (the degree-1 feature node only)
    # the spine: the tree is deeper than one 32-height band
    assert _heights(off, idx, root)[root] > 32


@pytest.mark.parametrize("heights", [31, 32, 33, 64, 65, 129])
def test_ladder_heights(heights):
    off, idx, root = _shapes.ladder(heights)
    _check_tree(off, idx, root)
    mat = _materialised(off, idx, root)
    h = _heights(off, idx, root)
    # one materialised node at every height 1..heights, the root on top
    assert sorted(h[mat].tolist()) == list(range(1, heights + 1))
    assert h[root] == heights


@pytest.mark.parametrize("nodes", [63, 64, 65])
def test_fat_cluster_nodes(nodes):
    off, idx, root = _shapes.fat_cluster(nodes)
    _check_tree(off, idx, root)
    mat = _materialised(off, idx, root)
    assert len(mat) == nodes
    h = _heights(off, idx, root)
    assert h[root] < 32   # one band
    # every internal child of a materialised node is materialised or a cherry: the cluster is
    # the whole tree
    for v in mat:
        for c in _kids(off, idx, v):
            assert off[c] == off[c + 1] or c in mat or _kind(off, idx, c) == "cherry"


def test_fat_cluster_five_live_sets():
    off, idx, root = _shapes.fat_cluster(0, five_live=True)
    _check_tree(off, idx, root)
    mat = set(_materialised(off, idx, root))
    h = _heights(off, idx, root)
    five = [v for v in mat if sum(c in mat for c in _kids(off, idx, v)) == 5]
    assert len(five) == 1
    assert len({int(h[c]) for c in _kids(off, idx, five[0])}) == 1
    assert len(mat) == 17


@pytest.mark.parametrize("width", [255, 65537])
def test_star_with_sibling(width):
    off, idx, root = _shapes.star_with_sibling(width)
    _check_tree(off, idx, root)
    assert np.diff(off).max() == width
    kinds = {_kind(off, idx, c) for v in _kids(off, idx, root) for c in _kids(off, idx, v)}
    assert {"s2", "s3"} <= kinds


def _word_census(codes, cons):
    """Per word, from the leaf rows alone: 0 every leaf equals the consensus, 1 every leaf holds
    one common non-consensus code at each site, 2 the rest."""
    sites = cons.shape[0]
    same = (codes == codes[0]).all(axis=0)
    is_cons = same & (codes[0] == cons)
    non_cons = same & (codes[0] != cons)
    words = (sites + WORD - 1) // WORD
    out = np.full(words, 2, np.int64)
    for w in range(words):
        s = slice(w * WORD, min(sites, (w + 1) * WORD))
        if is_cons[s].all():
            out[w] = 0
        elif non_cons[s].all():
            out[w] = 1
    return out


def test_mixed_columns_census():
    off, idx, root = _shapes.edge_tree(MAIN_DEGREES, unary_every=7)
    sites = 4100
    codes, cons, forced = _shapes.mixed_columns(np.random.default_rng(11), off, idx, root, sites, with_forced=True)
    leaves = int((np.diff(off) == 0).sum())
    assert codes.shape == (leaves, sites) and cons.shape == (sites,) and forced.shape == (sites,)
    assert codes.dtype == np.uint8 and codes.max() <= 15
    assert {0, 15, 3, 5, 10} <= set(np.unique(codes).tolist())   # gaps, N and ambiguity codes
    cls = _word_census(codes, cons)
    assert cls.shape[0] == 129
    # 4100 sites are two whole tiles of 64 words and a third of one ragged word (4 sites): the
    # three classes are required of each whole tile; the ragged word is of the mixed class
    for t in range(cls.shape[0] // TILE_WORDS):
        tile = cls[t * TILE_WORDS:(t + 1) * TILE_WORDS]
        for k in range(3):
            assert (tile == k).sum() >= 8, (t, k, np.bincount(tile, minlength=3))
    assert cls[128] == 2
    # the classes are interleaved inside a tile (non-trivial ranks): no class in one run
    for t in range(2):
        tile = cls[t * TILE_WORDS:(t + 1) * TILE_WORDS]
        assert (np.diff(tile) != 0).sum() >= 16


@pytest.mark.parametrize("degrees", [MAIN_DEGREES, WIDE_DEGREES])
def test_mixed_columns_clade_sites(degrees):
    """For every node of >= 4 children: a site where exactly the leaves under it hold one
    non-consensus code and every other leaf the consensus (one code counted out-degree times at
    that node, against a different state above it), and a site where its first child's leaves
    hold a third code -- in every whole tile."""
    off, idx, root = _shapes.edge_tree(degrees)
    sites = 2049
    codes, cons = _shapes.mixed_columns(np.random.default_rng(13), off, idx, root, sites)
    deg = np.diff(off)
    leaves = int((deg == 0).sum())
    for v in np.flatnonzero(deg >= 4):
        under = np.zeros(leaves, bool)
        under[_shapes._leaves_under(off, idx, int(v))] = True
        first = np.zeros(leaves, bool)
        first[_shapes._leaves_under(off, idx, int(idx[off[v]]))] = True
        outside = (codes[~under] == cons[None, :]).all(axis=0)
        inside = codes[under]
        full = outside & (inside == inside[0]).all(axis=0) & (inside[0] != cons)
        rest = inside[~first[under]]
        short = outside & (rest == rest[0]).all(axis=0) & (rest[0] != cons) & \
            (codes[first] == codes[first][0]).all(axis=0) & (codes[first][0] != rest[0]) & (codes[first][0] != cons)
        assert full[:2048].any() and short[:2048].any(), (int(deg[v]), int(full.sum()), int(short.sum()))
        # hole sites: for every child j, a site where exactly child j's leaves (and every leaf
        # outside the node) hold the consensus and the node's other leaves one common other code
        at_cons = inside == cons[None, :]
        holes = set()
        for s in np.flatnonzero(outside & ~at_cons.all(axis=0)):
            other = inside[~at_cons[:, s], s]
            if (other == other[0]).all():
                holes.add(at_cons[:, s].tobytes())
        for c in _kids(off, idx, int(v)):
            mask = np.zeros(leaves, bool)
            mask[_shapes._leaves_under(off, idx, c)] = True
            assert mask[under].tobytes() in holes, (int(deg[v]), c)


@pytest.mark.parametrize("algo", [0, 1])
def test_oracle_score_identity_on_edge_tree(oracle, algo):
    off, idx, root = _shapes.edge_tree(MAIN_DEGREES, unary_every=7)
    sites = 2049
    codes, cons = _shapes.mixed_columns(np.random.default_rng(12), off, idx, root, sites)
    node_row = _shapes.leaf_rows(off)
    _, recs, rootc = oracle.csr_columns(off, idx, root, names_for(off), codes, node_row, cons, None,
                                        algo=algo, threads=8, with_root=True)
    assert rootc.shape == (sites,) and recs.shape[0] > 0
    # the score identity of the GPU tests: one record per changed non-root node and site, so the
    # per-site record count is the parsimony score; it is at least the number of distinct
    # unambiguous leaf states minus one (each needs its own change), and zero where every leaf
    # holds the consensus
    score = np.bincount(recs[recs[:, 0] != root][:, 1], minlength=sites)
    base = np.isin(codes, [1, 2, 4, 8])
    distinct = np.zeros(sites, np.int64)
    for c in (1, 2, 4, 8):
        distinct += ((codes == c) & base).any(axis=0)
    assert (score >= np.maximum(distinct - 1, 0)).all()
    quiet = (codes == cons[None, :]).all(axis=0)
    assert quiet.any() and (score[quiet] == 0).all()
    for t0 in range(0, sites, TILE_WORDS * WORD):
        assert (score[t0:t0 + TILE_WORDS * WORD] > 0).any()
