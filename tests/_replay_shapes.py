"""Planted PanMATs for the replay kernels' capacity and tile edges, and a pure-Python census of
what replay_flatten (pm_replay.cpp) lays out for them: canonical columns, per-node edits,
override flags, the depth-first leaf order with its group cut, and the per-(leaf, tile) counts
the kernels' capacities are compared against (pm_replay.hip: kOvrCap, kRestoreRanges, the
DfsLds block table, kDfsPCap / kDfsOCap, kFastNodes / kFastEdits).

CASES names every planted input once; test_replay_shapes.py asserts on the CPU that each sits
on its edge (Case.check), test_gpu_replay_edges.py runs the same builders on the GPU."""
from __future__ import annotations

import bisect
import functools
from dataclasses import dataclass, field

import numpy as np

from _trees import names_for, parse_newick, to_newick
from panman_amd.panmat import CODE, PanMAT

CHAR = "-ACMGRSVTWYHKDBN"
DFS_UNION_CAP, DFS_LEAVES, DFS_TILE, REPLAY_TILE, REPLAY_GROUP = 128, 16, 4096, 16384, 8
OVR_CAP, RESTORE_RANGES, DFS_PCAP, DFS_OCAP, FAST_NODES, FAST_EDITS = 1024, 6, 384, 64, 4, 16


# ---------------------------------------------------------------------------- trees
def caterpillar(leaves: int):
    """((((s0,s1),s2),s3)...): leaf k hangs off spine node k; the deepest path holds `leaves` nodes."""
    n = 2 * leaves - 1
    kids = {}
    cur = 0
    nxt = leaves
    for k in range(1, leaves):
        kids[nxt] = [cur, k]
        cur = nxt
        nxt += 1
    off = np.zeros(n + 1, np.int32)
    idx = []
    for v in range(n):
        idx += kids.get(v, [])
        off[v + 1] = len(idx)
    return off, np.array(idx, np.int32), cur


def tree_of(kids: list[list[int]]):
    """Child lists (node 0 = root) -> (names, off, idx, root)."""
    off = np.zeros(len(kids) + 1, np.int32)
    idx = []
    for v, ch in enumerate(kids):
        idx += ch
        off[v + 1] = len(idx)
    return names_for(off), off, np.array(idx, np.int32), 0


class Kids:
    """Grow a tree node by node (node 0 = root)."""

    def __init__(self):
        self.kids = [[]]

    def add(self, parent: int) -> int:
        self.kids.append([])
        self.kids[parent].append(len(self.kids) - 1)
        return len(self.kids) - 1

    def chain(self, parent: int, n: int) -> list[int]:
        out = []
        for _ in range(n):
            parent = self.add(parent)
            out.append(parent)
        return out


def ladder(leaves: int):
    """Caterpillar in the reference's naming (pre-order ids) -> (names, off, idx, root)."""
    off, idx, root = caterpillar(leaves)
    return parse_newick(to_newick(off, idx, root, names_for(off)))


def stem_ladder(stem: int, leaves: int):
    """A chain of `stem` one-child nodes under the root, then a ladder of `leaves` leaves, and
    one more leaf under the root (reroot refuses a one-child root): a deep path with few
    leaves (the deepest path holds stem + leaves nodes)."""
    k = Kids()
    at = k.chain(0, stem)[-1]
    for _ in range(leaves - 2):
        nxt = k.add(at)
        k.add(at)
        at = nxt
    k.add(at)
    k.add(at)
    k.add(0)
    return tree_of(k.kids)


def paths_of(off, idx, root):
    """{leaf: root-first path}, and the parent array."""
    n = len(off) - 1
    parent = [-1] * n
    for v in range(n):
        for c in idx[off[v]:off[v + 1]]:
            parent[int(c)] = v
    out = {}
    for v in range(n):
        if off[v] == off[v + 1]:
            p = []
            u = v
            while u >= 0:
                p.append(u)
                u = parent[u]
            out[v] = p[::-1]
    return out, parent


# ---------------------------------------------------------------------------- layout
def block_text(bid: int, n: int) -> str:
    """A deterministic ACGT block (no run structure shared between blocks)."""
    return "".join("ACGT"[(j * (2 * (bid % 5) + 1) + j // 7 + bid) & 3] for j in range(n))


class Layout:
    """Canonical columns (replay_flatten, pm_replay.cpp:143-176)."""

    def __init__(self, pm: PanMAT):
        self.len, self.slots = {}, {}
        text = {}
        for bid, words in pm.blocks:
            s = []
            for w in words:
                for k in range(8):
                    c = (w >> (4 * (7 - k))) & 15
                    if c == 0:
                        break
                    s.append(CHAR[c])
                else:
                    continue
                break
            text[bid] = "".join(s)
            self.len[bid] = len(s)
            self.slots[bid] = None
        for bid, sl in pm.gaps:
            if self.slots[bid] is None:
                self.slots[bid] = [0] * (self.len[bid] + 1)
            for p, l in sl:
                self.slots[bid][p] = l
        self.ids = sorted(self.len)
        self.M = self.ids[-1] + 1
        self.col_start, self.width, self.main_col, self.gap_col = [0] * self.M, [0] * self.M, {}, {}
        cons = bytearray()
        for bid in range(self.M):
            self.col_start[bid] = len(cons)
            if bid not in self.len:
                continue
            n, sl = self.len[bid], self.slots[bid]
            if sl is None:
                self.main_col[bid] = range(len(cons), len(cons) + n + 1)
                cons += text[bid].encode() + b"x"
            else:
                mc, gc = [], []
                for j in range(n + 1):
                    gc.append(len(cons))
                    cons += b"-" * sl[j]
                    mc.append(len(cons))
                    cons += (text[bid][j] if j < n else "x").encode()
                self.main_col[bid], self.gap_col[bid] = mc, gc
            self.width[bid] = len(cons) - self.col_start[bid]
        self.cons = bytes(cons)
        self.columns = len(cons)
        self._starts = [self.col_start[b] for b in self.ids]

    def locate(self, col: int):
        """column -> (block id, position, gap index or -1)."""
        bid = self.ids[bisect.bisect_right(self._starts, col) - 1]
        assert self.col_start[bid] <= col < self.col_start[bid] + self.width[bid], col
        if self.slots[bid] is None:
            return bid, col - self.col_start[bid], -1
        mc = self.main_col[bid]
        j = bisect.bisect_left(mc, col)
        return (bid, j, -1) if mc[j] == col else (bid, j, col - self.gap_col[bid][j])


def other(lay, col, k):
    return [c for c in "ACGT" if c != chr(lay.cons[col])][k % 3]


def snp(pm, lay, node, col, ch):
    """One substitution; ch: a letter, or a number k for the k-th base that differs from the
    consensus there (an edit that rewrites the consensus could be dropped unseen)."""
    bid, pos, gap = lay.locate(col)
    if isinstance(ch, int):
        ch = other(lay, col, ch)
    pm.add_nuc_mut(node, bid, pos, gap, 3 if gap == -1 else 4, [CODE[ch]])


def mnp(pm, lay, node, col, text):
    """A substitution run (type 0) over consecutive main columns of one gap-free block."""
    bid, pos, gap = lay.locate(col)
    assert gap == -1 and lay.slots[bid] is None and pos + len(text) <= lay.len[bid] and len(text) <= 6, (col, text)
    pm.add_nuc_mut(node, bid, pos, -1, 0, [CODE[c] for c in text])


def delete(pm, lay, node, col, n=1):
    bid, pos, gap = lay.locate(col)
    if n == 1:
        pm.add_nuc_mut(node, bid, pos, gap, 5, [0])
    else:
        assert gap == -1 and pos + n <= lay.len[bid] and n <= 6
        pm.add_nuc_mut(node, bid, pos, -1, 1, [0] * n)


def new_panmat(tree, widths, ids=None, gaps=None) -> tuple[PanMAT, Layout]:
    """Blocks of the given column widths (length + gap slots + the sentinel), every block
    inserted at the root."""
    names, off, idx, root = tree
    pm = PanMAT(names, off, idx, root)
    ids = list(range(len(widths))) if ids is None else ids
    for bid, w in zip(ids, widths):
        g = sum(l for _, l in (gaps or {}).get(bid, []))
        pm.add_block(bid, block_text(bid, w - 1 - g))
        if bid in (gaps or {}):
            pm.add_gaps(bid, gaps[bid])
        pm.add_block_mut(root, bid, True, False)
    return pm, Layout(pm)


# ---------------------------------------------------------------------------- census
class Census:
    def __init__(self, pm: PanMAT):
        lay = self.lay = Layout(pm)
        off, idx = pm.child_offsets, pm.child_index
        N = self.N = pm.num_nodes
        self.columns = lay.columns
        self.paths, self.parent = paths_of(off, idx, pm.root)
        self.leaves = sorted(self.paths)                       # rows: leaves in node-id order
        self.max_depth = max(len(p) for p in self.paths.values())
        self.dfs = self.max_depth <= DFS_UNION_CAP
        self.tile = DFS_TILE if self.dfs else REPLAY_TILE
        self.stride = (self.columns + 15) // 16 * 16
        self.tiles = (self.stride + self.tile - 1) // self.tile
        # per-node edits, the last edit of a column wins (pm_replay.cpp:179-256)
        self.node_edits = [dict() for _ in range(N)]
        for v in range(N):
            e = self.node_edits[v]
            for bid, _sec, pos, gap, info, nucs in pm.nuc_muts[v]:
                typ, n = info & 7, info >> 4
                if typ > 5:
                    continue
                if typ >= 3:
                    n = 1
                for j in range(n):
                    col = lay.main_col[bid][pos + j] if gap == -1 else lay.gap_col[bid][pos] + gap + j
                    e[col] = "-" if typ in (1, 5) else CHAR[(nucs >> (4 * (5 - j))) & 15]
        self.edits = sum(len(e) for e in self.node_edits)
        # override flags: some ancestor edits the column (pm_replay.cpp:367-400)
        kids = [[int(c) for c in idx[off[v]:off[v + 1]]] for v in range(N)]
        self.kids = kids
        self.override = [set() for _ in range(N)]
        active: dict[int, int] = {}
        stack = [(pm.root, False)]
        order = []
        while stack:
            v, leaving = stack.pop()
            if leaving:
                for c in self.node_edits[v]:
                    active[c] -= 1
                continue
            if not kids[v]:
                order.append(v)
            for c in self.node_edits[v]:
                if active.get(c, 0) > 0:
                    self.override[v].add(c)
                active[c] = active.get(c, 0) + 1
            stack.append((v, True))
            for c in reversed(kids[v]):
                stack.append((c, False))
        # per-(node, tile) plain / overriding counts
        T = self.tiles
        self.node_plain = np.zeros((N, T), np.int32)
        self.node_ovr = np.zeros((N, T), np.int32)
        for v in range(N):
            for c in self.node_edits[v]:
                (self.node_ovr if c in self.override[v] else self.node_plain)[v, c // self.tile] += 1
        # depth-first leaf order, shared prefixes, group cut (pm_replay.cpp:298-348)
        self.dfs_order = order
        self.dfs_lp, self.groups = [], []
        cnt = uni = 0
        for i, v in enumerate(order):
            pa = self.paths[v]
            lp = 0
            if i > 0:
                pb = self.paths[order[i - 1]]
                while lp < len(pa) and lp < len(pb) and pa[lp] == pb[lp]:
                    lp += 1
            if i == 0 or cnt == DFS_LEAVES or uni + (len(pa) - lp) > DFS_UNION_CAP:
                if i > 0:
                    self.groups[-1] = (self.groups[-1][0], i)
                self.groups.append((i, len(order)))
                cnt = uni = lp = 0
            uni += len(pa) - lp
            cnt += 1
            self.dfs_lp.append(lp)
        # presence (pm_replay.cpp:457-468) and the tiles' block tables
        self.present = {}
        for v in self.leaves:
            pres = set()
            for u in self.paths[v]:
                for bid, ins, inv in pm.block_muts[u]:
                    if ins:
                        pres.add(bid)
                    elif not inv:
                        pres.discard(bid)
            self.present[v] = pres
        # per tile: the real blocks overlapping it, and the ids the kernels' tables hold for it
        # (from the first id that ends beyond the tile's start while an id starts before its
        # end: ids that are no block take an empty entry, absent_ranges / dfs_leaf_tables)
        self.tile_blocks, self.tile_ids = [], []
        hi = [lay.col_start[b] + lay.width[b] for b in range(lay.M)]
        for t in range(T):
            c0, c1 = t * self.tile, min((t + 1) * self.tile, self.stride)
            first = next((b for b in range(lay.M) if hi[b] > c0), lay.M)
            ids = [b for b in range(first, lay.M) if lay.col_start[b] < c1]
            self.tile_ids.append(ids)
            self.tile_blocks.append([b for b in ids if lay.width[b] > 0])

    # ---- per (leaf, tile)
    def path_counts(self, leaf: int, t: int, lo: int = 0, hi: int | None = None):
        """(plain, overriding) edits of path positions [lo, hi) of `leaf` in tile t."""
        p = self.paths[leaf][lo:hi]
        return int(self.node_plain[p, t].sum()), int(self.node_ovr[p, t].sum())

    def max_leaf_tile(self):
        """The maxima over (leaf, tile) of the plain and of the overriding edits on a path."""
        cp, co = self.node_plain.copy(), self.node_ovr.copy()
        best_p = best_o = 0
        order = [v for p in self.paths.values() for v in p]
        done = set()
        for v in order:        # paths are root first: a parent is summed before its children
            if v in done:
                continue
            done.add(v)
            if self.parent[v] >= 0:
                cp[v] += cp[self.parent[v]]
                co[v] += co[self.parent[v]]
        for v in self.leaves:
            best_p, best_o = max(best_p, int(cp[v].max())), max(best_o, int(co[v].max()))
        return best_p, best_o

    def chunk_counts(self, leaf: int, t: int):
        """Per 64-node path chunk: (plain, overriding) edits in tile t."""
        n = len(self.paths[leaf])
        return [self.path_counts(leaf, t, q, min(q + 64, n)) for q in range(0, n, 64)]

    def absent(self, leaf: int, t: int, real: bool = True):
        """Blocks (real=False: table ids) of tile t absent at the leaf."""
        return [b for b in (self.tile_blocks if real else self.tile_ids)[t] if b not in self.present[leaf]]

    def all_present(self):
        return all(set(self.lay.ids) <= self.present[v] for v in self.leaves)

    def plain(self, pm):
        """Every block present and forward at every leaf, no rotation, inversion or circular offset."""
        return bool(self.all_present() and not any(inv for lst in pm.block_muts for _, _, inv in lst)
                    and not pm.rotation.any() and not pm.inverted.any() and (pm.circular < 0).all())

    # ---- depth-first kernel
    def group_of(self, i: int):
        return next(g for g in self.groups if g[0] <= i < g[1])

    def group_prefix(self, g):
        i0, i1 = g
        return min([len(self.paths[self.dfs_order[i0]])] + [self.dfs_lp[k] for k in range(i0 + 1, i1)])

    def group_nodes(self, g):
        return len({v for i in range(*g) for v in self.paths[self.dfs_order[i]]})

    def stack_counts(self, i: int, t: int):
        """(plain, overriding) entries the undo stacks would hold once leaf i (depth-first
        index) is applied in tile t: its path positions from the group's shared prefix on."""
        return self.path_counts(self.dfs_order[i], t, self.group_prefix(self.group_of(i)))

    def transition(self, i: int, t: int):
        """(entering nodes, most plain edits on one of them, most overriding) of leaf i in tile t."""
        p = self.paths[self.dfs_order[i]][self.dfs_lp[i]:]
        return len(p), int(self.node_plain[p, t].max()), int(self.node_ovr[p, t].max())

    def fast(self, i: int, t: int):
        """dfs_fast_prefetch's decision (a group's first leaf always takes the general path)."""
        n, mp, mo = self.transition(i, t)
        return i != self.group_of(i)[0] and n <= FAST_NODES and mp <= FAST_EDITS and mo <= FAST_EDITS

    def rebuilds(self):
        """(leaf, tile) rows k_replay_dfs rebuilds: from the first leaf of a group whose stacks
        would overflow in the tile, every later leaf of the group."""
        total = 0
        for g in self.groups:
            gc = self.group_prefix(g)
            for t in range(self.tiles):
                for i in range(*g):
                    p, o = self.path_counts(self.dfs_order[i], t, gc)
                    if p > DFS_PCAP or o > DFS_OCAP:
                        total += g[1] - i
                        break
        return total


def direct_fasta(pm: PanMAT, aligned: bool, census: Census | None = None) -> str:
    """Replay without any of the kernels' structure: the consensus with gap slots as '-', the
    deepest edit on the path wins, 'x' dropped, '-' dropped when unaligned, wrapped at 70.
    Only for inputs whose blocks are all present, forward and unrotated."""
    c = census or Census(pm)
    out = []
    for v in sorted(c.leaves, key=lambda v: pm.names[v]):
        row = bytearray(c.lay.cons)
        for u in c.paths[v]:
            for col, ch in c.node_edits[u].items():
                row[col] = ord(ch)
        s = row.replace(b"x", b"")
        if not aligned:
            s = s.replace(b"-", b"")
        s = s.decode()
        out.append(">" + pm.names[v] + "\n" + "".join(s[k:k + 70] + "\n" for k in range(0, len(s) - len(s) % 70, 70))
                   + s[len(s) - len(s) % 70:] + "\n")
    return "".join(out)


def records(text: str):
    return sorted(">" + r for r in text.split(">")[1:])


# ---------------------------------------------------------------------------- cases
@dataclass
class Case:
    build: object                       # () -> PanMAT
    check: object                       # (Census, PanMAT) -> None: the edge the input sits on
    depth: int                          # replay.max_depth
    dfs: bool                           # k_replay_dfs (else k_replay)
    groups: int | None = None           # replay.dfs_groups, when the case pins it
    rebuild: bool | None = None         # replay.dfs_rebuilds > 0 / == 0 (depth-first kernel)
    reroot: list = field(default_factory=list)   # leaf names to reroot at (restore cases)
    plain: bool = True                  # every block present, no rotation / inversion / offset


CASES: dict[str, Case] = {}


def that(pred):
    def check(c, pm):
        assert pred(c, pm)
    return check


def case(name, **kw):
    def reg(fn):
        CASES[name] = Case(build=fn, **kw)
        return fn
    return reg


@functools.lru_cache(maxsize=4)
def built(name: str):
    pm = CASES[name].build()
    return pm, Census(pm)


def _spine_of(tree):
    """The deepest leaf of a ladder and its path."""
    paths, _ = paths_of(tree[1], tree[2], tree[3])
    deep = max(paths, key=lambda v: (len(paths[v]), -v))
    return deep, paths[deep], paths


def _plant_positions(pm, lay, path, positions, base, shared, mnp_at):
    """On each named path position: a column only it edits, the column `shared` all of them
    edit (each but the first overriding, the deepest wins) and an MNP of 6 (overlapping its
    neighbours')."""
    for i, p in enumerate(q for q in positions if q < len(path)):
        v = path[p]
        snp(pm, lay, v, base + i, i)
        snp(pm, lay, v, shared, "CGTA"[i & 3])
        mnp(pm, lay, v, mnp_at + 2 * i, "".join("GTAC"[(i + k) & 3] for k in range(6)))


# ---- A: kernel choice, path positions
def _a_ladder(leaves):
    tree = ladder(leaves)
    pm, lay = new_panmat(tree, [51, 71, 41])
    deep, path, paths = _spine_of(tree)
    _plant_positions(pm, lay, path, [0, 62, 63, 64, 65, 127, 128], 5, 30, 56)
    for k, v in enumerate(sorted(paths)):      # leaves override again
        if k % 3 == 0:
            snp(pm, lay, v, 30, "N")
    return pm


def _a_check(depth, positions):
    def check(c, pm):
        deep, path, _ = _spine_of((pm.names, pm.child_offsets, pm.child_index, pm.root))
        assert len(path) == depth == c.max_depth
        assert c.dfs == (depth <= 128) and c.tile == (4096 if depth <= 128 else 16384)
        here = [p for p in positions if p < depth]
        for t in range(c.tiles):
            for i, p in enumerate(here):    # the shared column: overriding on all but the first
                assert c.node_ovr[path[p], t] >= (1 if i > 0 else 0)
        assert c.path_counts(deep, 0)[1] >= len(here) - 1
        if c.dfs:   # a deep ladder's leaves cannot share a group: one-leaf groups, no stacks
            assert c.groups[0] == (0, 1) and c.group_prefix(c.groups[0]) == depth and c.rebuilds() == 0
    return check


CASES["A_ladder128"] = Case(lambda: _a_ladder(128), _a_check(128, [0, 62, 63, 64, 65, 127, 128]), 128, True, rebuild=False)
CASES["A_ladder129"] = Case(lambda: _a_ladder(129), _a_check(129, [0, 62, 63, 64, 65, 127, 128]), 129, False)


@case("A_ring513", check=_a_check(513, [255, 256, 511, 512]), depth=513, dfs=False)
def _a_ring():
    tree = ladder(513)
    pm, lay = new_panmat(tree, [11001, 11001, 11001])     # 33 003 columns: three tiles
    deep, path, paths = _spine_of(tree)
    for t in range(3):
        c0 = t * REPLAY_TILE
        _plant_positions(pm, lay, path, [255, 256, 511, 512], c0 + 100, c0 + 150, c0 + 200)
    for k, v in enumerate(sorted(paths)):
        if k % 3 == 0:
            snp(pm, lay, v, 150, "N")
    return pm


def _a_super_check(c, pm):
    deep, path, _ = _spine_of((pm.names, pm.child_offsets, pm.child_index, pm.root))
    chunks = c.chunk_counts(deep, 0)
    assert chunks[1] == (576, 576) and chunks[1][0] > 4 * 128 and chunks[1][1] > 4 * 128   # two super-rounds each
    assert chunks[0] == (9, 0) and chunks[2] == (0, 0) and c.path_counts(deep, 1) == (2, 1)


@case("A_super_rounds", check=_a_super_check, depth=130, dfs=False)
def _a_super():
    tree = ladder(130)
    pm, lay = new_panmat(tree, [12001, 8001])       # 20 002 columns: two tiles
    deep, path, _ = _spine_of(tree)
    for k in range(9):                               # the columns' first editor above the chunk
        snp(pm, lay, path[0], 20 * k, "T")
    for i, p in enumerate(range(64, 128)):           # one whole chunk: 9 plain + 9 overriding each
        for k in range(9):
            snp(pm, lay, path[p], 1000 + 9 * i + k, i + k)
            snp(pm, lay, path[p], 20 * k, "ACGT"[(i + k) & 3])
    snp(pm, lay, path[3], 17000, "G")
    snp(pm, lay, path[100], 17000, "A")
    snp(pm, lay, path[100], 17001, "A")
    return pm


# ---- B: tile, group and row-end edges
def _b_build(leaves, tile, width):
    """Blocks: one that straddles the first tile boundary and ends on a tile boundary, one from
    there to the end (straddling the last boundary).  Single edits at c0 - 1 and c0 and an MNP
    over c0 - 3 .. c0 + 2 at the first and the last tile boundary (for k_replay the last is
    the 8-tile group boundary), high on the spine and again, overriding, lower and at leaves."""
    tree = ladder(leaves)
    stride = (width + 15) // 16 * 16
    tiles = (stride + tile - 1) // tile
    widths = [width] if tiles == 1 or width <= 2 * tile else [2 * tile, width - 2 * tile]
    pm, lay = new_panmat(tree, widths)
    deep, path, paths = _spine_of(tree)
    top, low = path[1], path[len(path) - 4]
    leaf_a, leaf_b = path[-1], sorted(paths)[len(paths) // 2]
    bounds = sorted({b for b in (tile, (tiles - 1) * tile, min(tiles - 1, REPLAY_GROUP) * tile) if 3 <= b < width - 3})
    for k, (v, s) in enumerate([(top, "ACGTAC"), (low, "CATGCA"), (leaf_a, "GGNRYK"), (leaf_b, "TTACGM")]):
        for c0 in bounds:
            if lay.locate(c0 - 3)[0] == lay.locate(c0 + 2)[0]:
                mnp(pm, lay, v, c0 - 3, s)
                snp(pm, lay, v, c0 - 1, s[k % 4])
                snp(pm, lay, v, c0, s[(k + 1) % 4])
        if len(widths) == 2:      # the block boundary on a tile boundary: last base, first base
            snp(pm, lay, v, 2 * tile - 2, s[0])
            snp(pm, lay, v, 2 * tile, s[1])
        snp(pm, lay, v, 0, s[2])
        snp(pm, lay, v, width - 2, s[3])
    return pm


def _b_check(tile, width, depth):
    def check(c, pm):
        assert (c.columns, c.tile, c.max_depth) == (width, tile, depth)
        assert c.stride - c.columns == (-width) % 16
        tiles = -(-c.stride // tile)
        assert c.tiles == tiles
        deep = _spine_of((pm.names, pm.child_offsets, pm.child_index, pm.root))[0]
        if tiles > 1 and width > 2 * tile:
            assert c.lay.col_start[1] == 2 * tile                        # block boundary == tile boundary
            assert c.tile_blocks[0] == [0] and c.tile_blocks[1] == [0] and c.tile_blocks[-1] == [1]
            for t in (0, 1, tiles - 2, tiles - 1):                       # 3 + 3 columns of each MNP, overridden below
                p, o = c.path_counts(deep, t)
                assert p >= 3 and o >= 3, (t, p, o)
            if c.stride % tile:
                assert 0 < c.stride - (tiles - 1) * tile < tile          # a final tile narrower than a tile
        if not c.dfs and width > REPLAY_GROUP * tile:
            assert tiles == REPLAY_GROUP + 1                              # a second workgroup per leaf
    return check


for _w in (4096, 12304, 12305, 12303):     # one tile exactly; three tiles + a 16 / 32 / 16 wide one
    CASES[f"B_dfs_{_w}"] = Case(functools.partial(_b_build, 20, DFS_TILE, _w), _b_check(DFS_TILE, _w, 20), 20, True,
                                rebuild=False)
for _w in (16384, 131072, 135008, 135009, 135007):   # one tile, one 8-tile group, a ninth narrow tile
    CASES[f"B_replay_{_w}"] = Case(functools.partial(_b_build, 130, REPLAY_TILE, _w), _b_check(REPLAY_TILE, _w, 130),
                                   130, False)


# ---- C: absent-block restore
_C_LAYOUT = [  # (width, role): blocks of the k_replay restore input, in id order
    (35, "p"), (5, "a"),          # [35, 40): inside one 16-byte unit
    (7, "p"), (53, "a"),          # [47, 100): starts at column = 15 (mod 16)
    (100, "p"), (57, "a"),        # [200, 257): ends at column = 1 (mod 16)
    (743, "p"), (1000, "a"),      # [1000, 2000)
    (1000, "p"), (10, "x"),       # [3000, 3010): the seventh absent block of the sibling input
    (1990, "p"), (16, "a"),       # [5000, 5016): whole 16-byte units
    (11364, "p"), (20, "a"),      # [16380, 16400): straddles the tile boundary
    (600, "p"),
]


def _c_replay(seven: bool, wide: bool):
    tree = ladder(130)
    layout = list(_C_LAYOUT)
    if wide:   # ... and a block that straddles the 8-tile group boundary at column 131 072 (a deep
        tree = stem_ladder(118, 12)   # path with few leaves: reroot works through every leaf's row)
        layout += [(131060 - 17000, "p"), (30, "a"), (400, "p")]
    pm, lay = new_panmat(tree, [w for w, _ in layout])
    deep, path, paths = _spine_of(tree)
    leaves = sorted(paths, key=lambda v: -len(paths[v]))
    victim = leaves[7]
    absent = [b for b, (_, r) in enumerate(layout) if r == "a" or (r == "x" and seven)]
    for b in absent:
        pm.add_block_mut(victim, b, False, False)
    pm.add_block_mut(leaves[0], 3, False, False)
    pm.add_block_mut(leaves[0], 13, False, False)
    pm.add_block_mut(leaves[min(40, len(leaves) - 1)], 5, False, False)
    # the victim's ancestors edit inside (first, last base) and just outside every such block
    anc = paths[victim][:-1]
    for k, (b, (w, r)) in enumerate(enumerate(layout)):
        if r == "p":
            continue
        lo = lay.col_start[b]
        for j, col in enumerate([lo, lo + w - 2, lo - 2, lo + w]):
            snp(pm, lay, anc[(3 * k + j) % len(anc)], col, "ACGT"[(k + j) & 3])
            snp(pm, lay, anc[-1 - (k + j) % 5], col, "TGCA"[(k + j) & 3])
        if w >= 20:
            mnp(pm, lay, anc[5 + k], lo + 6, "NNRYKM")
    return pm


def _c_replay_check(n, wide):
    def check(c, pm):
        paths = c.paths
        victim = sorted(paths, key=lambda v: -len(paths[v]))[7]
        assert c.tile == REPLAY_TILE and len(c.absent(victim, 0)) == n == len(c.absent(victim, 0, real=False))
        assert max(len(c.absent(v, t)) for v in c.leaves for t in range(c.tiles)) == n
        assert len(c.absent(victim, 1)) == 1 and 13 in c.absent(victim, 0) and 13 in c.absent(victim, 1)
        lay = c.lay
        assert (lay.col_start[1] // 16 == (lay.col_start[1] + lay.width[1] - 1) // 16
                and lay.col_start[3] % 16 == 15 and (lay.col_start[5] + lay.width[5]) % 16 == 1)
        # ancestors edit inside every absent block; none of it may reach the victim's row
        for b in c.absent(victim, 0):
            lo, hi = lay.col_start[b], lay.col_start[b] + lay.width[b]
            assert any(lo <= col < hi for u in paths[victim][:-1] for col in c.node_edits[u]), b
        if wide:
            b = len(_C_LAYOUT) + 1
            assert lay.col_start[b] < REPLAY_GROUP * REPLAY_TILE < lay.col_start[b] + lay.width[b]
            assert b in c.absent(victim, REPLAY_GROUP - 1) and b in c.absent(victim, REPLAY_GROUP)
    return check


def _c_names(pm, which):
    paths, _ = paths_of(pm.child_offsets, pm.child_index, pm.root)
    leaves = sorted(paths, key=lambda v: -len(paths[v]))
    return [pm.names[leaves[k]] for k in which]


CASES["C_replay_6"] = Case(lambda: _c_replay(False, False), _c_replay_check(6, False), 130, False, reroot=[7, 0], plain=False)
CASES["C_replay_7"] = Case(lambda: _c_replay(True, False), _c_replay_check(7, False), 130, False, reroot=[7], plain=False)
CASES["C_replay_group"] = Case(lambda: _c_replay(False, True), _c_replay_check(6, True), 130, False, reroot=[7], plain=False)


def _c_dfs_tree():
    k = Kids()
    a = k.add(0)
    b = k.add(a)
    leaves = [k.add(b), k.add(b), k.add(a), k.add(a), k.add(0)]
    return tree_of(k.kids), a, b, leaves


def _c_dfs(n):
    """68 blocks of 60 columns fill tile 0 up to column 4080, block 68 straddles the tile
    boundary, n - 1 more follow: the last tile overlaps exactly n blocks (ids 68 ..)."""
    tree, a, b, leaves = _c_dfs_tree()
    nblocks = 68 + n
    pm, lay = new_panmat(tree, [60] * nblocks)
    last = nblocks - 1
    sets = [[68, 68 + 62, last, 5], [33, 70, 100, 68 + 31], list(range(68, nblocks)), [], [0, 31, 32, 63, 64, last]]
    for leaf, ids in zip(leaves, sets):
        for bid in sorted(set(ids)):
            pm.add_block_mut(leaf, bid, False, False)
    edited = {x for s in sets[:2] + sets[4:] for x in s} | set(range(68, nblocks, 7))
    for k, bid in enumerate(sorted(edited)):
        lo = lay.col_start[bid]
        for j, (v, col) in enumerate([(0, lo), (a, lo + 58), (b, lo + 30), (a, lo), (b, lo + 58)]):
            snp(pm, lay, v, col, "ACGT"[(k + j) & 3])
    return pm


def _c_dfs_check(n):
    def check(c, pm):
        assert c.dfs and c.tiles == 2 and len(c.groups) == 1
        assert len(c.tile_blocks[1]) == n == len(c.tile_ids[1]) and len(c.tile_ids[0]) == 69
        assert c.tile_blocks[1][0] == 68 and max(c.lay.width) <= 60
        _, a, b, leaves = _c_dfs_tree()
        got = [c.absent(v, 1) for v in leaves]
        assert len({tuple(g) for g in got}) == 5                      # leaves of one group, different sets
        assert got[2] == c.tile_blocks[1] and got[3] == []           # every block of the tile / none
        assert 68 + 62 in got[0] and 68 + n - 1 in got[0]             # table index 62 and the tile's last block
        assert any(bid > 63 for bid in got[1]) and any(31 < bid <= 63 for bid in c.absent(leaves[4], 0))
        for v in leaves[:3]:
            for bid in c.absent(v, 1)[:1]:
                lo = c.lay.col_start[bid]
                assert any(lo <= col < lo + 60 for u in c.paths[v][:-1] for col in c.node_edits[u])
    return check


for _n in (63, 64, 65):
    CASES[f"C_dfs_{_n}"] = Case(functools.partial(_c_dfs, _n), _c_dfs_check(_n), 4, True, groups=1, rebuild=False,
                                reroot=[0, 2], plain=False)


# The reference indexes vectors of blocks.size() + 1 entries by block id (src/fasta.cpp:2001-2012),
# so the ids of B blocks lie in [0, B]: one hole is the most a PanMAT it can replay has ("hole":
# M = B + 1 > B, id 1 is no block).  "wide" ({0, 3, 4, 40, 41}) is outside that: the oracle
# refuses it and the engine is not compared on it.  FASTA only: reroot refuses any hole ("Block
# with id 1 -1 not found!", src/reroot.cpp; the oracle and pm_reroot say the same).
_SPARSE = {"hole": ([0, 2, 3, 4, 5], [40, 33, 17, 64, 50])}


def _c_sparse(stem, which):
    """Block ids with holes: ids that are no block sit between the blocks (M > B)."""
    ids, widths = _SPARSE[which]
    k = Kids()
    top = k.chain(0, stem)[-1] if stem else 0
    a = k.add(top)
    leaves = [k.add(a), k.add(a), k.add(top), k.add(top)]
    pm, lay = new_panmat(tree_of(k.kids), widths, ids=ids)
    for leaf, gone in zip(leaves, [[1, 3], [len(ids) - 1], [0, 2], []]):
        for j in gone:
            pm.add_block_mut(leaf, ids[j], False, False)
    for j, bid in enumerate(ids):
        lo = lay.col_start[bid]
        snp(pm, lay, top, lo, "ACGT"[j & 3])
        snp(pm, lay, a, lo, "CGTA"[j & 3])
        snp(pm, lay, a, lo + lay.width[bid] - 2, "G")
        snp(pm, lay, 0, lo + 5, "T")
    return pm


def _c_sparse_check(which):
    def check(c, pm):
        ids, widths = _SPARSE[which]
        assert c.lay.M == ids[-1] + 1 > len(ids) == len(c.lay.ids) and c.columns == sum(widths)
        assert len(c.tile_ids[0]) == c.lay.M and c.tile_blocks[0] == ids      # the tables hold the ids in between too
        assert sorted(len(c.absent(v, 0)) for v in c.leaves) == [0, 1, 2, 2]
        assert all(len(c.absent(v, 0, real=False)) == len(c.absent(v, 0)) + 1 for v in c.leaves)   # ... as absent
    return check


for _which in _SPARSE:
    _rr = []
    CASES[f"C_sparse_{_which}_dfs"] = Case(functools.partial(_c_sparse, 0, _which), _c_sparse_check(_which), 3, True,
                                           groups=1, rebuild=False, reroot=_rr, plain=False)
    CASES[f"C_sparse_{_which}_replay"] = Case(functools.partial(_c_sparse, 130, _which), _c_sparse_check(_which), 133,
                                              False, reroot=_rr, plain=False)


# ---- D: override and undo-stack capacities
def _d_ovr(extra):
    tree = ladder(130)
    pm, lay = new_panmat(tree, [17001, 3001])
    deep, path, _ = _spine_of(tree)
    for p in range(129):            # 129 spine nodes rewrite the same 8 columns: 128 x 8 overriding
        for k in range(8):
            snp(pm, lay, path[p], 64 * k + 3, "ACGT"[(p + k) & 3])
    if extra:
        snp(pm, lay, path[129], 3, "N")
    for p in range(5):               # the next tile starts its own count
        snp(pm, lay, path[p], 16500, "ACGT"[p & 3])
    return pm


def _d_ovr_check(n):
    def check(c, pm):
        deep = _spine_of((pm.names, pm.child_offsets, pm.child_index, pm.root))[0]
        assert c.path_counts(deep, 0) == (8, n) and c.path_counts(deep, 1) == (1, 4)
        assert c.max_leaf_tile()[1] == n and (n > OVR_CAP) == (n == 1025)
    return check


CASES["D_ovr_1024"] = Case(lambda: _d_ovr(False), _d_ovr_check(1024), 130, False)
CASES["D_ovr_1025"] = Case(lambda: _d_ovr(True), _d_ovr_check(1025), 130, False)


def _d_tree(two_leaf):
    """root -> a -> chain of 8 -> leaf A, then B under a, then d -> (C, D) under a, then Z
    under the root (two_leaf: root -> chain of 8 -> A, and Z)."""
    k = Kids()
    if two_leaf:
        ch = k.chain(0, 8)
        la = k.add(ch[-1])
        z = k.add(0)
        return tree_of(k.kids), ch, la, [z], []
    a = k.add(0)
    ch = k.chain(a, 8)
    la = k.add(ch[-1])
    lb = k.add(a)
    d = k.add(a)
    rest = [lb, k.add(d), k.add(d), k.add(0)]
    return tree_of(k.kids), ch, la, rest, [d]


def _d_stack(kind, n, two_leaf=False):
    tree, ch, la, rest, inner = _d_tree(two_leaf)
    pm, lay = new_panmat(tree, [4001, 2001])
    if kind == "plain":     # 8 x 48 = 384 plain edits below the shared prefix, then the leaf's
        for i, v in enumerate(ch):
            for k in range(48):
                snp(pm, lay, v, 10 + 48 * i + k, i + k)
        if n == 385:
            snp(pm, lay, la, 3000, "N")
    else:                   # the root edits 64 columns (shared prefix: no push), the chain re-edits them
        for k in range(64):
            snp(pm, lay, 0, 10 + 3 * k, "T")
        for i, v in enumerate(ch):
            for k in range(8):
                snp(pm, lay, v, 10 + 3 * (8 * i + k), "ACG"[(i + k) % 3])
        if n == 65:
            snp(pm, lay, la, 10, "N")
    for j, v in enumerate(rest + inner):     # the later leaves rebuild too; a tile that never overflows
        snp(pm, lay, v, 20 + 3 * j, "G")     # (overrides the root's or a chain column's neighbour)
        snp(pm, lay, v, 3500 + j, "C")
        snp(pm, lay, v, 4200 + j, "A")
    snp(pm, lay, ch[2], 4200, "T")
    snp(pm, lay, la, 4300, "T")
    return pm


def _d_stack_check(kind, n, two_leaf):
    def check(c, pm):
        assert len(c.groups) == 1 and len(c.leaves) <= 16 and c.group_nodes(c.groups[0]) <= 128
        assert c.group_prefix(c.groups[0]) == 1                          # only the root is never undone
        p, o = c.stack_counts(0, 0)
        assert (p if kind == "plain" else o) == n
        over = n > (DFS_PCAP if kind == "plain" else DFS_OCAP)
        assert (p > DFS_PCAP or o > DFS_OCAP) == over
        assert c.rebuilds() == (len(c.leaves) if over else 0)            # tile 0 only; tile 1 never overflows
        assert max(c.stack_counts(i, 1) for i in range(len(c.leaves))) <= (4, 4)
    return check


for _kind, _lo in (("plain", 384), ("ovr", 64)):
    for _n in (_lo, _lo + 1):
        CASES[f"D_{_kind}_{_n}"] = Case(functools.partial(_d_stack, _kind, _n), _d_stack_check(_kind, _n, False), 11, True,
                                        groups=1, rebuild=_n > _lo)
    CASES[f"D_{_kind}_{_lo + 1}_two_leaf"] = Case(functools.partial(_d_stack, _kind, _lo + 1, True),
                                                  _d_stack_check(_kind, _lo + 1, True), 10, True, groups=1, rebuild=True)


def _d_one_leaf_check(c, pm):
    assert len(c.leaves) == 1 and c.groups == [(0, 1)] and c.group_prefix((0, 1)) == 3
    assert c.path_counts(c.leaves[0], 0) == (500, 105) and c.stack_counts(0, 0) == (0, 0) and c.rebuilds() == 0


@case("D_one_leaf_group", check=_d_one_leaf_check, depth=3, dfs=True, groups=1, rebuild=False)
def _d_one_leaf():
    """The whole path is the group's shared prefix: applied without pushes, however many edits."""
    k = Kids()
    leaf = k.add(k.add(0))
    pm, lay = new_panmat(tree_of(k.kids), [3001])
    for j in range(500):
        snp(pm, lay, (0, 1)[j & 1], 5 * j, "ACGT"[j & 3])
    for j in range(70):
        snp(pm, lay, 1 + (j & 1), 5 * (2 * j), "TGCA"[j & 3])
        snp(pm, lay, leaf, 5 * (2 * j), "N")
    return pm


def _d_undo_tree():
    k = Kids()
    a = k.add(0)
    l0 = k.add(a)        # the group's first leaf (always the general path); leaf 1 then enters 4 nodes
    b = k.add(a)
    cc = k.add(b)
    p1 = k.add(cc)
    l1 = k.add(p1)
    leaves = [l0, l1, k.add(cc), k.add(b), k.add(a), k.add(0)]
    return tree_of(k.kids), [a, b, cc, p1], leaves


def _d_undo(general):
    """a sets X to C; b, c, leaf 1's private node and leaf 1 override X again and each edits a
    fresh column; the sibling subtrees that follow must see the overrides popped deepest first.
    general: 17 plain edits on the private node and on leaf 3, so both take dfs_apply."""
    tree, (a, b, cc, p1), leaves = _d_undo_tree()
    pm, lay = new_panmat(tree, [301, 5001])
    for X in (40, 4500):             # both tiles
        for v, ch in ((a, "C"), (b, "G"), (cc, "T"), (p1, "A"), (leaves[1], "N")):
            snp(pm, lay, v, X, ch)
        for j, v in enumerate((b, cc, p1, leaves[1], leaves[2])):
            snp(pm, lay, v, X + 10 + j, j)
    if general:
        for j in range(17):
            snp(pm, lay, p1, 100 + j, j)
            snp(pm, lay, leaves[3], 100 + j, j + 1)
    return pm


def _d_undo_check(general):
    def check(c, pm):
        _, (a, b, cc, p1), leaves = _d_undo_tree()
        assert c.dfs_order == leaves and len(c.groups) == 1 and c.dfs_lp == [0, 2, 4, 3, 2, 1]
        assert [40 in c.override[v] for v in (a, b, cc, p1, leaves[1])] == [False, True, True, True, True]
        assert c.stack_counts(1, 0) == (5 + 17 * general, 4) and c.rebuilds() == 0   # three nested frames + the leaf's
        assert c.transition(1, 0)[0] == 4
        assert [c.fast(i, 0) for i in range(6)] == [False, not general, True, not general, True, True]
        text = dict(r.split("\n", 1) for r in records(direct_fasta(pm, True, c)))
        row = {v: text[">" + pm.names[v]].replace("\n", "") for v in leaves}
        cons = c.lay.cons.decode()
        # (block 0: columns are row positions up to its sentinel at column 300)
        assert [row[v][40] for v in leaves] == ["C", "N", "T", "G", "C", cons[40]]
        y = [other(c.lay, 50 + j, j) for j in range(5)]      # the fresh columns of b, c, the private node, leaves 1, 2
        assert row[leaves[1]][50:55] == "".join(y[:4]) + cons[54] and row[leaves[2]][50:55] == y[0] + y[1] + cons[52:54] + y[4]
        assert row[leaves[3]][50:55] == y[0] + cons[51:55]
        assert row[leaves[4]][50:55] == cons[50:55]
    return check


CASES["D_undo_fast"] = Case(lambda: _d_undo(False), _d_undo_check(False), 6, True, groups=1, rebuild=False)
CASES["D_undo_general"] = Case(lambda: _d_undo(True), _d_undo_check(True), 6, True, groups=1, rebuild=False)


# ---- E: fast-transition thresholds
_E_CHAINS = [2, 1, 4, 5, 4, 1, 4, 5, 1]     # entering nodes per leaf (the first leaf: general anyway)


def _e_tree():
    k = Kids()
    h = k.add(0)
    chains = [k.chain(h, n) for n in _E_CHAINS]
    return tree_of(k.kids), h, chains


def _e_build(kind, n, spread=False):
    tree, h, chains = _e_tree()
    pm, lay = new_panmat(tree, [3001, 3001])
    for k in range(17):
        snp(pm, lay, h, 10 + 2 * k, "T")
    target = chains[4][1]           # in the 4-node transition that follows a 5-node (general) one
    for k in range(n):
        col = (10 + 2 * k) if kind == "ovr" else (500 + k)
        if spread and k >= 9:
            col += DFS_TILE
        snp(pm, lay, target, col, "ACG"[k % 3] if kind == "ovr" else k)
    if spread and kind == "ovr":
        for k in range(9, 17):
            snp(pm, lay, 0, 10 + 2 * k + DFS_TILE, "T")
    for i, ch in enumerate(chains):  # every node: a column of its own and an override of h's
        for j, v in enumerate(ch):
            snp(pm, lay, v, 1000 + 10 * i + j, i + j)
            snp(pm, lay, v, 4200 + 10 * i + j, i + j + 1)
            if v != target and (i + j) % 2 == 0:
                snp(pm, lay, v, 10 + 2 * ((i + j) % 17), "ACG"[(i + j) % 3])
    return pm


def _e_check(kind, n, spread):
    def check(c, pm):
        assert len(c.groups) == 1 and c.group_nodes((0, 9)) == 2 + sum(_E_CHAINS) and c.rebuilds() == 0
        tr = [c.transition(i, 0) for i in range(9)]
        assert [t[0] for t in tr] == [2 + _E_CHAINS[0]] + _E_CHAINS[1:]     # entering 1, 4 and 5 nodes
        assert all(t[1] <= 2 and t[2] <= 1 for i, t in enumerate(tr) if i not in (0, 4))
        here = 9 if spread else n
        most = here + 1 if kind == "plain" else here     # (the node's own column is plain as well)
        assert tr[4] == ((4, most, 1) if kind == "plain" else (4, 1, most)), tr[4]
        fast4 = most <= FAST_EDITS
        # fast after general (leaf 4 after 3 when it fits, 5 after 3/4), general after fast (3 after 2, 7 after 6)
        assert [c.fast(i, 0) for i in range(9)] == [False, True, True, False, fast4, True, True, False, True]
        assert c.fast(4, 1)       # the same transition is fast in the next tile
        if spread:   # 17 edits on the node, but at most 10 in one tile: fast in both
            t1 = c.transition(4, 1)
            assert (t1[1] if kind == "plain" else t1[2]) >= 8 and n == 17 and fast4
    return check


for _kind in ("plain", "ovr"):
    for _n in (16, 17):
        # a plain count of n on the node next to its own column: n - 1 planted + 1
        CASES[f"E_{_kind}_{_n}"] = Case(functools.partial(_e_build, _kind, _n - (1 if _kind == "plain" else 0)),
                                        _e_check(_kind, _n - (1 if _kind == "plain" else 0), False), 7, True, groups=1,
                                        rebuild=False)
    CASES[f"E_{_kind}_17_two_tiles"] = Case(functools.partial(_e_build, _kind, 17, True), _e_check(_kind, 17, True), 7, True,
                                            groups=1, rebuild=False)


# ---- F: formatter
def star(leaves: int):
    return tree_of([list(range(1, leaves + 1))] + [[] for _ in range(leaves)])


_F_LENGTHS = [0, 1, 69, 70, 71, 139, 140, 141]


def _f_lengths():
    """One block of 141 bases; leaf k keeps the first _F_LENGTHS[k] of them (the rest deleted:
    dropped unaligned, dashes aligned); a ninth leaf has the block absent."""
    pm, lay = new_panmat(star(9), [142])
    for k, n in enumerate(_F_LENGTHS):
        col = n
        while col < 141:
            step = min(6, 141 - col)
            delete(pm, lay, 1 + k, col, step)
            col += step
        if n:
            snp(pm, lay, 1 + k, n - 1, "N")
    pm.add_block_mut(9, 0, False, False)
    return pm


def _f_lengths_check(c, pm):
    for aligned in (True, False):
        recs = dict(r.split("\n", 1) for r in records(direct_fasta(pm, aligned, c)))
        got = [len(recs[">" + pm.names[1 + k]].replace("\n", "")) for k in range(8)]
        assert got == ([141] * 8 if aligned else _F_LENGTHS)


CASES["F_lengths"] = Case(_f_lengths, _f_lengths_check, 2, True, groups=1, plain=False)


def _f_block_len(n):
    pm, lay = new_panmat(star(3), [n + 1])
    if n:
        snp(pm, lay, 2, n - 1, "N")
        snp(pm, lay, 3, 0, "R")
    return pm


for _n in _F_LENGTHS:
    CASES[f"F_block_{_n}"] = Case(functools.partial(_f_block_len, _n),
                                  that(lambda c, pm, n=_n: (c.columns, c.stride) == (n + 1, (n + 16) // 16 * 16)),
                                  2, True, groups=1)


@case("F_all_absent", check=that(lambda c, pm: [len(c.present[v]) for v in c.leaves] == [0, 3, 2]), depth=2, dfs=True,
      groups=1, plain=False)
def _f_all_absent():
    pm, lay = new_panmat(star(3), [30, 75, 12])
    for b in range(3):
        pm.add_block_mut(1, b, False, False)
    pm.add_block_mut(3, 1, False, False)
    snp(pm, lay, 0, 3, "G")
    snp(pm, lay, 0, 40, "G")
    return pm


def _f_circular(L):
    pm, lay = new_panmat(star(6), [L + 1])
    for k, o in enumerate([0, 1, L - 1, L, L + 1]):
        pm.circular[1 + k] = o
        snp(pm, lay, 1 + k, k, "N")
    return pm


for _L in (70, 71):
    CASES[f"F_circular_{_L}"] = Case(functools.partial(_f_circular, _L),
                                     that(lambda c, pm, L=_L: c.columns == L + 1 and list(pm.circular[1:6]) == [0, 1, L - 1, L, L + 1]),
                                     2, True, groups=1, plain=False)


def _f_rotation(absent):
    """Six blocks; every leaf rotates to one of {0, 1, existing - 1, existing, existing + 3},
    half of them inverted as well; `absent`: block 2 deleted and block 4 never inserted at the
    rotating leaves (the aligned dash runs are then indexed by print position)."""
    rots = lambda ex: [0, 1, ex - 1, ex, ex + 3]
    names, off, idx, root = star(10)
    pm = PanMAT(names, off, idx, root)
    widths = [13, 29, 71, 8, 40, 17]
    for b, w in enumerate(widths):
        pm.add_block(b, block_text(b, w - 1))
        if not (absent and b == 4):
            pm.add_block_mut(root, b, True, b == 3)        # block 3 on the reverse strand
    lay = Layout(pm)
    ex = 4 if absent else 6
    for k in range(10):
        v = 1 + k
        if absent:
            pm.add_block_mut(v, 2, False, False)
        pm.rotation[v] = rots(ex)[k % 5]
        pm.inverted[v] = k // 5
        snp(pm, lay, v, lay.col_start[k % 6 if not absent or k % 6 not in (2, 4) else 0] + 1, "N")
    return pm


def _f_rotation_check(absent):
    def check(c, pm):
        ex = 4 if absent else 6
        assert all(len(c.present[v]) == ex for v in c.leaves)
        assert sorted(set(int(r) for r in pm.rotation[1:])) == sorted({0, 1, ex - 1, ex, ex + 3})
        assert list(pm.inverted[1:]) == [0] * 5 + [1] * 5
    return check


CASES["F_rotation"] = Case(lambda: _f_rotation(False), _f_rotation_check(False), 2, True, groups=1, plain=False)
CASES["F_rotation_absent"] = Case(lambda: _f_rotation(True), _f_rotation_check(True), 2, True, groups=1, plain=False)

_IUPAC = "ACMGRSVTWYHKDBN"


def _f_inverted(width):
    """One reverse-strand block of `width` columns holding every IUPAC letter, with '-' runs
    (gap slots nobody fills, type-1 and type-5 deletions) at columns 0, 63, 64, 255 and 256."""
    names, off, idx, root = star(4)
    pm = PanMAT(names, off, idx, root)
    n = width - 1 - 3
    pm.add_block(0, "".join(_IUPAC[(j * 7 + j // 15) % 15] for j in range(n)))
    pm.add_gaps(0, [(0, 3)])                                # columns 0 .. 2
    pm.add_block_mut(root, 0, True, True)
    lay = Layout(pm)
    for v, col, k in ((0, 61, 5), (0, 250, 6), (2, 256, 1), (2, width - 2, 1)):   # 61 .. 65, 250 .. 255, 256, the last base
        if col + k <= width - 1:
            delete(pm, lay, v, col, k)
    snp(pm, lay, 2, 1, "G")                                  # a gap slot filled at one leaf
    pm.add_block_mut(3, 0, False, True)                      # back to the forward strand
    snp(pm, lay, 4, 64, "N")
    return pm


def _f_inverted_check(width):
    def check(c, pm):
        assert c.columns == width and set(_IUPAC) <= set(c.lay.cons.decode())
        row = bytearray(c.lay.cons)
        for col, ch in c.node_edits[0].items():
            row[col] = ord(ch)
        dash = {k for k in range(width) if row[k:k + 1] == b"-"}
        assert {0, 1, 2, 63, 64} <= dash and (width <= 256 or 255 in dash)
    return check


for _w in (255, 256, 257, 512, 513):
    CASES[f"F_inverted_{_w}"] = Case(functools.partial(_f_inverted, _w), _f_inverted_check(_w), 2, True, groups=1, plain=False)


@case("F_70000_leaves", check=that(lambda c, pm: len(c.leaves) == 70000 > 65535 and len(c.groups) == 4375), depth=2,
      dfs=True, groups=4375, rebuild=False)
def _f_many():
    """More leaves than a grid's y dimension holds on many runtimes (65 535)."""
    pm, lay = new_panmat(star(70000), [21])
    for v in range(1, 70001, 7):
        snp(pm, lay, v, v % 20, "ACGT"[v & 3])
    return pm
