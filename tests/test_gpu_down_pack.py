"""PM_OPT_DOWN_PACK: a pre-order level's nodes in groups of G per wave, a group's live (node, word)
pairs gathered into full waves (k_down<.., G>, down_packed), give exactly the records, per-site
scores and root codes of one wave per (node, tile) -- and of the oracle -- at the group edges
(levels of G - 1, G, G + 1 and 1 nodes), for every kind of first and second child, under unary,
polytomy and root parents, at the tile edges and at both extremes of lane density (every lane
live: G rounds and mid-wave stage flushes; no lane live: the wave leaves).  The launches it does
not take (absent leaves, Sankoff, PM_OPT_SUB_DOWN, grouped levels, bands, the root's level) run
the kernels they ran before.  Every case reads what it ran with off phase_report().

The module runs with level groups, bands and sweeps off (set_group(0), set_narrow(0),
set_cluster(0)) unless a case says otherwise: each of these tiny trees' levels is then a launch
of its own, which -1 packs."""
import functools

import numpy as np
import pytest

import _shapes
import panman_amd
from _trees import names_for
from panman_amd._lib import phase_report, phase_reset

pytestmark = pytest.mark.gpu

FITCH, SANKOFF = panman_amd.MODE_FITCH, panman_amd.MODE_SANKOFF
PACK_DEFAULT = 1          # the library's default: on from kDownPackMinWaves (node, tile) waves a level
ALWAYS = -1               # on at any size: these trees are far below the threshold
G = 8                     # kDownPack
GROUP_OF = {0: 0, ALWAYS: G}   # the group size a run reports


def _plain(e):
    """One launch per pre-order level: no level groups, no bands, no sweeps (at the next upload)."""
    e.set_group(0)
    e.set_narrow(0)
    e.set_cluster(0)


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)   # (a context of this module's own: its options die with it)
    _plain(e)
    yield e
    e.close()


def _run(engine, pack, mode=FITCH, expect=None):
    """One run with PM_OPT_DOWN_PACK = pack; (records, score, root codes), and the number of packed
    launches.  expect: the group size the run must report (default: by the option)."""
    engine.set_down_pack(pack)
    phase_reset()
    engine.run(mode)
    ph = dict(phase_report())
    want = GROUP_OF[pack] if expect is None else expect
    if mode == FITCH:
        assert ph["run.down_pack"] == want, ph
        assert (ph["run.down_pack_launches"] > 0) == (want > 0), ph
    else:
        assert "run.down_pack" not in ph, ph   # Sankoff's launch sequence has no packed levels
    got = engine.mutations()
    score, rootc = engine.site_results()
    return (got, score, rootc), int(ph.get("run.down_pack_launches", 0))


def _equal(a, b):
    assert a[0].shape == b[0].shape, (a[0].shape, b[0].shape)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all()


def _same_as_oracle(res, want, root, sites):
    got, score, rootc = res
    recs, want_root = want
    assert got.shape == recs.shape, (got.shape, recs.shape)
    assert (got == recs).all()
    assert (rootc == want_root).all()
    nonroot = recs[recs[:, 0] != root]
    assert (score == np.bincount(nonroot[:, 1], minlength=sites)).all()


def _upload(engine, inp, node_row=None):
    off, idx, root, codes, cons, forced = inp
    engine.tree_upload(off, idx, root)
    engine.leaves_upload(codes, _shapes.leaf_rows(off) if node_row is None else node_row)
    engine.sites_upload(cons, forced)


def _oracle(oracle, inp, mode=FITCH, node_row=None):
    off, idx, root, codes, cons, forced = inp
    rows = _shapes.leaf_rows(off) if node_row is None else node_row
    _, recs, rootc = oracle.csr_columns(off, idx, root, names_for(off), codes, rows, cons, forced,
                                        algo=mode, threads=8, with_root=True)
    return recs, rootc


def _m3(b):
    """The smallest node that is always materialised: three leaves (never evaluated inline)."""
    return b.node([b.leaf(), b.leaf(), b.leaf()])


LEVEL_NODES = (1, G - 1, G, G + 1)   # materialised nodes at depths 1 .. 4 of level_tree()


@functools.lru_cache(maxsize=None)
def level_tree():
    """Levels of 1, G - 1, G and G + 1 materialised nodes below the root: fewer items than G, a
    ragged group, one full group, a full group and a group of one.  The G - 1 nodes hang under a
    polytomy."""
    b = _shapes._Builder()
    pairs = [b.node([_m3(b), _m3(b)]) for _ in range(4)]           # depth 3; their 8 children at depth 4
    one = b.node([_m3(b), b.cherry()])                             # depth 3; a ninth node at depth 4
    depth2 = [b.node([pairs[k], one if k == 0 else _m3(b)]) for k in range(4)]   # their 8 children at depth 3
    depth2 += [_m3(b) for _ in range(G - 1 - 4)]
    top = b.node(depth2)                                           # depth 1, G - 1 children
    return b.csr(b.node([top, b.leaf()]))


@functools.lru_cache(maxsize=None)
def kinds_tree():
    """One level (under a polytomy) whose nodes' first two children are, between them, a leaf, a
    leaf-parent of one leaf, a leaf-parent of two and a materialised child; a unary node; a node
    whose third and later children are tail items; nodes whose S2 / S3 children leave the
    descriptor (one keeping a materialised child, one keeping none)."""
    b = _shapes._Builder()
    nodes = [
        b.node([b.leaf(), b.kind("single"), b.leaf()]),
        b.node([b.cherry(), _m3(b)]),
        b.node([b.cherry(), b.kind("single"), b.leaf()]),
        b.node([_m3(b)]),
        b.node([_m3(b), b.leaf(), b.leaf(), b.cherry()]),
        _m3(b),
        b.node([b.kind("s2"), _m3(b)]),
        b.node([b.kind("s2"), b.kind("s3")]),
        b.node([b.kind("rec", 1), b.leaf()]),
    ]
    return b.csr(b.node([b.node(nodes), b.cherry()]))


@functools.lru_cache(maxsize=None)
def root_tree():
    """The root's children are level items: their parent's final comes from root_final."""
    b = _shapes._Builder()
    x = b.node([b.cherry(), _m3(b)])
    y = b.node([b.leaf(), b.kind("single"), b.leaf()])
    return b.csr(b.node([x, y]))


TREES = {"levels": level_tree, "kinds": kinds_tree, "root": root_tree}


@functools.lru_cache(maxsize=None)
def _mixed(tree, sites, forced=False):
    off, idx, root = TREES[tree]()
    rng = np.random.default_rng(9000 + 31 * sites + len(tree) + (1 if forced else 0))
    out = _shapes.mixed_columns(rng, off, idx, root, sites, with_forced=forced)
    # (the first 33 sites may fall on quiet words: a fifth of their leaf codes redrawn, so the
    # shortest cases have records too)
    codes = out[0]
    hit = rng.random((codes.shape[0], min(33, sites))) < 0.2
    codes[:, :hit.shape[1]][hit] = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, size=int(hit.sum()))]
    return (off, idx, root) + tuple(out) + (() if forced else (None,))


def _both_vs_oracle(engine, oracle, inp, sites):
    want = _oracle(oracle, inp)
    assert want[0].shape[0] > 0
    _upload(engine, inp)
    try:
        plain, _ = _run(engine, 0)
        packed, launches = _run(engine, ALWAYS)
        _equal(packed, plain)
        _same_as_oracle(packed, want, inp[2], sites)
    finally:
        engine.set_down_pack(PACK_DEFAULT)
    return launches


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("tree", ["random-join", "sars-like"])
def test_equals_one_wave_per_node(engine, tree, graph):
    """141 words: two full tiles and a ragged tile of 13 words.  With the graph on, toggling the
    option re-captures (a capture runs the launch sequence, which reports; a replay does not)."""
    if tree == "sars-like":
        off, idx, root = panman_amd.sars_like_tree(6000, seed=31)
    else:
        off, idx, root = panman_amd.random_join_tree(8000, seed=32)
    engine.tree_upload(off, idx, root)
    engine.synth_columns(0, 4500, seed=7)
    try:
        engine.set_graph(False)
        want, _ = _run(engine, 0)
        assert want[0].shape[0] > 0
        engine.set_graph(graph)
        for pack in (0, ALWAYS):
            engine.set_down_pack(pack)
            phase_reset()
            engine.run(FITCH)
            first = dict(phase_report())
            assert first.get("run.down_pack") == GROUP_OF[pack], (pack, first)   # launched or captured anew
            if graph:
                phase_reset()
                engine.run(FITCH)
                assert "run.down_pack" not in dict(phase_report())   # the same option: a replay
            got = engine.mutations()
            score, rootc = engine.site_results()
            _equal((got, score, rootc), want)
    finally:
        engine.set_graph(False)
        engine.set_down_pack(PACK_DEFAULT)


@pytest.mark.parametrize("sites", [33, 2049, 4129])
def test_level_sizes_vs_oracle(engine, oracle, sites):
    """Levels of 1, G - 1, G and G + 1 nodes, each a packed launch of its own; sites: one word
    plus one site, a second tile of one word, two full tiles and a ragged one of two words."""
    launches = _both_vs_oracle(engine, oracle, _mixed("levels", sites), sites)
    assert launches == len(LEVEL_NODES)


@pytest.mark.parametrize("sites", [1, 33, 2049])
def test_kid_and_parent_kinds_vs_oracle(engine, oracle, sites):
    """Every kind of first / second child in one level under a polytomy, a unary node, tail
    children, dropped S2 / S3 children; 1 site, 33 sites, and a second tile holding one word."""
    assert _both_vs_oracle(engine, oracle, _mixed("kinds", sites), sites) > 0


@pytest.mark.parametrize("forced", [False, True], ids=["free", "forced"])
def test_root_parent(engine, oracle, forced):
    """The root's children read root_final (a forced root's differs from its set: every lane is
    live under the root); the root's own level is never packed and stays correct."""
    inp = _mixed("root", 2049, forced)
    assert _both_vs_oracle(engine, oracle, inp, 2049) > 0


def test_density_extremes(engine, oracle):
    """Tile 0 uniformly random in every leaf (every lane of every node live: T = 64 G, G rounds,
    the 128-entry stage flushed mid-wave), tile 1 at the consensus in every leaf (T = 0 below the
    root's children: the wave leaves, zero records there), tile 2 (ragged, 3 words) random again."""
    off, idx, root = level_tree()
    leaves = int((np.diff(off) == 0).sum())
    sites = 2 * 2048 + 70
    rng = np.random.default_rng(5)
    bases = np.array([1, 2, 4, 8], np.uint8)
    cons = bases[rng.integers(0, 4, size=sites)]
    codes = bases[rng.integers(0, 4, size=(leaves, sites))]
    codes[:, 2048:4096] = cons[None, 2048:4096]
    inp = (off, idx, root, codes, cons, None)
    want = _oracle(oracle, inp)
    assert want[0].shape[0] > 128 * G          # (more records than any stage holds)
    assert not ((want[0][:, 1] >= 2048) & (want[0][:, 1] < 4096)).any()   # the quiet tile: no record
    _upload(engine, inp)
    try:
        plain, _ = _run(engine, 0)
        packed, _ = _run(engine, ALWAYS)
        _equal(packed, plain)
        _same_as_oracle(packed, want, root, sites)
    finally:
        engine.set_down_pack(PACK_DEFAULT)


def test_absent_leaf_falls_back(engine, oracle):
    """A leaf missing from the alignment: the all-present kernels do not run, nothing packs."""
    inp = _mixed("kinds", 2049)
    rows = _shapes.leaf_rows(inp[0]).copy()
    rows[3] = -1
    want = _oracle(oracle, inp, node_row=rows)
    _upload(engine, inp, node_row=rows)
    try:
        off_res, _ = _run(engine, 0)
        on_res, _ = _run(engine, ALWAYS, expect=0)
    finally:
        engine.set_down_pack(PACK_DEFAULT)
    _equal(on_res, off_res)
    _same_as_oracle(on_res, want, inp[2], 2049)


def test_sankoff_keeps_its_levels(engine, oracle):
    inp = _mixed("kinds", 2049)
    want = _oracle(oracle, inp, SANKOFF)
    _upload(engine, inp)
    try:
        off_res, _ = _run(engine, 0, SANKOFF)
        on_res, _ = _run(engine, ALWAYS, SANKOFF)
    finally:
        engine.set_down_pack(PACK_DEFAULT)
    _equal(on_res, off_res)
    got, _, rootc = on_res
    assert got.shape == want[0].shape and (got == want[0]).all() and (rootc == want[1]).all()


def test_sub_down_keeps_its_levels(engine, oracle):
    """PM_OPT_SUB_DOWN: the levels run k_down<.., SUB>, never packed."""
    inp = _mixed("kinds", 2049)
    want = _oracle(oracle, inp)
    _upload(engine, inp)
    try:
        engine.set_sub_down(True)
        res, _ = _run(engine, ALWAYS, expect=0)
        _same_as_oracle(res, want, inp[2], 2049)
    finally:
        engine.set_sub_down(False)
        engine.set_down_pack(PACK_DEFAULT)


def test_groups_and_bands_keep_their_kernels(engine, oracle):
    """With the option on, a band takes its run of narrow levels and a level group its levels as
    before; only a level left a launch of its own packs."""
    inp = _mixed("levels", 2049)
    want = _oracle(oracle, inp)
    try:
        engine.set_narrow(16)            # every level of this tree is narrow: one band, nothing packs
        _upload(engine, inp)
        res, _ = _run(engine, ALWAYS, expect=0)
        _same_as_oracle(res, want, inp[2], 2049)
        engine.set_narrow(0)
        engine.set_group(32768, 4)       # the root's level and the three below it: one grouped launch
        _upload(engine, inp)
        res, launches = _run(engine, ALWAYS)
        assert launches == 1             # (the fifth level, alone)
        _same_as_oracle(res, want, inp[2], 2049)
    finally:
        _plain(engine)
        engine.set_down_pack(PACK_DEFAULT)


@pytest.mark.parametrize("tree, packs", [("levels", True), ("kinds", False)])
def test_leaf_parent_form(engine, oracle, tree, packs):
    """set_subtree(False): the leaf-parent form packs by the same rule -- its levels run the same
    kernel where each is one range of dense indices, which holds for a tree without three- and
    four-leaf subtrees (`levels`); with such subtrees materialised (`kinds`) its levels are no
    dense ranges, run k_down<.., !DENSE> and stay as they were."""
    inp = _mixed(tree, 2049)
    want = _oracle(oracle, inp)
    try:
        engine.set_subtree(False)
        _upload(engine, inp)
        plain, _ = _run(engine, 0)
        packed, launches = _run(engine, ALWAYS, expect=G if packs else 0)
        assert launches == (len(LEVEL_NODES) if packs else 0)
        _equal(packed, plain)
        _same_as_oracle(packed, want, inp[2], 2049)
    finally:
        engine.set_subtree(True)
        engine.set_down_pack(PACK_DEFAULT)


def test_threshold(engine):
    """The default leaves these levels (at most 2 (G + 1) waves) unpacked; a value >= 2 packs
    exactly the levels of at least that many (node, tile) waves; -1 packs every level."""
    inp = _mixed("levels", 2049)   # two tiles
    _upload(engine, inp)
    waves = [2 * n for n in LEVEL_NODES]

    def launches(value):
        engine.set_down_pack(value)
        phase_reset()
        engine.run(FITCH)
        ph = dict(phase_report())
        assert (ph["run.down_pack"] == G) == (ph["run.down_pack_launches"] > 0), ph
        return int(ph["run.down_pack_launches"])

    try:
        assert launches(PACK_DEFAULT) == 0 and launches(0) == 0
        assert launches(ALWAYS) == len(waves)
        for t in (2, 3, 2 * G - 2, 2 * G - 1, 2 * G, 2 * G + 1, 2 * G + 2, 2 * G + 3):
            assert launches(t) == sum(w >= t for w in waves), t
    finally:
        engine.set_down_pack(PACK_DEFAULT)


def test_combines_with_tail_pack(engine, oracle):
    """Both packed forms, each alone and together."""
    inp = _mixed("kinds", 2049)
    want = _oracle(oracle, inp)
    _upload(engine, inp)
    try:
        for tail in (0, ALWAYS):
            engine.set_tail_pack(tail)
            for pack in (0, ALWAYS):
                res, _ = _run(engine, pack)
                assert dict(phase_report())["run.tail_pack"] == (G if tail else 0)
                _same_as_oracle(res, want, inp[2], 2049)
    finally:
        engine.set_tail_pack(1)
        engine.set_down_pack(PACK_DEFAULT)
