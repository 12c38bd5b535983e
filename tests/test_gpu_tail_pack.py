"""PM_OPT_TAIL_PACK: the tail's S2 / S3 items in groups of G per wave, a group's dirty (item,
word) pairs gathered into full waves (k_tail<.., G>), give exactly the records, per-site scores
and root codes of one wave per item -- and of the oracle -- at the group edges (ragged last
group, fewer items than G), the tile edges, under a root parent, and at both extremes of lane
density (every lane of every item dirty: G rounds and mid-wave stage flushes; no lane dirty: the
wave leaves).  Every case reads the group size it ran with off phase_report()."""
import functools

import numpy as np
import pytest

import _shapes
import panman_amd
from _trees import names_for
from panman_amd._lib import phase_report, phase_reset
from panman_amd.engine import CLUSTER_DEFAULT

pytestmark = pytest.mark.gpu

FITCH, SANKOFF = panman_amd.MODE_FITCH, panman_amd.MODE_SANKOFF
PACK_DEFAULT = 1          # the library's default: on from kTailPackMinWaves (item, tile) waves
ALWAYS = -1               # on at any size: these trees are far below the threshold
MIN_WAVES = 65536         # kTailPackMinWaves
GROUP_OF = {0: 0, ALWAYS: 8}   # the group size a run reports (kTailPack)


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    e.set_cluster(CLUSTER_DEFAULT)
    yield e
    e.set_tail_pack(PACK_DEFAULT)
    e.set_graph(False)
    e.close()


def _run(engine, pack, mode=FITCH):
    """One run with PM_OPT_TAIL_PACK = pack; (records, score, root codes)."""
    engine.set_tail_pack(pack)
    phase_reset()
    engine.run(mode)
    ph = dict(phase_report())
    if mode == FITCH and "run.tail_pack" in ph:   # (absent: a graph replay, nothing launched by hand)
        assert ph["run.tail_pack"] == GROUP_OF[pack], ph
    got = engine.mutations()
    score, rootc = engine.site_results()
    return got, score, rootc


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


def _upload(engine, inp):
    off, idx, root, codes, cons, forced = inp
    engine.set_cluster(CLUSTER_DEFAULT)
    engine.tree_upload(off, idx, root)
    engine.leaves_upload(codes, _shapes.leaf_rows(off))
    engine.sites_upload(cons, forced)


def _oracle(oracle, inp, mode=FITCH):
    off, idx, root, codes, cons, forced = inp
    _, recs, rootc = oracle.csr_columns(off, idx, root, names_for(off), codes, _shapes.leaf_rows(off), cons, forced,
                                        algo=mode, threads=8, with_root=True)
    return recs, rootc


@functools.lru_cache(maxsize=None)
def caterpillar(k):
    """A spine of binary nodes carrying exactly k S-shaped children, alternating s2 / s3, above a
    three-leaf node (never evaluated inline): k S2 / S3 tail items, each under a binary parent."""
    b = _shapes._Builder()
    cur = b.node([b.leaf(), b.leaf(), b.leaf()])
    for i in range(k):
        cur = b.node([cur, b.kind("s3" if i % 2 else "s2")])
    return b.csr(cur)


@functools.lru_cache(maxsize=None)
def _mixed(tree_key, sites, forced=False):
    kind, arg = tree_key
    off, idx, root = (caterpillar(arg) if kind == "cat" else _shapes.edge_tree() if kind == "edge"
                      else _shapes.star_with_sibling(arg) if kind == "star" else _root_pair())
    rng = np.random.default_rng(7000 + 31 * sites + (arg or 0) + (1 if forced else 0))
    out = _shapes.mixed_columns(rng, off, idx, root, sites, with_forced=forced)
    # (the first 33 sites may fall on quiet words: a fifth of their leaf codes redrawn, so the
    # shortest case has records too)
    codes = out[0]
    hit = rng.random((codes.shape[0], 33)) < 0.2
    codes[:, :33][hit] = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, size=int(hit.sum()))]
    return (off, idx, root) + tuple(out) + (() if forced else (None,))


def _root_pair():
    """root = (S2, S3): both tail items' parent is the root, every lane dirty, the parent's final
    read from root_final."""
    b = _shapes._Builder()
    return b.csr(b.node([b.kind("s2"), b.kind("s3")]))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("tree", ["random-join", "sars-like"])
def test_equals_one_wave_per_item(engine, tree, graph):
    """141 words: two full tiles and a ragged tile of 13 words.  With the graph on, toggling the
    option re-captures (a capture runs the launch sequence, which reports; a replay does not)."""
    if tree == "sars-like":
        off, idx, root = panman_amd.sars_like_tree(6000, seed=31)
    else:
        off, idx, root = panman_amd.random_join_tree(8000, seed=32)
    engine.set_cluster(CLUSTER_DEFAULT)
    engine.tree_upload(off, idx, root)
    engine.synth_columns(0, 4500, seed=7)
    try:
        engine.set_graph(False)
        want = _run(engine, 0)
        assert want[0].shape[0] > 0
        engine.set_graph(graph)
        for pack in (0, ALWAYS):
            engine.set_tail_pack(pack)
            phase_reset()
            engine.run(FITCH)
            first = dict(phase_report())
            assert first.get("run.tail_pack") == GROUP_OF[pack], (pack, first)   # launched or captured anew
            if graph:
                phase_reset()
                engine.run(FITCH)
                assert "run.tail_pack" not in dict(phase_report())   # the same option: a replay
            _equal(_run(engine, pack), want)
    finally:
        engine.set_graph(False)
        engine.set_tail_pack(PACK_DEFAULT)


def test_threshold(engine):
    """The default packs from kTailPackMinWaves (S item, tile) waves; a value >= 2 is the threshold
    (waves >= threshold packs), -1 packs whatever the size."""
    off, idx, root = panman_amd.random_join_tree(8000, seed=32)
    engine.set_cluster(CLUSTER_DEFAULT)
    engine.tree_upload(off, idx, root)
    engine.synth_columns(0, 4500, seed=7)

    def group(value):
        engine.set_tail_pack(value)
        phase_reset()
        engine.run(FITCH)
        ph = dict(phase_report())
        return ph["run.tail_pack"], int(ph["run.tail_s_waves"])

    try:
        g, waves = group(PACK_DEFAULT)
        assert 2 <= waves < MIN_WAVES and waves % 3 == 0 and g == 0, (g, waves)   # (three tiles)
        assert group(waves)[0] == 8 and group(waves + 1)[0] == 0
        assert group(ALWAYS)[0] == 8 and group(0)[0] == 0
    finally:
        engine.set_tail_pack(PACK_DEFAULT)


@pytest.mark.parametrize("sites", [33, 2049, 4096])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33])
def test_group_edges_vs_oracle(engine, oracle, k, sites):
    """k S items: a ragged last group and fewer items than G for G = 4, 8 and 16 alike; sites: one
    word plus one site, a second tile of one word, two full tiles."""
    inp = _mixed(("cat", k), sites)
    want = _oracle(oracle, inp)
    assert want[0].shape[0] > 0
    _upload(engine, inp)
    try:
        for pack in (0, ALWAYS):
            _same_as_oracle(_run(engine, pack), want, inp[2], sites)
    finally:
        engine.set_tail_pack(PACK_DEFAULT)


@pytest.mark.parametrize("forced", [False, True], ids=["free", "forced"])
def test_root_parent(engine, oracle, forced):
    inp = _mixed(("root", 0), 2049, forced)
    want = _oracle(oracle, inp)
    assert want[0].shape[0] > 0
    _upload(engine, inp)
    try:
        for pack in (0, ALWAYS):
            _same_as_oracle(_run(engine, pack), want, inp[2], 2049)
    finally:
        engine.set_tail_pack(PACK_DEFAULT)


@pytest.mark.parametrize("tree", [("edge", 0), ("star", 300)], ids=["edge", "star300"])
def test_mixed_density(engine, oracle, tree):
    """The edge tree's S children under nodes of every degree class with random, uniform and quiet
    words in every tile; the star's tail launch holds both its leaves beyond the second (one wave
    each) and two S items (packed), so both tail launches run."""
    sites = 4129   # two full tiles and a ragged one of two words
    inp = _mixed(tree, sites)
    want = _oracle(oracle, inp)
    _upload(engine, inp)
    try:
        for pack in (0, ALWAYS):
            _same_as_oracle(_run(engine, pack), want, inp[2], sites)
    finally:
        engine.set_tail_pack(PACK_DEFAULT)


def test_density_extremes(engine, oracle):
    """17 S items, tile 0 uniformly random in every leaf (all 64 lanes of every item dirty:
    T = 64 G, G rounds, the 128-entry stage flushed mid-wave), tile 1 at the consensus in every
    leaf (T = 0: the wave leaves), tile 2 (ragged, 3 words) random again."""
    off, idx, root = caterpillar(17)
    leaves = int((np.diff(off) == 0).sum())
    sites = 2 * 2048 + 70
    rng = np.random.default_rng(5)
    bases = np.array([1, 2, 4, 8], np.uint8)
    cons = bases[rng.integers(0, 4, size=sites)]
    codes = bases[rng.integers(0, 4, size=(leaves, sites))]
    codes[:, 2048:4096] = cons[None, 2048:4096]
    inp = (off, idx, root, codes, cons, None)
    want = _oracle(oracle, inp)
    assert want[0].shape[0] > 128 * 17   # (more records than any stage holds)
    _upload(engine, inp)
    try:
        for pack in (0, ALWAYS):
            _same_as_oracle(_run(engine, pack), want, root, sites)
    finally:
        engine.set_tail_pack(PACK_DEFAULT)


def test_sankoff_keeps_its_tail(engine, oracle):
    """Sankoff's S items stay one wave per item whatever the option says: the same results with
    it on and off, and the oracle's."""
    inp = _mixed(("cat", 9), 2049)
    want = _oracle(oracle, inp, SANKOFF)
    _upload(engine, inp)
    try:
        off_res = _run(engine, 0, SANKOFF)
        on_res = _run(engine, ALWAYS, SANKOFF)
    finally:
        engine.set_tail_pack(PACK_DEFAULT)
    _equal(on_res, off_res)
    got, _, rootc = on_res
    assert got.shape == want[0].shape and (got == want[0]).all() and (rootc == want[1]).all()
