"""The subtree form (every leaf present) against the oracle at the degree, band and option edges
the launch schedule branches on (run_paths / schedule_run in pm_schedule.cpp, executed by
launch_fitch / launch_sankoff: sub, grp, clu -- Sankoff's with h0 == 0 and no node above 255
children, "sk_clu" below -- cld, sub_down, narrow bands, level groups, the non-temporal build,
the four out-degree classes), on the
deterministic trees and mixed-class columns of _shapes.py.  Every comparison is bit-exact:
records, root codes and score == records per site; every case reads the path it means to take
off phase_report()."""
import functools

import numpy as np
import pytest

import _shapes
import panman_amd
from _trees import names_for, random_tree
from panman_amd._lib import phase_report, phase_reset
from panman_amd.engine import CLUSTER_DEFAULT

pytestmark = pytest.mark.gpu

FITCH, SANKOFF = panman_amd.MODE_FITCH, panman_amd.MODE_SANKOFF
MODES = [pytest.param(FITCH, id="fitch"), pytest.param(SANKOFF, id="sankoff")]
ALL = 1 << 20   # a level threshold no level exceeds: every height swept, cluster.first_level == 0

DEFAULTS = dict(cluster=CLUSTER_DEFAULT, narrow=16, group=(32768, 4), up_group=True, plain_up=(True, 0),
                sub_down=False, nt=-1, graph=False, subtree=True, virtual=True)


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    _apply(e, DEFAULTS)
    e.close()


def _apply(engine, cfg):
    engine.set_cluster(cfg["cluster"])
    engine.set_narrow(cfg["narrow"])
    engine.set_group(*cfg["group"])
    engine.set_up_group(cfg["up_group"])
    engine.set_plain_up(*cfg["plain_up"])
    engine.set_sub_down(cfg["sub_down"])
    engine.set_nt_loads(cfg["nt"])
    engine.set_graph(cfg["graph"])
    engine.set_subtree(cfg["subtree"])
    engine.set_virtual(cfg["virtual"])


@functools.lru_cache(maxsize=None)
def _tree(key):
    kind, arg = key
    if kind == "edge":
        return _shapes.edge_tree(_shapes.MAIN_DEGREES, unary_every=7)
    if kind == "wide":
        return _shapes.edge_tree(_shapes.WIDE_DEGREES)
    if kind == "ladder":
        return _shapes.ladder(arg)
    if kind == "fat":
        return _shapes.fat_cluster(arg)
    if kind == "five":
        return _shapes.fat_cluster(0, five_live=True)
    if kind == "random":
        return random_tree(1500, np.random.default_rng(arg), max_children=9, unary=0.05)
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def _inputs(key, sites, forced):
    """(off, idx, root, codes, cons, forced | None), computed once and left unchanged."""
    off, idx, root = _tree(key)
    rng = np.random.default_rng(9000 + sites + (1 if forced else 0))
    out = _shapes.mixed_columns(rng, off, idx, root, sites, with_forced=forced)
    return (off, idx, root) + tuple(out) + (() if forced else (None,))


_WANT = {}


def _want(oracle, cache_key, inp, mode):
    """The oracle's (records, root codes), once per input and mode."""
    k = (cache_key, mode)
    if k not in _WANT:
        off, idx, root, codes, cons, forced = inp
        _, recs, rootc = oracle.csr_columns(off, idx, root, names_for(off), codes, _shapes.leaf_rows(off), cons,
                                            forced, algo=mode, threads=8, with_root=True)
        _WANT[k] = (recs, rootc)
    return _WANT[k]


def _upload(engine, inp, cfg):
    """Options, tree and columns; returns the upload's phase report."""
    off, idx, root, codes, cons, forced = inp
    _apply(engine, {**DEFAULTS, **cfg})
    phase_reset()
    engine.tree_upload(off, idx, root)
    ph = dict(phase_report())
    engine.leaves_upload(codes, _shapes.leaf_rows(off))
    engine.sites_upload(cons, forced)
    return ph


def _run(engine, mode):
    """One run; returns (records, score, root codes, the run's phase report)."""
    phase_reset()
    engine.run(mode)
    run_ph = dict(phase_report())
    got = engine.mutations()
    score, rootc = engine.site_results()
    return got, score, rootc, run_ph


def _same(res, want, inp):
    got, score, rootc = res[:3]
    recs, want_root = want
    root, sites = inp[2], inp[4].shape[0]
    assert recs.shape[0] > 0
    if got.shape == recs.shape and not (got == recs).all():
        k = int(np.flatnonzero((got != recs).any(axis=1))[0])
        raise AssertionError(f"first differing record {k}: got {got[k]}, oracle {recs[k]}")
    assert got.shape == recs.shape, (got.shape, recs.shape)
    assert (rootc == want_root).all()
    nonroot = recs[recs[:, 0] != root]
    assert (score == np.bincount(nonroot[:, 1], minlength=sites)).all()


# (name, options, what the upload's / run's phase report must show)
# The main edge tree's heights 1 and 2 hold the wide feature nodes' materialised (cherry, leaf) /
# (cherry, cherry) children -- well over 64 nodes -- while every level of the spine's top holds
# one node: thresholds 2 and 64 start the sweeps above height 0 (partial sweeps, no pre-order
# sweeps); its widest node has 255 children, so Sankoff sweeps it too (cl.max_degree <= 255,
# which the report does not expose).
CONFIGS = [
    ("defaults", {}, lambda ph, run: ph["cluster.bands"] > 0),
    ("cluster0", dict(cluster=0), lambda ph, run: ph["cluster.bands"] == 0),
    ("all", dict(cluster=ALL),
     lambda ph, run: ph["cluster.bands"] > 0 and ph["cluster.first_level"] == 0 and ph["cluster.down"] == 1),
    # (set_group(0) is accepted: one pre-order launch per level)
    ("partial2_no_bands_no_groups", dict(cluster=2, narrow=0, group=(0, 4)),
     lambda ph, run: ph["cluster.bands"] > 0 and ph["cluster.first_level"] > 0 and ph["cluster.down"] == 0),
    ("partial64_heights_wide_bands", dict(cluster=64, up_group=False, narrow=1024),
     lambda ph, run: ph["cluster.bands"] > 0 and ph["cluster.first_level"] > 0 and ph["cluster.down"] == 0),
    # (the plan still has its pre-order clusters; launch_fitch leaves them for k_down<.., SUB>:
    # cld = clu && cl.down && !sub_down.  Sankoff ignores the option.)
    ("all_sub_down", dict(cluster=ALL, sub_down=True),
     lambda ph, run: ph["cluster.bands"] > 0 and ph["cluster.first_level"] == 0),
    ("all_nt", dict(cluster=ALL, nt=1),
     lambda ph, run: ph["cluster.bands"] > 0 and ph["cluster.first_level"] == 0 and run["run.nt_loads"] == 1),
    # (the second run logs no launch sequence: it replays the captured graph)
    ("all_graph", dict(cluster=ALL, graph=True),
     lambda ph, run: ph["cluster.bands"] > 0 and ph["cluster.first_level"] == 0 and "run.nt_loads" not in run),
    ("plain_up_min_waves2", dict(plain_up=(True, 2)), lambda ph, run: ph["cluster.bands"] > 0),
    # (sub is false without the subtree form / the virtual leaf-parents: the plan is made at
    # upload all the same but no launcher uses it)
    ("leafparent_form", dict(subtree=False, virtual=True), lambda ph, run: True),
    ("plain_form", dict(virtual=False), lambda ph, run: True),
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", range(len(CONFIGS)), ids=[c[0] for c in CONFIGS])
def test_edge_tree_option_matrix(engine, oracle, k, mode):
    """The main edge tree (degrees 1 .. 255 with children of every kind, unary nodes in the
    spine), mixed-class columns at 2049 sites, a forced root on odd configs."""
    name, cfg, path_ok = CONFIGS[k]
    forced = bool(k % 2)
    inp = _inputs(("edge", 0), 2049, forced)
    want = _want(oracle, ("edge", 2049, forced), inp, mode)
    try:
        ph = _upload(engine, inp, cfg)
        res = _run(engine, mode)
        if cfg.get("graph"):
            first = res
            res = _run(engine, mode)
            assert "run.nt_loads" in first[3]   # (the first run captured the launch sequence)
            _same(first, want, inp)
    finally:
        _apply(engine, DEFAULTS)
    assert path_ok(ph, res[3]), (name, ph, res[3])
    _same(res, want, inp)


@pytest.mark.parametrize("mode", MODES)
def test_cluster_switched_off_after_upload(engine, oracle, mode):
    """set_cluster(0) after an upload that built a plan: Fitch falls back to one launch per
    height over the subtree form's own order (grp needs clu || !planned: pslot_k with
    up_desc_k), Sankoff keeps its grouped launches; switched on again, the sweeps return."""
    inp = _inputs(("edge", 0), 2049, False)
    want = _want(oracle, ("edge", 2049, False), inp, mode)
    try:
        ph = _upload(engine, inp, dict(cluster=ALL))
        assert ph["cluster.bands"] > 0 and ph["cluster.first_level"] == 0, ph
        engine.set_cluster(0)
        _same(_run(engine, mode), want, inp)
        engine.set_cluster(ALL)
        _same(_run(engine, mode), want, inp)
    finally:
        _apply(engine, DEFAULTS)


@pytest.mark.parametrize("up_group", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_sankoff_down_sweeps_over_part_merge_records(engine, oracle, mode, up_group):
    """Nodes of 256, 257 and 300 children of mixed kinds with every height swept: Sankoff's
    post-order stays level kernels (sk_clu needs cl.max_degree <= 255, not in the report) with
    k_sankoff_part / k_sankoff_merge, and its pre-order sweeps (k_down_cluster<Sankoff>) read
    their records; Fitch runs k_fitch_up_wide's degree class inside the sweeps."""
    inp = _inputs(("wide", 0), 2049, True)
    want = _want(oracle, ("wide", 2049, True), inp, mode)
    assert np.diff(inp[0]).max() == 300
    try:
        ph = _upload(engine, inp, dict(cluster=ALL, up_group=up_group))
        res = _run(engine, mode)
    finally:
        _apply(engine, DEFAULTS)
    assert ph["cluster.bands"] > 0 and ph["cluster.first_level"] == 0 and ph["cluster.down"] == 1, ph
    _same(res, want, inp)


@pytest.mark.parametrize("cluster", [ALL, CLUSTER_DEFAULT], ids=["all", "default"])
@pytest.mark.parametrize("heights", [31, 32, 33, 64, 65, 129])
@pytest.mark.parametrize("mode", MODES)
def test_ladder_band_edges(engine, oracle, mode, heights, cluster):
    """Chains of exactly `heights` levels, one node each: plan_clusters cuts a band after
    kClBandHeights = 32 levels (a chain needs one slot and 32 steps), so ceil(heights / 32)
    bands, the longest cluster min(heights, 32) steps; a chain is never bushy (one node per
    level <= kClChain), so the default plan is the same."""
    inp = _inputs(("ladder", heights), 2048, heights % 2 == 1)
    want = _want(oracle, ("ladder", heights, 2048), inp, mode)
    try:
        ph = _upload(engine, inp, dict(cluster=cluster))
        res = _run(engine, mode)
    finally:
        _apply(engine, DEFAULTS)
    assert ph["cluster.bands"] == -(-heights // 32) and ph["cluster.first_level"] == 0, ph
    assert ph["cluster.max_rounds"] == min(heights, 32) and ph["cluster.down"] == 1, ph
    _same(res, want, inp)


# fat_cluster(63 / 64): 18 levels, three slots, `nodes` <= kClMaxSteps steps: one band, one cluster.
# fat_cluster(65): band [0, 18) has a 65-node cluster (size > kClMaxSteps), so plan_clusters'
# binary search keeps the tallest band that fits, [0, 17): it leaves out the root alone, and its
# clusters are X = (chain 16, chain 16) with 33 nodes and Y = (chain 15, chain 15) with 31; the
# root is the second band.  Five live sets: P's five chains each hold an LDS slot until P's
# step, one more than kClSlots, so the first band stops below P ([0, 3): five clusters of 3
# nodes) and P and the root (2 nodes) make the second.
FAT = [("fat", 63, 1, 63), ("fat", 64, 1, 64), ("fat", 65, 2, 33), ("five", 0, 2, 3)]


@pytest.mark.parametrize("kind,nodes,bands,rounds", FAT, ids=["63", "64", "65", "five_live_sets"])
@pytest.mark.parametrize("mode", MODES)
def test_cluster_size_and_slot_edges(engine, oracle, mode, kind, nodes, bands, rounds):
    inp = _inputs((kind, nodes), 2049, nodes % 2 == 1)
    want = _want(oracle, (kind, nodes, 2049), inp, mode)
    try:
        ph = _upload(engine, inp, dict(cluster=ALL))
        res = _run(engine, mode)
    finally:
        _apply(engine, DEFAULTS)
    assert ph["cluster.first_level"] == 0 and ph["cluster.down"] == 1, ph
    assert ph["cluster.max_rounds"] <= 64, ph
    assert ph["cluster.bands"] == bands and ph["cluster.max_rounds"] == rounds, ph
    _same(res, want, inp)


@pytest.mark.parametrize("width", [255, 256, 257, 4096, 65535, 65536, 65537])
@pytest.mark.parametrize("mode", MODES)
def test_all_present_stars(engine, oracle, mode, width):
    """A star of `width` leaves beside a subtree with an S2 and an S3 node, no leaf absent: the
    subtree form (sub needs num_sshape > 0 and every leaf present; neither is in the report).
    The default plan sweeps the three materialised nodes as one cluster; from 256 children on
    Sankoff's post-order is k_sankoff_part with k_sankoff_merge<16>, from 65 536 on <32>."""
    off, idx, root = _shapes.star_with_sibling(width)
    rng = np.random.default_rng(width)
    leaves = width + 7
    alphabet = np.array([1, 2, 4, 8, 1, 2, 4, 8, 0, 15, 5, 10, 3], np.uint8)
    codes = alphabet[rng.integers(0, alphabet.size, size=(leaves, 97))]
    codes[rng.random(codes.shape) < 0.2] = 0
    codes[rng.random(codes.shape) < 0.6] = 4   # a majority state
    cons = rng.choice(np.array([1, 2, 4, 8], np.uint8), size=97)
    # sites where every child of the star agrees, so one code's count is the full width (the
    # counters' widths are what the degree classes and merge<16> / <32> differ in) and the
    # sibling's leaves disagree (a star whose set came out wrong then follows the root's state
    # and every one of its leaves gets a record); one site where all but one child agree
    codes[:width, 0:4] = np.array([4, 4, 2, 15], np.uint8)
    codes[width:, 0:4] = np.array([1, 1, 1, 0], np.uint8)
    codes[0, 2] = 8
    cons[0:4] = np.array([1, 4, 1, 2], np.uint8)
    inp = (off, idx, root, codes, cons, None)
    want = _want(oracle, ("star", width), inp, mode)
    try:
        ph = _upload(engine, inp, {})
        res = _run(engine, mode)
    finally:
        _apply(engine, DEFAULTS)
    assert ph["cluster.bands"] == 1 and ph["cluster.first_level"] == 0 and ph["cluster.max_rounds"] == 3, ph
    _same(res, want, inp)


@pytest.mark.parametrize("cluster", [CLUSTER_DEFAULT, ALL], ids=["default", "all"])
@pytest.mark.parametrize("mode", MODES)
def test_mixed_classes_every_column(engine, oracle, mode, cluster):
    """A random polytomy tree with unary nodes, 4100 sites whose words mix the consensus, simple
    and complex record classes inside every tile, a forced root: every column against the
    oracle.  (Whether the default plan sweeps a random tree depends on its bands' bushiness, so
    the path is asserted for the explicit threshold only.)"""
    inp = _inputs(("random", 77), 4100, True)
    want = _want(oracle, ("random", 4100), inp, mode)
    try:
        ph = _upload(engine, inp, dict(cluster=cluster))
        res = _run(engine, mode)
    finally:
        _apply(engine, DEFAULTS)
    if cluster == ALL:
        assert ph["cluster.bands"] > 0 and ph["cluster.first_level"] == 0, ph
    _same(res, want, inp)
