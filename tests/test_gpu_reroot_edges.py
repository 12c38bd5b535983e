"""pm_reroot at the edges of its kernels and host steps (tests/_reroot_cases.py): dump for dump against the
hand-derived texts and against the oracle -- topology (deep chains, polytomies, unary nodes, both kinds of old
root), block states at the bcodes packing's edges, column counts around k_rows_to_codes' pairs and workgroups,
NucMut runs, and the column chunks of the nucleotide Fitch (PM_OPT_REROOT_CHUNK_SITES)."""
import numpy as np
import pytest

import _reroot_cases as cases
import panman_amd
from _panmat import tree_dump
from panman_amd.panmat import PanmanFile

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    e.close()


def _reroot(engine, pm, leaf):
    f = engine.reroot(pm, leaf)
    try:
        return tree_dump(f)
    finally:
        f.close()


@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_reroot_matches_hand_case(engine, name):
    case, leaf, want = cases.HAND[name]
    assert _reroot(engine, cases.hand_panmat(case), leaf) == want


@pytest.mark.parametrize("name", list(cases.EDGE))
def test_reroot_edge_matches_oracle(engine, oracle, name):
    case = cases.EDGE[name]()
    assert _reroot(engine, case.pm, case.leaf) == oracle.reroot(case.pm, case.leaf)


def test_unary_root_is_refused_and_the_engine_goes_on(engine, oracle):
    pm, leaf = cases.unary_root()
    assert oracle.reroot(pm, leaf) == "#error\tunary root\n"
    with pytest.raises(panman_amd.PanmanError, match="unary root"):
        engine.reroot(pm, leaf)
    case, leaf, want = cases.HAND["D_unary_node_on_the_chain"]
    assert _reroot(engine, cases.hand_panmat(case), leaf) == want


def test_missing_block_id(engine, oracle):
    pm, leaf = cases.block_ids_0_2()
    assert oracle.reroot(pm, leaf) == "#error\tBlock with id 1 -1 not found!\n"
    with pytest.raises(panman_amd.PanmanError, match="Block with id 1 -1 not found!"):
        engine.reroot(pm, leaf)


def test_reroot_twice_with_unary_nodes(engine, oracle, tmp_path):
    """Rerooted below the unary node of the chain, written, reloaded (internal nodes renamed in pre-order), then
    rerooted at a tip two levels below the new root and at one much deeper, behind the second unary node."""
    f = engine.reroot(cases.mixed_pm(), "t9")
    path = str(tmp_path / "once.panman")
    f.write(path)
    f.close()
    h = PanmanFile(path)
    pm2 = h.to_panmat(0)
    h.close()
    for leaf in ("t8", "t5"):
        assert _reroot(engine, pm2, leaf) == oracle.reroot(pm2, leaf)


@pytest.fixture(scope="module")
def runs_case(engine, oracle):
    case = cases.runs()
    want = oracle.reroot(case.pm, case.leaf)
    case.check(want)
    return case, want


def test_chunk_default_matches_oracle(engine, runs_case):
    case, want = runs_case
    assert _reroot(engine, case.pm, case.leaf) == want


@pytest.mark.parametrize("size", cases.CHUNK_SIZES)
def test_chunk_size_does_not_change_the_dump(engine, runs_case, size):
    """The second and later chunks: k_rows_to_codes from a column above 0 (odd for sizes 1 and 7), a shorter
    last chunk, records offset by the chunk's first column, runs rejoined across chunk edges."""
    case, want = runs_case
    engine.set_reroot_chunk_sites(size)
    try:
        got = _reroot(engine, case.pm, case.leaf)
    finally:
        engine.set_reroot_chunk_sites(0)
    assert got == want


@pytest.mark.parametrize("size", (2, 7, 64))
def test_chunk_size_is_what_the_context_ran_last(engine, runs_case, size):
    """The option takes effect: the context's last run is pm_reroot's last chunk, so its records are those of
    the one-chunk run from that chunk's first column on, their sites counted from it."""
    case, _ = runs_case
    _reroot(engine, case.pm, case.leaf)
    whole = engine.mutations()
    engine.set_reroot_chunk_sites(size)
    try:
        _reroot(engine, case.pm, case.leaf)
        last = engine.mutations()
    finally:
        engine.set_reroot_chunk_sites(0)
    c0 = (case.columns - 1) // size * size
    want = whole[whole[:, 1] >= c0].copy()
    want[:, 1] -= c0
    assert 0 < len(want) < len(whole) and np.array_equal(last, want)


def test_chunk_option_range(engine):
    for bad in (-1, (1 << 24) - 4095):
        with pytest.raises(panman_amd.PanmanError, match="PM_OPT_REROOT_CHUNK_SITES"):
            engine.set_reroot_chunk_sites(bad)
    try:
        engine.set_reroot_chunk_sites((1 << 24) - 4096)
    finally:
        engine.set_reroot_chunk_sites(0)
