"""pm_leaves_upload_sparse against pm_leaves_upload of the same matrix built densely: the leaf codes
read back, and the block Fitch records.  Shapes around the kernel's edges: one lane expands one
32-bit word (8 sites) of a staging row, found by binary search in the row's entry list."""
import numpy as np
import pytest

import panman_amd
from _trees import random_tree

pytestmark = pytest.mark.gpu

SITES = [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1001]
ROWS = [1, 3, 70]


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    e.close()


def _tree(rows, rng):
    """A tree with rows + 2 leaves (two of them get no row)."""
    off, idx, root = random_tree(rows + 2, rng, max_children=3, unary=0.0)
    leaves = [v for v in range(len(off) - 1) if off[v] == off[v + 1]]
    return off, idx, root, leaves


def _matrix(rows, S, fill, rng):
    """Dense [rows, S] codes: `fill` except at random entries; then the listed special rows."""
    dense = np.full((rows, S), fill, np.uint8)
    mask = rng.random((rows, S)) < 0.2
    dense[mask] = rng.integers(0, 3 if fill == 0 else 16, size=int(mask.sum()), dtype=np.uint8)
    listed = mask.copy()

    def whole(r, sites):
        listed[r] = False
        dense[r] = fill
        for s in sites:
            listed[r, s] = True
            dense[r, s] = 1 + (s + r) % 2

    kinds = [[], range(S), [0], [S - 1], [s for s in (2, 3) if s < S], [s for s in (8, 15) if s < S]]
    for k, sites in enumerate(kinds):   # empty, full, only site 0, only S - 1, one byte, one word
        if k < rows:
            whole(rows - 1 - k, list(sites))
    return dense, listed


def _csr(dense, listed):
    row_off = np.zeros(dense.shape[0] + 1, np.int64)
    site, code = [], []
    for r in range(dense.shape[0]):
        s = np.flatnonzero(listed[r])
        site += s.tolist()
        code += dense[r, s].tolist()
        row_off[r + 1] = len(site)
    return row_off, np.array(site, np.int32), np.array(code, np.uint8)


def _upload_both(engine, rows, S, fill, seed):
    rng = np.random.default_rng(seed)
    off, idx, root, leaves = _tree(rows, rng)
    dense, listed = _matrix(rows, S, fill, rng)
    node_row = np.full(len(off) - 1, -1, np.int32)
    order = rng.permutation(len(leaves))
    for r in range(rows):
        node_row[leaves[order[r]]] = r     # the last two leaves of the permutation: no row
    engine.tree_upload(off, idx, root)
    engine.leaves_upload(dense, node_row)
    want_codes = engine.leaf_codes(0, S, len(leaves))
    engine.sites_upload(np.zeros(S, np.uint8))
    engine.run(panman_amd.MODE_BLOCK_FITCH)
    want_recs = engine.mutations()
    row_off, site, code = _csr(dense, listed)
    engine.leaves_upload_sparse(row_off, site, code, node_row, S, fill_code=fill)
    got_codes = engine.leaf_codes(0, S, len(leaves))
    engine.sites_upload(np.zeros(S, np.uint8))
    engine.run(panman_amd.MODE_BLOCK_FITCH)
    got_recs = engine.mutations()
    expect = np.array([dense[node_row[v]] if node_row[v] >= 0 else np.zeros(S, np.uint8) for v in leaves])
    return expect, want_codes, got_codes, want_recs, got_recs


@pytest.mark.parametrize("fill", [0, 3])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("S", SITES)
def test_sparse_equals_dense(engine, S, rows, fill):
    expect, want_codes, got_codes, want_recs, got_recs = _upload_both(engine, rows, S, fill, 1000 * rows + S)
    assert (want_codes == expect).all()
    assert (got_codes == want_codes).all()
    assert got_recs.shape == want_recs.shape and (got_recs == want_recs).all()
    if rows == 70 and S >= 7:
        assert len(got_recs) > S


def test_every_code_and_a_previous_upload_left_behind(engine):
    """Codes 0..15 in the entries; the sparse upload follows a dense one of another shape."""
    rng = np.random.default_rng(5)
    off, idx, root, leaves = _tree(9, rng)
    node_row = np.full(len(off) - 1, -1, np.int32)
    node_row[leaves[:9]] = np.arange(9)
    S = 77
    dense = rng.integers(0, 16, size=(9, S), dtype=np.uint8)
    listed = dense != 5
    engine.tree_upload(off, idx, root)
    engine.leaves_upload(rng.integers(0, 16, size=(9, 300), dtype=np.uint8), node_row)
    row_off, site, code = _csr(dense, listed)
    engine.leaves_upload_sparse(row_off, site, code, node_row, S, fill_code=5)
    got = engine.leaf_codes(0, S, len(leaves))
    assert (got[:9] == dense).all() and (got[9:] == 0).all()


def test_bad_arguments_are_errors(engine):
    rng = np.random.default_rng(6)
    off, idx, root, leaves = _tree(2, rng)
    node_row = np.full(len(off) - 1, -1, np.int32)
    node_row[leaves[0]], node_row[leaves[1]] = 0, 1
    engine.tree_upload(off, idx, root)
    good = ([0, 2, 3], [1, 4, 0], [1, 2, 1])
    bad = [
        ("not strictly increasing", ([0, 2, 3], [4, 1, 0], [1, 2, 1])),
        ("not strictly increasing", ([0, 2, 3], [4, 4, 0], [1, 2, 1])),   # a repeated site
        ("site out of range", ([0, 2, 3], [1, 9, 0], [1, 2, 1])),
        ("site out of range", ([0, 2, 3], [-1, 4, 0], [1, 2, 1])),
        ("code above 15", ([0, 2, 3], [1, 4, 0], [1, 16, 1])),
    ]
    for what, (row_off, site, code) in bad:
        with pytest.raises(panman_amd.PanmanError) as err:
            engine.leaves_upload_sparse(row_off, site, code, node_row, 9)
        assert "rc=-1" in str(err.value) and what in str(err.value), what
    beyond = node_row.copy()
    beyond[leaves[2]] = 2
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.leaves_upload_sparse(*good, beyond, 9)
    assert "rc=-1" in str(err.value) and "node_row" in str(err.value)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.leaves_upload_sparse(*good, node_row, 1 << 24)
    assert "rc=-1" in str(err.value)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.leaves_upload_sparse(*good, node_row, 9, fill_code=16)
    assert "rc=-1" in str(err.value)
    engine.leaves_upload_sparse(*good, node_row, 9)   # the context is still usable
    got = engine.leaf_codes(0, 9, len(leaves))
    assert got[0].tolist() == [0, 1, 0, 0, 2, 0, 0, 0, 0] and got[1].tolist() == [1] + [0] * 8


def test_the_tree_comes_first():
    e = panman_amd.Engine(0)
    try:
        with pytest.raises(panman_amd.PanmanError) as err:
            e.leaves_upload_sparse([0], [], [], [-1], 4)
        assert "rc=-5" in str(err.value)
    finally:
        e.close()
