"""pm_to_usher on the GPU, byte for byte against the Python restatement (tests/_usher_ref.py, pinned to
src/panman2usher.cpp by tests/test_usher_ref.py): the hand cases against their written-out bytes, random
PanMATs with block mutations and all six types, and the kernels' edges (tests/_usher_cases.py, each shape
proved present by tests/test_usher_cases.py) -- entries per node around a wave and around
k_usher_write's round, a run that straddles a round's end, positions and list lengths on both sides of
the varint steps, all 16 codes, ref and par zero and non-zero, runs in slots, over bases and into the
sentinel, cells written two and three times in one list, 258 nodes whose pre-order is not their id order
over 130 blocks, block mutations that change nothing; batches of one node, a pipe and a file, the error
codes; and pm_print_mutations unchanged by the move of its helpers."""
import os
import threading

import pytest

import panman_amd
import _mutations_ref
import _usher_ref
from _usher_cases import (ARG_ERRORS, HAND, RANDOM, UNSUPPORTED, codes_case, entry_count_case, list_length_case,
                          long_text_case, one_node_batches_case, position_case, random_case, rewrite_case, root_map_case,
                          straddle_case, substitution_case, without_block_mutations)
from panman_amd._lib import phase_report, phase_reset

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def permuted():
    """(the 258-node PanMAT, the restatement's result): computed once, read by two tests."""
    pm, _ = root_map_case()
    return pm, _usher_ref.to_usher(pm)


def _assert_same(got, want, where=()):
    """got == want for (bytes, records), naming the first node and record that differ."""
    if got[0] != want[0]:
        pytest.fail(f"{where}: {_usher_ref.first_difference(got[0], want[0])}", pytrace=False)
    assert got[1] == want[1], (where, got[1], want[1])


@pytest.mark.parametrize("name", list(HAND))
def test_hand_case(engine, name):
    pm, want = HAND[name]()
    got, count = engine.to_usher(pm)
    _assert_same((got, count), (want, sum(map(len, _usher_ref.decode(want)[1]))), name)


@pytest.mark.parametrize("leaves,seed", RANDOM)
def test_random_panmat(engine, leaves, seed):
    pm = random_case(leaves, seed)
    _assert_same(engine.to_usher(pm), _usher_ref.to_usher(pm))


@pytest.mark.parametrize("leaves,seed", RANDOM[:1])
def test_block_mutations_change_nothing(engine, leaves, seed):
    want = engine.to_usher(random_case(leaves, seed))
    _assert_same(engine.to_usher(without_block_mutations(random_case(leaves, seed))), want)


def test_entries_per_node(engine):
    """0, 1, 63, 64, 65, 255, 256, 257 and two rounds plus five records on one node each."""
    pm = entry_count_case()
    _assert_same(engine.to_usher(pm), _usher_ref.to_usher(pm))


def test_run_straddles_a_round(engine):
    pm = straddle_case()
    _assert_same(engine.to_usher(pm), _usher_ref.to_usher(pm))


def test_position_varint_steps(engine):
    pm = position_case()
    _assert_same(engine.to_usher(pm), _usher_ref.to_usher(pm))


def test_list_length_varint_steps(engine):
    pm = list_length_case()
    _assert_same(engine.to_usher(pm), _usher_ref.to_usher(pm))


def test_codes_runs_and_the_sentinel(engine):
    pm = codes_case()
    _assert_same(engine.to_usher(pm), _usher_ref.to_usher(pm))


def test_cells_written_again_in_one_list(engine):
    pm = rewrite_case()
    _assert_same(engine.to_usher(pm), _usher_ref.to_usher(pm))


def test_preorder_is_not_id_order(engine, permuted):
    pm, want = permuted
    _assert_same(engine.to_usher(pm), want)


def _batches():
    return [v for k, v in phase_report() if k == "usher.batches"][-1]


def test_batches_of_one_node(engine, permuted):
    """4096 bytes: one node a batch where every node holds 60 records; the bytes never depend on the option."""
    engine.set_usher_batch_bytes(4096)
    try:
        pm = one_node_batches_case()
        phase_reset()
        _assert_same(engine.to_usher(pm), _usher_ref.to_usher(pm), "one node a batch")
        assert _batches() == pm.num_nodes
        pm, want = permuted
        phase_reset()
        _assert_same(engine.to_usher(pm), want, "258 nodes")
        assert 1 < _batches() <= 258
        pm = entry_count_case()
        _assert_same(engine.to_usher(pm), _usher_ref.to_usher(pm), "entry counts")
        pm = rewrite_case()
        _assert_same(engine.to_usher(pm), _usher_ref.to_usher(pm), "rewritten cells")
    finally:
        engine.set_usher_batch_bytes(1 << 30)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.set_usher_batch_bytes(4095)
    assert "rc=-1" in str(err.value)


def test_fd_into_a_pipe_and_a_file(engine, tmp_path):
    pm = long_text_case()
    want = _usher_ref.to_usher(pm)
    records = sum(map(len, _usher_ref.decode(want[0])[1]))
    r, w = os.pipe()
    chunks = []

    def drain():
        while True:
            b = os.read(r, 1 << 16)
            if not b:
                return
            chunks.append(b)

    t = threading.Thread(target=drain)
    t.start()
    try:
        length, count = engine.to_usher_fd(pm, w)
    finally:
        os.close(w)
        t.join()
        os.close(r)
    got = b"".join(chunks)
    assert len(want[0]) > 1 << 16   # (longer than the pipe's buffer)
    assert length == len(got) and count == records
    _assert_same((got, count), want, "pipe")
    fd = os.open(tmp_path / "out.pb", os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        length, count = engine.to_usher_fd(pm, fd)
    finally:
        os.close(fd)
    got = (tmp_path / "out.pb").read_bytes()
    assert length == len(got) and count == records
    _assert_same((got, count), want, "file")


def test_errors_leave_the_context_usable(engine):
    pm, want = substitution_case()
    for name, build in UNSUPPORTED.items():
        with pytest.raises(panman_amd.PanmanError) as err:
            engine.to_usher(build())
        assert "rc=-4" in str(err.value), name
        assert engine.to_usher(pm)[0] == want
    for name, build in ARG_ERRORS.items():
        with pytest.raises(panman_amd.PanmanError) as err:
            engine.to_usher(build())
        assert "rc=-1" in str(err.value), name
        assert engine.to_usher(pm)[0] == want
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.to_usher_fd(pm, -1)
    assert "rc=-1" in str(err.value)
    r, w = os.pipe()
    os.close(r)
    os.close(w)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.to_usher_fd(pm, w)   # a closed descriptor: the write fails
    assert "rc=-1" in str(err.value) and "write" in str(err.value)
    assert engine.to_usher(pm)[0] == want


def test_print_mutations_is_unchanged(engine):
    """The cell-to-column lookup and the element search moved into pm_cell.h: the same text."""
    pm = random_case(20, 2)
    assert engine.print_mutations(pm) == _mutations_ref.print_mutations(pm)
