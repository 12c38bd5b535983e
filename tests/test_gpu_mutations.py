"""pm_print_mutations on the GPU, byte for byte against the Python reference (tests/_mutations_ref.py,
pinned to src/panman.cpp:3699-4057 by tests/test_mutations_ref.py): the hand cases, random PanMATs,
and the kernels' edges (tests/_mutations_cases.py, each shape proved present by
tests/test_mutations_cases.py) -- entries per node around a wave and around k_mut_write's round, a
run that straddles a round's end, nodes with one section only between nodes with none, coordinates at
every digit count, root blocks of 63, 64, 65 and 257 columns on both strands and absent (the chunk
edges of the root map), 130 blocks, 258 nodes, names of 1 to 40 bytes; batches of one node, a pipe,
both error codes, the header, the facade."""
import os
import subprocess
import threading

import pytest

import panman_amd
import _mutations_ref
from _mutations_cases import (ARG_ERRORS, ENTRY_COUNTS, HAND, RANDOM, UNSUPPORTED, digits_case, entry_count_case, issue_case,
                              long_text_case, random_case, root_map_case, straddle_case, text_of)
from panman_amd.panmat import PanmanFile, write_panman

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def root_map():
    """(the PanMAT, the reference's result): computed once, read by three tests."""
    pm, _ = root_map_case()
    return pm, _mutations_ref.print_mutations(pm)


def _assert_same(got, want, where=()):
    """got == want for (text, odd substitutions), naming the first line that differs."""
    assert got[1] == want[1], (where, got[1], want[1])
    if got[0] == want[0]:
        return
    g, w = got[0].split("\n"), want[0].split("\n")
    for n in range(max(len(g), len(w))):
        a, b = (g[n] if n < len(g) else None), (w[n] if n < len(w) else None)
        if a == b:
            continue
        at = next((k for k in range(min(len(a or ""), len(b or ""))) if a[k] != b[k]), min(len(a or ""), len(b or "")))
        cut = lambda s: None if s is None else s[max(0, at - 30):at + 50]
        pytest.fail(f"{where}: line {n} differs at byte {at}: got {cut(a)!r} (of {len(a or '')}), want {cut(b)!r} "
                    f"(of {len(b or '')}); {len(g)} lines against {len(w)}", pytrace=False)


@pytest.mark.parametrize("name", list(HAND))
def test_hand_case(engine, name):
    pm, want, odd = HAND[name]()
    assert engine.print_mutations(pm) == (text_of(pm, want), odd)
    assert engine.print_mutations(pm) == _mutations_ref.print_mutations(pm)


@pytest.mark.parametrize("leaves,seed", RANDOM)
def test_random_panmat(engine, leaves, seed):
    pm = random_case(leaves, seed)
    _assert_same(engine.print_mutations(pm), _mutations_ref.print_mutations(pm))


def test_entries_per_node(engine):
    """0, 1, 63, 64, 65, 255, 256, 257 and two rounds plus five entries on one node each."""
    pm = entry_count_case()
    want = _mutations_ref.print_mutations(pm)
    lines = want[0].split("\n")
    for n in ENTRY_COUNTS:
        assert lines[3 * pm.index(f"e{n}")].count(" > ") == n
    _assert_same(engine.print_mutations(pm), want)


def test_run_straddles_a_round(engine):
    pm = straddle_case()
    _assert_same(engine.print_mutations(pm), _mutations_ref.print_mutations(pm))


def test_coordinate_digits(engine):
    pm, _ = digits_case()
    _assert_same(engine.print_mutations(pm), _mutations_ref.print_mutations(pm))


def test_root_map_edges_blocks_nodes_names(engine, root_map):
    pm, want = root_map
    _assert_same(engine.print_mutations(pm), want)


def test_batches_of_one_node(engine, root_map):
    """4096 bytes hold one node: 258 batches, and the node with two rounds of entries runs alone."""
    engine.set_mutations_batch_bytes(4096)
    try:
        pm, want = root_map
        _assert_same(engine.print_mutations(pm), want, "root map")
        pm = entry_count_case()
        _assert_same(engine.print_mutations(pm), _mutations_ref.print_mutations(pm), "entry counts")
        pm, hand, odd = issue_case()
        assert engine.print_mutations(pm) == (text_of(pm, hand), odd)
    finally:
        engine.set_mutations_batch_bytes(1 << 30)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.set_mutations_batch_bytes(4095)
    assert "rc=-1" in str(err.value)


def test_fd_into_a_pipe(engine):
    pm = long_text_case()
    want = _mutations_ref.print_mutations(pm)
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
        length, odd = engine.print_mutations_fd(pm, w)
    finally:
        os.close(w)
        t.join()
        os.close(r)
    got = b"".join(chunks)
    assert len(want[0]) > 1 << 16   # (longer than the pipe's buffer)
    assert length == len(got)
    _assert_same((got.decode(), odd), want, "pipe")


def test_errors_leave_the_context_usable(engine):
    pm, want, odd = issue_case()
    for name, build in UNSUPPORTED.items():
        with pytest.raises(panman_amd.PanmanError) as err:
            engine.print_mutations(build())
        assert "rc=-4" in str(err.value), name
        assert engine.print_mutations(pm) == (text_of(pm, want), odd)
    for name, build in ARG_ERRORS.items():
        with pytest.raises(panman_amd.PanmanError) as err:
            engine.print_mutations(build())
        assert "rc=-1" in str(err.value), name
        assert engine.print_mutations(pm) == (text_of(pm, want), odd)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.print_mutations_fd(pm, -1)
    assert "rc=-1" in str(err.value)
    r, w = os.pipe()
    os.close(r)
    os.close(w)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.print_mutations_fd(pm, w)   # a closed descriptor: the write fails
    assert "rc=-1" in str(err.value) and "write" in str(err.value)
    assert engine.print_mutations(pm) == (text_of(pm, want), odd)


# ---- the C++ facade ----------------------------------------------------------------------------------

PROGRAM = r"""
#include <iostream>
#include <sstream>
#include "panman_tree.hpp"
int main(int argc, char** argv) {
    try {
        panman_gpu::TreeGroup tg(std::string(argv[1]), 0);
        std::ostringstream text;
        tg.trees[0].printMutationsNew(text);
        std::cout << text.str();
    } catch (const panman_gpu::Error& e) {
        std::cerr << "Error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
"""


def test_facade(tmp_path):
    pm, _, _ = issue_case()
    write_panman(str(tmp_path / "in.panman"), [pm])
    f = PanmanFile(str(tmp_path / "in.panman"))
    want = _mutations_ref.print_mutations(f.to_panmat(0))   # a loaded tree numbers its nodes in Newick order
    f.close()
    lines = lambda text: sorted((l.split("\t")[0], l.split("\t")[2]) for l in text.split("\n") if l)   # (it also renames internal nodes)
    assert lines(want[0]) == lines(_mutations_ref.print_mutations(pm)[0])
    (tmp_path / "main.cpp").write_text(PROGRAM)
    lib = os.path.dirname(panman_amd.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "mut"),
                    str(tmp_path / "main.cpp"), "-L", lib, "-l:libpanman_amd.so", f"-Wl,-rpath,{lib}"],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([str(tmp_path / "mut"), "in.panman"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want[0]
