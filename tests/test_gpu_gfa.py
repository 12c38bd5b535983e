"""pm_gfa on the GPU, byte for byte against the Python reference (tests/_gfa_ref.py, pinned to
src/gfa.cpp:3-500 by tests/test_gfa_ref.py): hand cases, random PanMATs, and the kernels' edges --
chunk widths on both strands, misaligned blocks, empty chunks and empty paths, block 0's start
collision between the strands, shared and merged
nodes, id digit widths, tip counts, the whole-block branch, batches, a pipe, errors, the facade,
the CLI."""
import os
import subprocess
import threading

import numpy as np
import pytest

import panman_amd
from _gfa_cases import HAND, hand_panmat, names, random_case, star
from _gfa_ref import gfa, gfa_to_sequences
from _maf_ref import _parents, _path, block_state
from panman_amd.panmat import PanMAT, PanmanFile, write_panman

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "panmanUtils")
WIDTHS = [1, 2, 31, 32, 33, 63, 64, 65, 97]   # columns of a block around the 32-column chunk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def big_case():
    pm = random_case(60, 1)
    return pm, gfa(pm)


def _paths(text):
    return {f[1]: f[2] for f in (line.split("\t") for line in text.split("\n")) if f[0] == "P"}


def _root_star(n, seqs, gaps=()):
    """A root with n tips; the blocks of `seqs` inserted at the root."""
    off = np.zeros(n + 2, np.int32)
    off[n + 1] = n
    pm = PanMAT(names(n) + ["root"], off, np.arange(n, dtype=np.int32), n)
    for b, seq in enumerate(seqs):
        pm.add_block(b, seq)
        pm.add_block_mut(n, b, True, False)
    for b, slots in gaps:
        pm.add_gaps(b, slots)
    return pm


@pytest.mark.parametrize("name", list(HAND))
def test_hand_case(engine, name):
    case, want = HAND[name]
    assert engine.gfa(hand_panmat(case)) == want


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_panmat(engine, seed):
    pm = random_case(60, seed)
    want = gfa(pm)
    steps = [s for p in _paths(want).values() for s in p.split(",") if s]
    assert {s[-1] for s in steps} == {"+", "-"}   # both strands
    parent = _parents(pm)
    held = [block_state(pm, _path(pm, parent, t), b)[0] for t in pm.leaves() for b in range(6)]
    assert any(held) and not all(held)            # absent blocks
    assert engine.gfa(pm) == want


# ---- chunk edges: forward chunks anchored at the block's start, reverse ones at its end ------------

@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("width", WIDTHS)
def test_single_block_width(engine, width, reverse):
    pm = star(names(5), [width], seed=width, gaps=width != 33, reverse=[(2, 0)] if reverse else [])
    want = gfa(pm)
    assert ("-" in "".join(_paths(want).values())) == (reverse and width > 1)
    assert engine.gfa(pm) == want


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("before", [[3], [5, 7, 9]])
def test_misaligned_block(engine, before, width, reverse):
    """Odd-width blocks in front: blk_lo of the last block is off every alignment grid."""
    last = len(before)
    pm = star(names(4), before + [width], seed=width, reverse=[(1, last), (3, 0)] if reverse else [])
    assert sum(before) % 4 != 0
    assert engine.gfa(pm) == gfa(pm)


def test_middle_chunk_all_gaps_in_one_tip(engine):
    """Columns: 32 bases, 32 gap slots, 32 bases, the sentinel.  Tip 0 leaves the slots empty: its
    middle chunk makes no node and no step; the other tips fill a slot each."""
    rng = np.random.default_rng(4)
    pm = _root_star(4, ["".join(rng.choice(list("ACGT"), size=64))], gaps=[(0, [(32, 32)])])
    for v in (1, 2, 3):
        pm.add_nuc_mut(v, 0, 32, 7 * v, 4, [1 << (v % 4)])
    pm.add_nuc_mut(0, 0, 3, -1, 3, [1])
    want = gfa(pm)
    lengths = [len(p.split(",")) for p in _paths(want).values()]
    assert lengths[0] < min(lengths[1:])
    assert engine.gfa(pm) == want


def test_block_0_start_collision_between_strands(engine):
    """Block 0 of 64 columns with column 32 a gap slot: the forward chunk of columns 32..63 starts
    at (0, 31, 1) and the reverse strand's first chunk, the same columns, at (-0, 31, 1) -- the
    same tuple (gfa.cpp:253).  t001 walks the block in reverse and reuses the node t000 made on
    the forward strand, and the path filter then drops that step.  Block 1 is built the same and
    does not collide: -1 is no forward block."""
    rng = np.random.default_rng(12)
    pm = _root_star(2, ["".join(rng.choice(list("ACGT"), size=61)) for _ in range(2)], gaps=[(0, [(31, 2)]), (1, [(31, 2)])])
    pm.add_nuc_mut(0, 0, 0, -1, 3, [1 if pm.blocks[0][1][0] >> 28 != 1 else 2])   # t000 changes base 0: A, or C for an A
    pm.add_block_mut(1, 0, False, True)
    pm.add_block_mut(1, 1, False, True)
    want = gfa(pm)
    spelled = gfa_to_sequences(want)
    assert len(spelled["t000"]) == 122 and len(spelled["t001"]) == 122 - 30   # the 30 bases of columns 32..63 are lost
    assert engine.gfa(pm) == want


def test_a_tip_holding_no_block(engine):
    pm = star(names(4), [40, 70], seed=3)
    for b in range(2):
        pm.add_block_mut(2, b, False, False)
    want = gfa(pm)
    assert "P\tt002\t\t*\n" in want
    assert engine.gfa(pm) == want


def test_identical_tips_and_a_single_tip(engine):
    rng = np.random.default_rng(6)
    pm = _root_star(2, ["".join(rng.choice(list("ACGT"), size=100))])
    pm.add_nuc_mut(2, 0, 50, -1, 3, [2])   # at the root: both tips carry it
    want = gfa(pm)
    paths = list(_paths(want).values())
    assert paths[0] == paths[1] == "1+,2+,3+" and want.count("S\t") == 3   # four chunks, the middle two merged
    assert engine.gfa(pm) == want
    one = star(names(1), [70], seed=2)
    assert engine.gfa(one) == gfa(one)


@pytest.fixture(scope="module")
def many_nodes():
    """1200 blocks of 8 bases, odd ones on the reverse strand, so no chain merges (the strands of
    neighbours differ): more than 1000 printed ids and "P" lines of more than 4096 bytes."""
    pm = star(names(2), [9] * 1200, seed=11, gaps=False, reverse=[(t, b) for t in range(2) for b in range(1, 1200, 2)])
    return pm, gfa(pm)


def test_id_digit_widths(engine, many_nodes):
    pm, want = many_nodes
    ids = {int(s[:-1]) for p in _paths(want).values() for s in p.split(",")}
    for k in (10, 100, 1000):
        assert {k - 1, k} <= ids
    assert engine.gfa(pm) == want


@pytest.mark.parametrize("tips", [1, 2, 65, 257])
def test_tip_counts(engine, tips):
    pm = star(names(tips), [3, 20, 300], seed=tips, reverse=[(t, 2) for t in range(0, tips, 5)])
    assert engine.gfa(pm) == gfa(pm)


# ---- the whole-block branch ----------------------------------------------------------------------------

def test_whole_blocks(engine):
    rng = np.random.default_rng(8)
    pm = _root_star(9, ["".join(rng.choice(list("ACGT"), size=int(n))) for n in (5, 8, 9, 16, 3, 7)])
    pm.block_muts[9] = [m for m in pm.block_muts[9] if m[0] != 4]   # block 4: nobody holds it
    for v in range(9):
        if v % 2:
            pm.add_block_mut(v, v % 4, False, False)
        if v % 3 == 0:
            pm.add_block_mut(v, 5, False, True)   # an inversion clears here
        if v == 7:
            pm.add_block_mut(v, 4, True, False)
            pm.add_block_mut(v, 4, False, True)
    want = gfa(pm)
    lines = want.split("\n")
    assert not want.startswith("H") and sum(line.startswith("S\t") for line in lines) == 6
    links = [(int(f[1]), int(f[3])) for f in (line.split("\t") for line in lines) if f[0] == "L"]
    assert links == sorted(links) and len(links) > 4                          # ascending (from, to)
    assert list(_paths(want)) == names(9)                                    # tip order
    assert all("4+" not in p and "-" not in p for p in _paths(want).values())
    assert engine.gfa(pm) == want


def test_whole_blocks_id_without_a_block(engine):
    """A held id equal to the number of blocks indexes the presence list's spare entry; it is no
    block's, and the reference's map lookup prints it as 0 (gfa.cpp:107, :112)."""
    pm = hand_panmat(HAND["E_whole_blocks_with_an_inversion"][0])
    pm.add_block_mut(pm.index("t1"), 4, True, False)
    want = gfa(pm)
    assert "L\t2\t+\t0\t+\t0M\n" in want and "P\tt1\t0+,1+,2+,0+\t*\n" in want
    assert engine.gfa(pm) == want


# ---- batches, descriptors ----------------------------------------------------------------------------------

def test_batches_give_the_same_text(engine):
    pm = star(names(257), [3, 20, 300], seed=257, reverse=[(t, 2) for t in range(0, 257, 5)])
    want = gfa(pm)
    assert sum(len(p) for p in _paths(want).values()) > 2 * 4096   # several batches of "P" lines
    engine.set_gfa_batch_bytes(4096)
    try:
        got = engine.gfa(pm)
    finally:
        engine.set_gfa_batch_bytes(1 << 30)
    assert got == want
    with pytest.raises(panman_amd.PanmanError):
        engine.set_gfa_batch_bytes(4095)


def test_a_line_longer_than_the_batch(engine, many_nodes):
    pm, want = many_nodes
    assert min(len(p) for p in _paths(want).values()) > 4096
    engine.set_gfa_batch_bytes(4096)
    try:
        got = engine.gfa(pm)
    finally:
        engine.set_gfa_batch_bytes(1 << 30)
    assert got == want


def test_gfa_fd_into_a_pipe(engine, big_case):
    pm, want = big_case
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
        length = engine.gfa_fd(pm, w)
    finally:
        os.close(w)
        t.join()
        os.close(r)
    got = b"".join(chunks)
    assert got == want.encode() and length == len(got)


# ---- errors ------------------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable(engine):
    case, want = HAND["A_two_tips_one_chunk"]
    pm = hand_panmat(case)
    secondary = hand_panmat(case)
    secondary.add_nuc_mut(secondary.index("t1"), 0, 1, -1, 3, [8], secondary=0)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.gfa(secondary)
    assert "rc=-4" in str(err.value) and "secondary" in str(err.value)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.gfa(PanMAT([], [0], [], 0))   # no node, so no tip
    assert "rc=-1" in str(err.value)
    beyond = hand_panmat(HAND["E_whole_blocks_with_an_inversion"][0])
    beyond.add_block_mut(beyond.index("t1"), 5, True, False)   # four blocks: ids up to 4 index the presence list
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.gfa(beyond)
    assert "rc=-1" in str(err.value)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.gfa_fd(pm, -1)
    assert "rc=-1" in str(err.value)
    r, w = os.pipe()
    os.close(r)
    os.close(w)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.gfa_fd(pm, w)   # a closed descriptor: the write fails
    assert "rc=-1" in str(err.value) and "GFA write" in str(err.value)
    assert engine.gfa(pm) == want


# ---- the C++ facade and the command line ---------------------------------------------------------------------

PROGRAM = r"""
#include <iostream>
#include "panman_tree.hpp"
int main(int argc, char** argv) {
    try {
        panman_gpu::TreeGroup tg(std::string(argv[1]), 0);
        tg.trees[0].convertToGFA(std::cout);
    } catch (const panman_gpu::Error& e) {
        std::cerr << "Error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
"""


def _written(path, panmats):
    """Write the PanMATs; the reference texts of the file's trees.  A loaded tree numbers its
    nodes in Newick order, so its tips run in another order than the list-built PanMAT's and the
    ids differ: the reference reads the loaded tree."""
    write_panman(path, panmats)
    f = PanmanFile(path)
    texts = [gfa(f.to_panmat(i)) for i in range(len(panmats))]
    f.close()
    for pm, text in zip(panmats, texts):
        assert sorted(_paths(text)) == sorted(_paths(gfa(pm)))
    return texts


def test_facade_convert_to_gfa(big_case, tmp_path):
    pm, _ = big_case
    want, = _written(str(tmp_path / "in.panman"), [pm])
    (tmp_path / "main.cpp").write_text(PROGRAM)
    lib = os.path.dirname(panman_amd.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "gfa"),
                    str(tmp_path / "main.cpp"), "-L", lib, "-l:libpanman_amd.so", f"-Wl,-rpath,{lib}"],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([str(tmp_path / "gfa"), "in.panman"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want


def test_cli_gfa(big_case, tmp_path):
    pm, _ = big_case
    path = str(tmp_path / "in.panman")
    first, want = _written(path, [random_case(12, 9), pm])
    r = subprocess.run([CLI, "-I", path, "--gfa", "--treeID", "1", "-o", "out"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "not part of the GPU path" not in r.stderr and "unrecognised option" not in r.stderr
    assert open(tmp_path / "info" / "out.gfa").read() == want
    assert "GFA generation time: " in r.stdout and r.stdout.rstrip().endswith("nanoseconds")
    r = subprocess.run([CLI, path, "-g"], cwd=tmp_path, capture_output=True, text=True, timeout=300)   # tree 0, stdout
    assert r.returncode == 0, r.stderr
    assert first + "GFA generation time: " in r.stdout
    r = subprocess.run([CLI, path, "--gfa", "-d", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "TreeID out of range" in r.stderr
    assert "not part of the GPU path" not in r.stderr and "unrecognised option" not in r.stderr
