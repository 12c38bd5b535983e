"""pm_maf on the GPU, byte for byte against the Python reference (tests/_maf_ref.py, pinned to
src/maf.cpp:68-188 by tests/test_maf_ref.py): hand cases, random PanMATs, and the kernels'
edges -- item widths of k_maf_size, the body chunk of k_maf_write, misaligned blocks and text,
the start scan's rounds, digit widths, tip counts, batches, a pipe, errors, the facade, the CLI."""
import os
import subprocess
import threading

import pytest

import panman_amd
from _maf_cases import HAND, hand_panmat, random_case, star
from _maf_ref import maf
from panman_amd.panmat import PanMAT, PanmanFile, write_panman
from test_maf_ref import ROUND_TRIP, round_trip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "panmanUtils")
CHUNK = 4096   # kMafChunk (pm_internal.h): body bytes per workgroup of k_maf_write

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def big_case():
    pm = random_case(60, 1)
    return pm, maf(pm)


def _names(n):
    return [f"t{k:03d}" for k in range(n)]


def _fields(text):
    return [line.split("\t") for line in text.split("\n") if line.startswith("s\t")]


@pytest.mark.parametrize("name", list(HAND))
def test_hand_case(engine, name):
    case, want = HAND[name]
    assert engine.maf(hand_panmat(case)) == want


@pytest.mark.parametrize("leaves,seed", ROUND_TRIP)
def test_random_panmat(engine, leaves, seed):
    pm = random_case(leaves, seed)
    want = maf(pm)
    strands = {f[4] for f in _fields(want)}
    assert strands == {"+", "-"} and len(_fields(want)) < 6 * leaves   # both strands, absent blocks
    got = engine.maf(pm)
    assert got == want
    compared, _ = round_trip(pm, engine.fasta(pm, False), got)
    assert compared >= leaves * 0.9


# ---- widths: the item classes of k_maf_size (4, 16, 64 lanes) and the writer's chunk -----------

@pytest.mark.parametrize("width", [2, 15, 16, 17, 49, 50, 63, 64, 65, 241, 242, 255, 256, 257,
                                   CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_single_block_width(engine, width):
    pm = star(_names(5), [width], seed=width)
    assert engine.maf(pm) == maf(pm)


@pytest.mark.parametrize("width", [2, 16, 17, 64, 257, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
@pytest.mark.parametrize("before", [[3], [5, 7, 9]])
def test_misaligned_block(engine, before, width):
    """Odd-width blocks in front: blk_lo of the last block is off the 16-byte grid."""
    pm = star(_names(4), before + [width], seed=width)
    assert sum(before) % 16 != 0
    assert engine.maf(pm) == maf(pm)


def test_name_lengths_shift_the_text(engine):
    """Names of 1 and 40 bytes: every body starts at another offset of the 16-byte grid."""
    names = ["a", "b" * 40, "cc", "d" * 17, "e" * 5, "f" * 31]
    pm = star(names, [3, 2 * CHUNK + 1, 70, 300], seed=5)
    want = maf(pm)
    offsets, at = set(), 0
    for line in want.split("\n"):
        if line.startswith("s\t"):
            offsets.add((at + line.rindex("\t") + 1) % 16)
        at += len(line) + 1
    assert len(offsets) >= 8
    assert engine.maf(pm) == want


# ---- the start scan: rounds of 64 print positions, rotation, inversion, circular offsets -------

@pytest.mark.parametrize("blocks", [65, 130])
def test_many_blocks(engine, blocks):
    widths = [2 + (7 * b) % 23 for b in range(blocks)]
    pm = star(_names(9), widths, seed=blocks)
    for v in range(9):
        if v % 3 == 0:
            pm.rotation[v] = 1 + 40 * v
        if v % 3 == 1:
            pm.inverted[v] = 1
        if v % 2 == 0:
            pm.circular[v] = 17 * v
    for v in (2, 5):   # a tip that lost some blocks: the rotation counts held blocks only
        for b in range(0, blocks, 4):
            pm.add_block_mut(v, b, False, False)
    want = maf(pm)
    starts = [int(f[2]) for f in _fields(want)]
    assert max(starts) > 64 * 5 and len(_fields(want)) < 9 * blocks
    assert engine.maf(pm) == want


def test_digit_widths(engine):
    """Starts, sizes and srcSize on both sides of 9 | 10, 99 | 100 and 999 | 1000: blocks of 9, 1,
    90, 900, 10, 100 and 1000 bases, sizes a little apart from tip to tip (star), and tips that
    hold only the first two, three or four blocks."""
    bases = [9, 1, 90, 900, 10, 100, 1000]
    pm = star(_names(48), [b + 3 if b >= 3 else b + 1 for b in bases], seed=7)
    for v in range(48):
        keep = (2, 3, 4, 7)[v % 4]
        for b in range(keep, 7):
            pm.add_block_mut(v, b, False, False)
    want = maf(pm)
    f = _fields(want)
    for col, what in ((2, "start"), (3, "size"), (5, "srcSize")):
        values = [int(x[col]) for x in f]
        for k in (10, 100, 1000):
            assert any(k - 4 <= v < k for v in values) and any(k <= v < k + 4 for v in values), (what, k)
    assert engine.maf(pm) == want


@pytest.mark.parametrize("tips", [2, 65, 257])
def test_tip_counts(engine, tips):
    pm = star(_names(tips), [3, 20, 300], seed=tips)
    assert engine.maf(pm) == maf(pm)


# ---- batches, descriptors ------------------------------------------------------------------------

def test_batches_give_the_same_text(engine, big_case):
    pm, want = big_case
    paragraphs = want.split("\na\n")
    assert max(len(p) for p in paragraphs) > 4096   # that group's "a" and closing line: different batches
    engine.set_maf_batch_bytes(4096)
    try:
        got = engine.maf(pm)
    finally:
        engine.set_maf_batch_bytes(1 << 30)
    assert got == want
    with pytest.raises(panman_amd.PanmanError):
        engine.set_maf_batch_bytes(4095)


def test_a_line_longer_than_the_batch(engine):
    pm = star(_names(3), [3, 2 * CHUNK + 1], seed=1)
    engine.set_maf_batch_bytes(4096)
    try:
        got = engine.maf(pm)
    finally:
        engine.set_maf_batch_bytes(1 << 30)
    assert got == maf(pm)


def test_maf_fd_into_a_pipe(engine, big_case):
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
        length = engine.maf_fd(pm, w)
    finally:
        os.close(w)
        t.join()
        os.close(r)
    got = b"".join(chunks)
    assert got == want.encode() and length == len(got)


# ---- errors --------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable(engine):
    case, want = HAND["A"]
    pm = hand_panmat(case)
    secondary = hand_panmat(case)
    secondary.add_nuc_mut(secondary.index("t1"), 0, 1, -1, 3, [8], secondary=0)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.maf(secondary)
    assert "rc=-4" in str(err.value) and "secondary" in str(err.value)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.maf(PanMAT([], [0], [], 0))   # no node, so no tip
    assert "rc=-1" in str(err.value)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.maf_fd(pm, -1)
    assert "rc=-1" in str(err.value)
    r, w = os.pipe()
    os.close(r)
    os.close(w)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.maf_fd(pm, w)   # a closed descriptor: the write fails
    assert "rc=-1" in str(err.value) and "MAF write" in str(err.value)
    assert engine.maf(pm) == want


# ---- the C++ facade and the command line -----------------------------------------------------------

PROGRAM = r"""
#include <iostream>
#include "panman_tree.hpp"
int main(int argc, char** argv) {
    try {
        panman_gpu::TreeGroup tg(std::string(argv[1]), 0);
        tg.trees[0].printMAF(std::cout);
    } catch (const panman_gpu::Error& e) {
        std::cerr << "Error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
"""


def _written(path, panmats):
    """Write the PanMATs; the reference texts of the file's trees.  A loaded tree numbers its
    nodes in Newick order, so inside a block its lines come in another order than the
    list-built PanMAT's: the same lines, the same paragraphs."""
    write_panman(path, panmats)
    f = PanmanFile(path)
    texts = [maf(f.to_panmat(i)) for i in range(len(panmats))]
    f.close()
    for pm, text in zip(panmats, texts):
        ours = maf(pm)
        assert sorted(text.split("\n")) == sorted(ours.split("\n"))
        assert [sorted(p.split("\n")) for p in text.split("\n\n")] == [sorted(p.split("\n")) for p in ours.split("\n\n")]
    return texts


def test_facade_print_maf(big_case, tmp_path):
    pm, _ = big_case
    want, = _written(str(tmp_path / "in.panman"), [pm])
    (tmp_path / "main.cpp").write_text(PROGRAM)
    lib = os.path.dirname(panman_amd.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "maf"),
                    str(tmp_path / "main.cpp"), "-L", lib, "-l:libpanman_amd.so", f"-Wl,-rpath,{lib}"],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([str(tmp_path / "maf"), "in.panman"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want


def test_cli_maf(big_case, tmp_path):
    pm, _ = big_case
    path = str(tmp_path / "in.panman")
    first, want = _written(path, [random_case(12, 9), pm])
    r = subprocess.run([CLI, "-I", path, "--maf", "--treeID", "1", "-o", "out"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "info" / "out.maf").read() == want
    assert "\nMAF execution time: " in r.stdout and r.stdout.rstrip().endswith("nanoseconds")
    r = subprocess.run([CLI, path, "-w"], cwd=tmp_path, capture_output=True, text=True, timeout=300)   # tree 0, stdout
    assert r.returncode == 0, r.stderr
    assert first + "\nMAF execution time: " in r.stdout
    r = subprocess.run([CLI, path, "--maf", "-d", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "TreeID out of range" in r.stderr
