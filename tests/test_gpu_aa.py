"""pm_aa on the GPU, byte for byte against the Python reference (tests/_aa_ref.py, pinned to
src/aaTrans.cpp:185-304 by tests/test_aa_ref.py): the hand cases, random PanMATs, and the kernels'
edges -- window lengths around a wave and around k_aa_codons' round of cells, codons that straddle
a round, a node without codons, four-digit indices, names of different lengths, batches, a pipe,
errors, the header, the facade; then the shapes of tests/_aa_cases.py that cross a kernel constant
away from the single forward block: blocks of 300 bases on both strands with gap slots, 129 blocks,
258 nodes, five-digit indices."""
import os
import re
import subprocess
import threading

import pytest

import panman_amd
import _aa_ref
from _aa_cases import (HAND, MANY_BLOCKS_WINDOWS, ND, RANDOM, SNP_DEL, WIDE_CASES, WIDE_ERRORS, WIDE_WINDOWS,
                       check_five_digit_case, five_digit_case, issue_case, many_blocks_case, many_nodes_case, random_case,
                       star, text_of, unsupported_case, wide_case)
from panman_amd.panmat import PanmanFile, write_panman
from test_aa_ref import _window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND = 256   # kAaChunk (pm_internal.h): window cells per round of k_aa_codons' workgroup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def long_star():
    """One block of 700 bases under 6 leaves; u and v delete bases so that a codon straddles the
    first round's end as 1 + 2 and as 2 + 1 bases with dashes between; z deletes everything."""
    edits = [("u", 10, SNP_DEL, [0]), ("u", 254, ND, [0, 0, 0]),
             ("v", 10, SNP_DEL, [0]), ("v", 255, ND, [0, 0])]
    edits += [("z", p, ND, [0] * 5) for p in range(0, 700, 5)]
    return star(["s", "t" * 23, "u", "v", "w" * 7, "z"], 700, seed=1, edits=edits)


@pytest.mark.parametrize("name", list(HAND))
def test_hand_case(engine, name):
    pm, start, end, want, ref_codons = HAND[name]()
    assert engine.aa(pm, start, end) == (text_of(pm, want), ref_codons, 0)
    assert engine.aa(pm, start, end) == _aa_ref.aa(pm, start, end)


@pytest.mark.parametrize("leaves,k,seed", RANDOM)
def test_random_panmat(engine, leaves, k, seed):
    pm, start, end = random_case(leaves, k, seed)
    assert engine.aa(pm, start, end) == _aa_ref.aa(pm, start, end)   # (never unsupported: equal block lengths)


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_random_panmat_every_start(engine, seed):
    """One random PanMAT, a spread of windows: starts and ends on slots and in every block."""
    pm, _, _ = random_case(30, 9, seed)
    from _aa_cases import lengths
    low = min(lengths(pm))
    compared = 0
    for start in range(0, low - 1, max(1, low // 7)):
        for end in (start + 1, start + 4, (start + low) // 2 + 1, low - 1):
            if not start < end < low:
                continue
            try:
                want = _aa_ref.aa(pm, start, end)
            except _aa_ref.ArgError:
                with pytest.raises(panman_amd.PanmanError) as err:
                    engine.aa(pm, start, end)
                assert "rc=-1" in str(err.value)
                continue
            assert engine.aa(pm, start, end) == want, (start, end)
            compared += 1
    assert compared >= 10


def test_many_blocks(engine):
    """130 blocks: k_aa_locate's block search carries over rounds of 64, and a window spans a hundred blocks."""
    from _aa_cases import lengths
    pm, _, _ = random_case(30, 4, 31, blocks=130)
    low = min(lengths(pm))
    assert low > 4 * 80
    compared = 0
    for start, end in ((3, low - 2), (2 * low // 3, low - 1), (low // 2, low // 2 + 30), (low - 9, low - 1)):
        try:
            want = _aa_ref.aa(pm, start, end)
        except _aa_ref.ArgError:
            with pytest.raises(panman_amd.PanmanError):
                engine.aa(pm, start, end)
            continue
        assert engine.aa(pm, start, end) == want, (start, end)
        compared += 1
    assert compared >= 3


# ---- window lengths: a wave of k_aa_locate, a round of k_aa_codons ------------------------------------

@pytest.mark.parametrize("length", [1, 2, 3, 63, 64, 65, 3 * 64 - 1, 3 * 64 + 1, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 5])
def test_window_length(engine, long_star, length):
    for start in (0, 7):
        want = _aa_ref.aa(long_star, start, start + length)
        assert want[1] == length // 3
        assert engine.aa(long_star, start, start + length) == want


def test_codon_straddles_a_round(engine, long_star):
    pm = long_star
    for name, parts in (("u", [253, 257, 258]), ("v", [253, 254, 257])):
        w = _window(pm, name, 0, 600)
        _, starts, ends = _aa_ref.codons(w)
        c = [k for k in range(len(starts)) if starts[k] < ROUND <= ends[k]]
        assert len(c) == 1 and [i for i in range(starts[c[0]], ends[c[0]] + 1) if w[i] != "-"] == parts
    want = _aa_ref.aa(pm, 0, 600)
    assert "\nu\t" in want[0] and "\nv\t" in want[0]
    assert engine.aa(pm, 0, 600) == want


def test_node_without_codons(engine, long_star):
    want = _aa_ref.aa(long_star, 0, 90)
    assert want[2] == 1                      # z holds no base: not located, no line
    assert engine.aa(long_star, 0, 90) == want
    pm, _, _, _, _ = issue_case()            # c's end wraps onto its start: an empty window, every codon deleted
    want = _aa_ref.aa(pm, 0, 10)
    assert "c\tD:0;D:1;D:2;\n" in want[0]
    assert engine.aa(pm, 0, 10) == want
    assert engine.aa(pm, 13, 14) == ("", 0, 0)   # the root without a codon: no header


def test_four_digit_indices_and_name_lengths(engine):
    names = ["a", "b" * 40, "cc", "d" * 17]
    edits = [("a", 3009, ND, [0] * 6), ("cc", 2, SNP_DEL, [0])]
    pm = star(names, 3100, seed=9, edits=edits)
    want = _aa_ref.aa(pm, 0, 3050)
    assert want[1] >= 1000 and re.search(r"[SI]:1\d{3}:", want[0]) and "D:1003;D:1004;" in want[0]
    assert engine.aa(pm, 0, 3050) == want


# ---- batches, descriptors ------------------------------------------------------------------------

def test_batches_give_the_same_text(engine):
    pm, start, end = random_case(30, 64, 8)
    want = _aa_ref.aa(pm, start, end)
    assert want[0].count("\n") > 20 and end - start > 150   # one node's tables fill a 4096-byte batch
    engine.set_aa_batch_bytes(4096)
    try:
        got = engine.aa(pm, start, end)
    finally:
        engine.set_aa_batch_bytes(1 << 30)
    assert got == want and engine.aa(pm, start, end) == want
    with pytest.raises(panman_amd.PanmanError):
        engine.set_aa_batch_bytes(4095)


def _through_a_pipe(engine, pm, start, end):
    """engine.aa_fd into a pipe that a thread drains: (the bytes read, aa_fd's result)."""
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
        result = engine.aa_fd(pm, start, end, w)
    finally:
        os.close(w)
        t.join()
        os.close(r)
    return b"".join(chunks), result


def test_aa_fd_into_a_pipe(engine, long_star):
    want = _aa_ref.aa(long_star, 3, 640)
    got, (length, ref_codons, unlocated) = _through_a_pipe(engine, long_star, 3, 640)
    assert got == want[0].encode() and (length, ref_codons, unlocated) == (len(got), want[1], want[2])


# ---- the rounds, waves and carries of the kernels (the builders and their checks: tests/_aa_cases.py,
# ---- tests/test_aa_cases.py) ---------------------------------------------------------------------------

def _assert_same(got, want, where=()):
    """got == want for (text, root codons, unlocated), naming the first line that differs and its
    node (pytest's own diff of two 100 KB strings takes minutes)."""
    assert got[1:] == want[1:], (where, got[1:], want[1:])
    if got[0] == want[0]:
        return
    g, w = got[0].split("\n"), want[0].split("\n")
    for n in range(max(len(g), len(w))):
        a, b = (g[n] if n < len(g) else None), (w[n] if n < len(w) else None)
        if a == b:
            continue
        at = next((k for k in range(min(len(a or ""), len(b or ""))) if a[k] != b[k]), min(len(a or ""), len(b or "")))
        cut = lambda s: None if s is None else s[max(0, at - 30):at + 50]
        node = (b if b is not None else a).partition("\t")[0]
        pytest.fail(f"{where}: line {n} (node {node!r}) differs at byte {at}: got {cut(a)!r} (of {len(a or '')}), "
                    f"want {cut(b)!r} (of {len(b or '')}); {len(g)} lines against {len(w)}", pytrace=False)


@pytest.mark.parametrize("strands,ids,slots", WIDE_CASES)
def test_wide_windows(engine, strands, ids, slots):
    """Blocks wider than a round of both kernels on both strands: second and later rounds of the
    backward rank-select and of the backward walk, rounds with unwalked cells before walked ones,
    an absent block of 300 dashes inside a codon, ids that hold no block, coordinates that wrap
    on one node alone."""
    pm = wide_case(strands, ids, slots)
    for start, end in WIDE_WINDOWS[strands, slots]:
        _assert_same(engine.aa(pm, start, end), _aa_ref.aa(pm, start, end), (start, end))


@pytest.mark.parametrize("strands,slots", list(WIDE_ERRORS))
def test_wide_error_windows(engine, strands, slots):
    """The root's window never reaches its end -- on a slot the walk leaves out beyond the first
    round, or wrapped in front of the start: rc=-1, and the context goes on."""
    pm = wide_case(strands, (0, 2, 5), slots)
    for start, end in WIDE_ERRORS[strands, slots]:
        with pytest.raises(panman_amd.PanmanError) as err:
            engine.aa(pm, start, end)
        assert "rc=-1" in str(err.value), (start, end)
    start, end = WIDE_WINDOWS[strands, slots][0]
    _assert_same(engine.aa(pm, start, end), _aa_ref.aa(pm, start, end), (start, end))


def test_block_scan_round_edges(engine):
    """129 blocks: starts and ends in blocks 63 | 64 | 65 and 127 | 128, the last lane of a round of
    k_aa_locate's block scan and the first of the next."""
    pm = many_blocks_case()
    for start, end in MANY_BLOCKS_WINDOWS:
        _assert_same(engine.aa(pm, start, end), _aa_ref.aa(pm, start, end), (start, end))


def test_five_digit_indices(engine):
    """10,020 root codons: S:1dddd and I:10020 entries, a line of more than 65,536 bytes -- also
    through a pipe, whose buffer is shorter than that line."""
    pm, start, end = five_digit_case()
    want = _aa_ref.aa(pm, start, end)
    check_five_digit_case(want)
    _assert_same(engine.aa(pm, start, end), want)
    got, (length, ref_codons, unlocated) = _through_a_pipe(engine, pm, start, end)
    _assert_same((got.decode(), ref_codons, unlocated), want, "pipe")
    assert length == len(got)


def test_many_nodes(engine):
    """258 nodes: k_aa_locate's last workgroup has two of its four waves."""
    pm, start, end = many_nodes_case()
    _assert_same(engine.aa(pm, start, end), _aa_ref.aa(pm, start, end))


def test_wide_batches(engine):
    """Batches of one node over a wide case: "same" prints nothing between two nodes that do, so
    a batch without bytes lies between two with bytes."""
    strands, ids, slots = "+-+", (0, 2, 5), True
    pm = wide_case(strands, ids, slots)
    assert pm.names.index("lost") + 1 == pm.names.index("same") == pm.names.index("flip_middle") - 1
    between = 0
    engine.set_aa_batch_bytes(4096)
    try:
        for start, end in WIDE_WINDOWS[strands, slots]:
            want = _aa_ref.aa(pm, start, end)
            if end - start > 150:   # one node's tables fill a 4096-byte batch
                between += "\nlost\t" in want[0] and "\nflip_middle\t" in want[0] and "\nsame\t" not in want[0]
            _assert_same(engine.aa(pm, start, end), want, (start, end))
    finally:
        engine.set_aa_batch_bytes(1 << 30)
    assert between >= 5


# ---- errors --------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable(engine):
    pm, start, end, want, ref_codons = issue_case()
    secondary, _, _, _, _ = issue_case()
    secondary.add_nuc_mut(secondary.index("a"), 0, 1, -1, 3, [8], secondary=0)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.aa(secondary, start, end)
    assert "rc=-4" in str(err.value) and "secondary" in str(err.value)
    for s, e in ((9, 9), (9, 3)):
        with pytest.raises(panman_amd.PanmanError) as err:
            engine.aa(pm, s, e)
        assert "rc=-1" in str(err.value) and "End coordinate must be greater than start" in str(err.value)
    for s, e in ((0, 26), (-1, 5)):
        with pytest.raises(panman_amd.PanmanError) as err:
            engine.aa(pm, s, e)
        assert "rc=-1" in str(err.value) and "coordinates out of range" in str(err.value)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.aa(pm, 2, 13)     # the end wraps in front of the start: the root's window is ERROR
    assert "rc=-1" in str(err.value)
    bad, s, e = unsupported_case()
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.aa(bad, s, e)
    assert "rc=-4" in str(err.value)
    assert engine.aa(bad, 0, 6) == _aa_ref.aa(bad, 0, 6)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.aa_fd(pm, start, end, -1)
    assert "rc=-1" in str(err.value)
    r, w = os.pipe()
    os.close(r)
    os.close(w)
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.aa_fd(pm, start, end, w)   # a closed descriptor: the write fails
    assert "rc=-1" in str(err.value) and "write" in str(err.value)
    assert engine.aa(pm, 14, 23) == _aa_ref.aa(pm, 14, 23)   # c is not located: counted
    assert engine.aa(pm, start, end) == (text_of(pm, want), ref_codons, 0)


def test_header_names_the_option():
    text = open(os.path.join(ROOT, "include", "panman_gpu.h")).read()
    assert "#define PM_OPT_AA_BATCH_BYTES 25\n" in text
    assert "int pm_aa(" in text and "int pm_aa_fd(" in text


# ---- the C++ facade ----------------------------------------------------------------------------------

PROGRAM = r"""
#include <iostream>
#include <sstream>
#include "panman_tree.hpp"
int main(int argc, char** argv) {
    try {
        panman_gpu::TreeGroup tg(std::string(argv[1]), 0);
        std::ostringstream text;
        tg.trees[0].extractAminoAcidTranslations(text, 0, 9);
        std::cout << text.str();
    } catch (const panman_gpu::Error& e) {
        std::cerr << "Error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
"""


def test_facade(tmp_path):
    pm, start, end, _, ref_codons = issue_case()
    write_panman(str(tmp_path / "in.panman"), [pm])
    f = PanmanFile(str(tmp_path / "in.panman"))
    want = _aa_ref.aa(f.to_panmat(0), start, end)     # a loaded tree numbers its nodes in Newick order
    f.close()
    strings = lambda text: sorted(line.partition("\t")[2] for line in text.split("\n"))   # (it also renames internal nodes)
    assert strings(want[0]) == strings(_aa_ref.aa(pm, start, end)[0])
    (tmp_path / "main.cpp").write_text(PROGRAM)
    lib = os.path.dirname(panman_amd.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "aa"),
                    str(tmp_path / "main.cpp"), "-L", lib, "-l:libpanman_amd.so", f"-Wl,-rpath,{lib}"],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([str(tmp_path / "aa"), "in.panman"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == f"{ref_codons} {ref_codons} {ref_codons}\n" + want[0]
