"""pm_vcf on the GPU against the Python reference (tests/_vcf_ref.py, pinned to src/vcf.cpp:177-382
by tests/test_vcf_ref.py) run on the rows of Engine.fasta(pm, aligned=True), the oracle-pinned
path.  The ##fileDate line is masked; everything else is compared byte for byte."""
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

import panman_amd
from _panmat import parse_records, random_panmat
from _trees import names_for, parse_newick, random_tree, to_newick
from _vcf_cases import (GAPPED_CASES, MANY_ALTS_TIPS, MANY_RECORDS, ROUND_CASES, check_gapped_rows,
                        check_many_alts_rows, check_many_records_rows, check_no_record_rows, check_round_rows,
                        edge_rows, gapped_rows, many_alts_rows, many_records_rows, modal_reference, no_record_rows,
                        random_case, round_rows, star_panmat)
from _vcf_ref import mask_date, records, scan, vcf
from panman_amd.panmat import write_panman
from test_vcf_ref import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    e.close()


def _rows(engine, pm):
    return parse_records(engine.fasta(pm, True))


def _same_text(got, want):
    """got == want, failing with the first differing line alone (pytest's diff of two long texts
    that differ on many lines runs for minutes)."""
    if got == want:
        return
    g, w = got.split("\n"), want.split("\n")
    k = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
    x, y = (t[k] if k < len(t) else None for t in (g, w))
    at = None if x is None or y is None else next((i for i, (a, b) in enumerate(zip(x, y)) if a != b), min(len(x), len(y)))
    show = [t if t is None else t[max(0, (at or 0) - 60):(at or 0) + 60] for t in (x, y)]
    pytest.fail(f"line {k} (of {len(g)} / {len(w)}), byte {at}: "
                f"got {show[0]!r}, want {show[1]!r}", pytrace=False)


def _check(engine, pm, reference, rows=None):
    """Engine.vcf == the Python reference on the engine's aligned rows; returns (text, skipped)."""
    got_rows = _rows(engine, pm)
    if rows is not None:
        assert got_rows == rows
    want, wskip = vcf(got_rows, reference)
    got, gskip = engine.vcf(pm, reference)
    _same_text(mask_date(got), mask_date(want))
    assert got.split("\n")[1] == want.split("\n")[1]   # (the date itself, barring midnight)
    assert gskip == wskip
    return got, gskip


# ---- hand cases --------------------------------------------------------------------------

def _hand_trees():
    """The hand cases' rows as the tips of two one-block trees (four and five columns)."""
    trees = {}
    for ref, tip, _ in CASES:
        for row in (ref, tip):
            trees.setdefault(len(row), {})[f"row_{row}"] = row
    return trees


@pytest.mark.parametrize("case", range(len(CASES)))
def test_hand_case(engine, case):
    ref, tip, want = CASES[case]
    rows = _hand_trees()[len(ref)]
    pm = star_panmat(rows, "ACGTA"[:len(ref)])
    text, skipped = _check(engine, pm, f"row_{ref}", rows)
    assert skipped == 0
    # the case's own records, read back from the text
    samples = text.split("\n")[4].split("\t")[9:]
    col = 9 + samples.index(f"row_{tip}") if ref != tip else None
    found = []
    for line in text.split("\n")[5:-1]:
        f = line.split("\t")
        if col is not None and f[col] != "0":
            alt = f[4].split(",")[int(f[col]) - 1]
            found.append((int(f[1]), "" if f[3] == "." else f[3], "" if alt == "." else alt))
    assert found == want == scan(ref, tip)


def test_twelve_alts_give_two_digit_genotypes(engine):
    codes = "MGRSVTWYHKDB"
    rows = {"r": "ACGT"}
    rows.update({f"s{k:02d}": "A" + c + "GT" for k, c in enumerate(codes)})
    rows["same"] = "ACGT"
    text, _ = _check(engine, star_panmat(rows, "ACGT"), "r", rows)
    data = text.split("\n")[5:-1]
    assert len(data) == 1
    f = data[0].split("\t")
    assert f[:5] == ["r", "2", "0", "C", ",".join(sorted(codes))]
    assert sorted(f[9:]) == sorted([str(k) for k in range(13)]) and "12" in f[9:]


# ---- random PanMATs: blocks, rotation, inversion, strands ----------------------------------

@pytest.fixture(scope="module")
def big_case(engine):
    pm = random_case(300, 1)
    rows = _rows(engine, pm)
    return pm, rows, modal_reference(rows)


def _conditions(rows, reference):
    table, skipped = records(rows, reference)
    tips = len(rows) - 1
    assert 2 * (tips - skipped) >= tips and skipped >= 1
    assert sum(len(t) for alts in table.values() for t in alts.values()) >= 50


@pytest.mark.parametrize("leaves,seed", [(40, 3), (40, 12)])
def test_random_panmat(engine, leaves, seed):
    pm = random_case(leaves, seed)
    rows = _rows(engine, pm)
    reference = modal_reference(rows)
    _conditions(rows, reference)
    _check(engine, pm, reference)


def test_random_panmat_300(engine, big_case):
    pm, rows, reference = big_case
    _conditions(rows, reference)
    text, _ = _check(engine, pm, reference)
    assert any(len(g) > 1 for line in text.split("\n")[5:-1] for g in line.split("\t")[9:])


# ---- edges -----------------------------------------------------------------------------------

def check_edge_rows(rows, ref_name, columns):
    """The planted shapes are there: the reference's place in name order, gaps in its row, an
    event over columns 69|70 and 2047|2048 (unequal compared columns on both sides merge into
    one event), an event open at the last column."""
    order = sorted(rows, key=lambda s: s.encode())
    where = {"a": 0, "z": len(rows) - 1}.get(ref_name[0])
    assert order.index(ref_name) == where if where is not None else 0 < order.index(ref_name) < len(rows) - 1
    ref = rows[ref_name]
    assert "-" in ref[:columns - 1]   # POS != column
    tips = [r for n, r in rows.items() if n != ref_name]

    def differs(r, i):
        return r[i] != ref[i]

    for edge in (70, 2048):
        if columns > edge:
            assert any(differs(r, edge - 1) and differs(r, edge) for r in tips), edge
    assert any(differs(r, columns - 1) for r in tips)


@pytest.mark.parametrize("columns,tips,ref_name", [
    (69, 5, "a_ref"), (70, 5, "z_ref"), (71, 5, "t002_ref"), (140, 6, "a_ref"), (2047, 5, "z_ref"),
    (2048, 6, "t002_ref"), (2049, 5, "a_ref"), (71, 65, "t031_ref"), (2049, 257, "t100_ref")])
def test_edges(engine, columns, tips, ref_name):
    rows, cons = edge_rows(columns, tips, seed=columns + tips, ref_name=ref_name)
    check_edge_rows(rows, ref_name, columns)
    text, skipped = _check(engine, star_panmat(rows, cons), ref_name, rows)
    assert skipped == 0 and len(text.split("\n")) > 7


# ---- the kernels' rounds, waves and digits (the constants are named in tests/_vcf_cases.py) ------

def _small_batches(engine, pm, reference):
    engine.set_vcf_batch_bytes(4096)
    try:
        return engine.vcf(pm, reference)
    finally:
        engine.set_vcf_batch_bytes(1 << 30)


def _data(text):
    return [line.split("\t") for line in text.split("\n")[5:-1]]


@pytest.mark.parametrize("columns,ref_name,ref_gap", ROUND_CASES)
def test_round_edges(engine, columns, ref_name, ref_gap):
    """1024 = kVcfWaveWords (16) words: one k_vcf_classify wave; 4096 = 64 words: one k_vcf_starts
    round and one classify workgroup; 8192: two of them; every 2048 = 256 x kRefItems (8) columns
    one k_vcf_ref round."""
    rows, cons = round_rows(columns, seed=columns, ref_name=ref_name, ref_gap=ref_gap)
    check_round_rows(rows, ref_name, columns, ref_gap)
    text, skipped = _check(engine, star_panmat(rows, cons), ref_name, rows)
    assert skipped == 0 and len(_data(text)) > 7


@pytest.fixture(scope="module")
def round_case(engine):
    """The 8193-column case of ROUND_CASES with the reference last."""
    rows, cons = round_rows(8193, seed=8193, ref_name="z_ref")
    return star_panmat(rows, cons), rows, "z_ref"


@functools.lru_cache(maxsize=None)
def _gapped_case(columns, run, end):
    rows, cons = gapped_rows(columns, run, seed=run, end=end)
    check_gapped_rows(rows, columns, run, end)
    return star_panmat(rows, cons), rows


def _insert_lines(text, run):
    """The lines of the "insert" tip's insertions of `run` bases (the second run has min(run, 130))."""
    samples = text.split("\n")[4].split("\t")[9:]
    col = 9 + samples.index("insert")
    found = [f for f in _data(text) if any(len(a) == run + 1 for a in f[4].split(","))]
    assert len(found) == (2 if run <= 130 else 1)
    for f in found:
        assert len(f[3]) == 1 and f[col] != "0" and len(f[4].split(",")[int(f[col]) - 1]) == run + 1
    return ["\t".join(f) for f in found]


@pytest.mark.parametrize("columns,run,end", GAPPED_CASES)
def test_gapped_runs(engine, columns, run, end):
    """Runs of columns that are gaps in both rows below an event: within one word (63), over whole
    words (64, 65, 130) and over a whole k_vcf_starts round of 64 words (4096)."""
    pm, rows = _gapped_case(columns, run, end)
    text, skipped = _check(engine, pm, "ref", rows)
    assert skipped == 0
    _insert_lines(text, run)


def test_a_line_longer_than_the_batch(engine):
    columns, run, end = GAPPED_CASES[-1]
    pm, rows = _gapped_case(columns, run, end)
    want, wskip = _check(engine, pm, "ref", rows)
    got, gskip = _small_batches(engine, pm, "ref")
    _same_text(got, want)
    assert gskip == wskip
    assert run == 4096 and len(_insert_lines(got, run)[0]) > 4096   # (the batch bytes as set)


def test_three_digit_genotypes(engine):
    rows, cons = many_alts_rows(MANY_ALTS_TIPS)
    alts, samples, prefix = check_many_alts_rows(rows)
    pm = star_panmat(rows, cons)
    text, skipped = _check(engine, pm, "r", rows)
    data = _data(text)
    assert skipped == 0 and len(data) == 1 and len(data[0]) == 9 + samples
    assert len("\t".join(data[0][:9])) == prefix > 256
    assert {len(g) for g in data[0][9:9 + 256]} == {len(g) for g in data[0][9 + 256:]} == {1, 2, 3}
    assert max(int(g) for g in data[0][9:]) == alts
    got, gskip = _small_batches(engine, pm, "r")
    _same_text(got, text)
    assert gskip == skipped


def test_many_records_sorted_in_pieces(engine, monkeypatch):
    """The host's sort in 1, 2 and 8 pieces (PM_HOST_THREADS; kPiece = 1024 records), and its
    comparator on records that share the 64-bit key (POS, REF[:4])."""
    rows, cons = many_records_rows(*MANY_RECORDS)
    nrec, lines, _ = check_many_records_rows(rows)
    pm = star_panmat(rows, cons)
    want, _ = _check(engine, pm, "ref", rows)
    for threads in ("1", "2", "8"):
        monkeypatch.setenv("PM_HOST_THREADS", threads)
        panman_amd.phase_reset()
        got, skipped = engine.vcf(pm, "ref")
        report = dict(panman_amd.phase_report())
        _same_text(got, want)
        assert skipped == 0, threads
        assert (report["vcf.records"], report["vcf.lines"]) == (nrec, lines), threads
    assert len(_data(want)) == lines


def test_no_events_and_no_records(engine):
    cases = no_record_rows()
    check_no_record_rows(cases)
    for rows, cons, reference in cases:
        text, skipped = _check(engine, star_panmat(rows, cons), reference, rows)
        assert skipped == 0 and _data(text) == [] and len(text.split("\n")) == 6
    ref, tip, want = CASES[7]   # the context still serves an ordinary case
    rows = _hand_trees()[len(ref)]
    text, _ = _check(engine, star_panmat(rows, "ACGTA"[:len(ref)]), f"row_{ref}", rows)
    assert want and len(_data(text)) > 0


# ---- batches, descriptors ----------------------------------------------------------------------

def test_batches_give_the_same_text(engine, big_case):
    pm, _, reference = big_case
    want, wskip = engine.vcf(pm, reference)
    engine.set_vcf_batch_bytes(4096)
    try:
        got, gskip = engine.vcf(pm, reference)
    finally:
        engine.set_vcf_batch_bytes(1 << 30)
    assert got == want and gskip == wskip
    with pytest.raises(panman_amd.PanmanError):
        engine.set_vcf_batch_bytes(4095)


def _through_a_pipe(engine, pm, reference):
    want, wskip = engine.vcf(pm, reference)
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
        length, skipped = engine.vcf_fd(pm, reference, w)
    finally:
        os.close(w)
        t.join()
        os.close(r)
    got = b"".join(chunks)
    assert got == want.encode() and length == len(got) and skipped == wskip
    return want


def test_vcf_fd_into_a_pipe(engine, big_case):
    pm, _, reference = big_case
    _through_a_pipe(engine, pm, reference)


def test_vcf_fd_of_a_multi_round_row(engine, round_case):
    pm, rows, reference = round_case
    want = _through_a_pipe(engine, pm, reference)
    _same_text(mask_date(want), mask_date(vcf(rows, reference)[0]))


# ---- errors --------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable(engine):
    rows = {"r": "ACGT", "a": "ATGT"}
    pm = star_panmat(rows, "ACGT")
    for name in ("nobody", "root"):
        with pytest.raises(panman_amd.PanmanError) as err:
            engine.vcf(pm, name)
        assert "rc=-1" in str(err.value) and name in str(err.value)
    one = star_panmat({"r": "ACGT"}, "ACGT")
    with pytest.raises(panman_amd.PanmanError) as err:
        engine.vcf(one, "r")
    assert "rc=-1" in str(err.value) and "two tips" in str(err.value)
    assert _rows(engine, pm) == rows
    _check(engine, pm, "r", rows)


# ---- the C++ facade ------------------------------------------------------------------------------

PROGRAM = r"""
#include <fstream>
#include <iostream>
#include "panman_tree.hpp"
int main(int argc, char** argv) {
    try {
        panman_gpu::TreeGroup tg(std::string(argv[1]), 0);
        tg.trees[0].printVCFParallel(argv[2], std::cout);
    } catch (const panman_gpu::Error& e) {
        std::cerr << "Error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
"""


def test_facade_print_vcf_parallel(engine, tmp_path):
    rng = np.random.default_rng(32)   # (the PanMAT of test_facade.py)
    off, idx, root = random_tree(30, rng, max_children=3, unary=0.0)
    names, off, idx, root = parse_newick(to_newick(off, idx, root, names_for(off)))
    pm = random_panmat(rng, off, idx, root, names, blocks=4)
    rows = _rows(engine, pm)
    reference = modal_reference(rows)
    want, _ = engine.vcf(pm, reference)
    write_panman(str(tmp_path / "in.panman"), [pm])
    (tmp_path / "main.cpp").write_text(PROGRAM)
    lib = os.path.dirname(panman_amd.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "vcf"),
                    str(tmp_path / "main.cpp"), "-L", lib, "-l:libpanman_amd.so", f"-Wl,-rpath,{lib}"],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([str(tmp_path / "vcf"), "in.panman", reference], cwd=tmp_path, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert mask_date(r.stdout) == mask_date(want)
    bad = subprocess.run([str(tmp_path / "vcf"), "in.panman", "nobody"], cwd=tmp_path, capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode == 1 and "pm_vcf" in bad.stderr
