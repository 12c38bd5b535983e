"""PanMATs for the VCF tests: one-block star trees whose aligned rows are given, and the
random block PanMATs (rotation, inversion, strands) of the replay tests.

The builders below `edge_rows` plant shapes at the constants of the kernels in pm_vcf.hip; each
has a check_* that proves from the rows alone (and, where the shape is a property of the
records, from tests/_vcf_ref.py) that the shapes are there."""
from __future__ import annotations

from collections import Counter

import numpy as np

from _panmat import random_panmat
from _trees import names_for, random_tree
from _vcf_ref import records, scan
from panman_amd.panmat import CODE, PanMAT

NSNPS, NSNPD = 3, 5   # NucMutationType: one-base substitution / deletion


def star_panmat(rows: dict[str, str], consensus: str) -> PanMAT:
    """A root with one tip per row; one block holding `consensus` (bases), every tip's aligned
    row made from it by one-base substitutions and deletions ('-')."""
    names = list(rows) + ["root"]
    n = len(rows)
    off = np.zeros(n + 2, np.int32)
    off[n + 1] = n
    pm = PanMAT(names, off, np.arange(n, dtype=np.int32), n)
    pm.add_block(0, consensus)
    pm.add_block_mut(n, 0, True, False)
    for v, row in enumerate(rows.values()):
        assert len(row) == len(consensus)
        for i, (c, ch) in enumerate(zip(consensus, row)):
            if ch == "-":
                pm.add_nuc_mut(v, 0, i, -1, NSNPD, [0])
            elif ch != c:
                pm.add_nuc_mut(v, 0, i, -1, NSNPS, [CODE[ch]])
    return pm


def random_case(leaves: int, seed: int) -> PanMAT:
    rng = np.random.default_rng(seed)
    off, idx, root = random_tree(leaves, rng, max_children=4, unary=0.1)
    return random_panmat(rng, off, idx, root, names_for(off), blocks=6)


def modal_reference(rows: dict[str, str]) -> str:
    """The first tip in byte order of the names whose row has the most common length."""
    length = Counter(len(r) for r in rows.values()).most_common(1)[0][0]
    return min((n for n in rows if len(rows[n]) == length), key=lambda s: s.encode())


def edge_rows(columns: int, tips: int, seed: int, ref_name: str = "ref"):
    """(rows, consensus) of one block of `columns` columns: the reference-to-be ("ref") has gaps
    (POS != column), every tip events across columns 69|70 and 2047|2048 where the block has
    them, an event open at the last column, and a few scattered ones."""
    rng = np.random.default_rng(seed)
    cons = "".join(rng.choice(list("ACGT"), size=columns))
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}

    def edit(row, i, kind):
        if 0 <= i < columns:
            row[i] = "-" if kind == 0 else other[cons[i]] if kind == 1 else cons[i]

    ref = list(cons)
    for i in (1, 5, 68, 69, 130, 2040, 2047, columns - 1):
        if tips % 2 or i != columns - 1:
            edit(ref, i, 0)
    rows = {ref_name: "".join(ref)}
    for k in range(tips):
        row = list(cons)
        for edge in (70, 2048):
            lo = edge - 1 - k % 3
            for i in range(lo, edge + 1 + (k // 3) % 3):
                edit(row, i, (i + k) % 3 if k % 7 else 1)
        edit(row, columns - 1, k % 2)
        if k % 4 == 0:
            edit(row, columns - 2, 0)
        for i in rng.integers(0, columns, size=3):
            edit(row, int(i), int(rng.integers(0, 2)))
        rows[f"t{k:03d}"] = "".join(row)
    return rows, cons


# ---- shapes at the kernels' constants (pm_vcf.hip) -----------------------------------------------

WORD = 64                      # columns of one plane word (one ballot of k_vcf_classify)
CLASSIFY_WAVE = 16 * WORD      # kVcfWaveWords = 16: columns of one k_vcf_classify wave (1024)
STARTS_ROUND = 64 * WORD       # 64 words per k_vcf_starts round (4096 columns); four classify
                               # waves, so also the columns of one k_vcf_classify workgroup
REF_ROUND = 256 * 8            # kRefItems = 8: columns of one k_vcf_ref scan round (2048)
ROUND_EDGES = (CLASSIFY_WAVE, STARTS_ROUND, 2 * STARTS_ROUND)

_OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def _skipped(ref: str, row: str, i: int) -> bool:
    return ref[i] == "-" and row[i] == "-"


def _equal(ref: str, row: str, i: int) -> bool:
    return ref[i] != "-" and ref[i] == row[i]


def _differs(ref: str, row: str, i: int) -> bool:
    return not _skipped(ref, row, i) and not _equal(ref, row, i)


def _before(ref: str, row: str, i: int) -> int:
    """The compared column before column i (-1: none)."""
    j = i - 1
    while j >= 0 and _skipped(ref, row, j):
        j -= 1
    return j


def _unlike(ref, cons: str, i: int) -> str:
    """A base for column i that differs from the reference's: a substitution, or an insertion
    where the reference has a gap."""
    return cons[i] if ref[i] == "-" else _OTHER[cons[i]]


def _scatter(rng, row, ref, cons: str, keep: set, edits: int):
    columns = len(cons)
    for i in rng.integers(0, columns, size=edits):
        i = int(i)
        if i not in keep:
            row[i] = "-" if rng.integers(0, 2) else _unlike(ref, cons, i)


def check_ref_place(rows, ref_name):
    """a*: first in the byte order of the names, z*: last, anything else: in between."""
    order = sorted(rows, key=lambda s: s.encode())
    where = {"a": 0, "z": len(rows) - 1}.get(ref_name[0])
    at = order.index(ref_name)
    assert at == where if where is not None else 0 < at < len(rows) - 1


def round_rows(columns: int, seed: int, ref_name: str = "ref", ref_gap: int | None = None):
    """(rows, consensus) of one block of `columns` columns with seven tips.  At every edge E of
    ROUND_EDGES below `columns`:
      t000  the compared column before E equal, column E unequal: an event starts exactly at E
      t001  the compared column before E and column E unequal: one event spans E
      t002  a deletion over [E-3, E+2]
      t003  ref_gap None: unequal at E-1 and equal at E (an event closes at E); otherwise a base
            where the reference has its gap (an insertion)
    ref_gap -1 / 0 puts a reference gap at E-1 / E (None: neither), so t000's carry comes through
    a skipped column / its event is an insertion.  The reference has two gaps in every 2048-column
    round (POS != column, every k_vcf_ref round carries another count), t004 and t005 have an
    event open at the last column, and every tip a few scattered edits away from the edges."""
    rng = np.random.default_rng(seed)
    cons = "".join(rng.choice(list("ACGT"), size=columns))
    edges = [e for e in ROUND_EDGES if columns > e]
    ref = list(cons)
    round_gaps = [i for r0 in range(0, columns, REF_ROUND) for i in (r0 + 5, r0 + 1000) if i < columns - 2]
    for i in round_gaps:
        ref[i] = "-"
    if ref_gap is not None:
        for e in edges:
            ref[e + ref_gap] = "-"
    keep = {i for e in edges for i in range(e - 4, e + 4)} | {columns - 2, columns - 1}
    rows = {ref_name: "".join(ref)}
    for k in range(7):
        row = list(ref)
        for n, i in enumerate(round_gaps):   # half of the reference's gaps hold a base here
            if (n + k) % 2:
                row[i] = cons[i]
        _scatter(rng, row, ref, cons, keep, 6)
        for e in edges:
            if k == 0:   # (a deletion behind the reference's gap: its anchor lies across the skipped column)
                row[e] = "-" if ref_gap == -1 else _unlike(ref, cons, e)
            elif k == 1:
                row[e - 1] = _unlike(ref, cons, e - 1)
                row[e] = _unlike(ref, cons, e)
            elif k == 2:
                for i in range(e - 3, min(e + 3, columns)):
                    row[i] = "-"
            elif k == 3:
                i = e - 1 if ref_gap is None else e + ref_gap
                row[i] = _unlike(ref, cons, i)
        if k == 4:
            row[columns - 1] = _unlike(ref, cons, columns - 1)
        elif k == 5:
            row[columns - 2] = "-"
            row[columns - 1] = "-" if ref[columns - 1] != "-" else cons[columns - 1]
        rows[f"t{k:03d}"] = "".join(row)
    return rows, cons


def check_round_rows(rows, ref_name, columns, ref_gap=None):
    check_ref_place(rows, ref_name)
    ref = rows[ref_name]
    tips = [r for n, r in rows.items() if n != ref_name]
    assert 6 <= len(tips) <= 8 and all(len(r) == columns for r in rows.values())
    for r0 in range(0, columns, REF_ROUND):
        if columns - r0 > 8:
            assert "-" in ref[r0:r0 + REF_ROUND], r0
    for e in ROUND_EDGES:
        if columns <= e:
            continue
        assert "-" in ref[:e - 4]   # POS != column at the edge
        near = [(r, _before(ref, r, e)) for r in tips if _differs(ref, r, e)]
        near = [(r, j) for r, j in near if j >= e - 2]
        assert any(_equal(ref, r, j) for r, j in near), e      # an event starts exactly at E
        assert any(_differs(ref, r, j) for r, j in near), e    # one event spans E
        window = slice(e - 3, min(e + 3, columns))
        width = window.stop - window.start
        assert sum(c != "-" for c in ref[window]) >= width - 1
        assert any(r[window] == "-" * width for r in tips), e
        if ref_gap is None:
            assert ref[e - 1] != "-" and ref[e] != "-"
            assert any(_differs(ref, r, e - 1) and _equal(ref, r, e) for r in tips), e
        else:
            assert ref[e + ref_gap] == "-" and any(r[e + ref_gap] != "-" for r in tips), e
    assert any(_differs(ref, r, columns - 1) for r in tips)


def gapped_rows(columns: int, run: int, seed: int, end: int = STARTS_ROUND):
    """(rows, consensus): the columns [end - run, end) are '-' in the reference ("ref") and in
    every tip but "insert", which has bases all through them (an insertion of `run` bases).
    "start" is equal at end - run - 1 and has a deletion at `end` (the event at `end` takes its
    carry-in and its anchor from below the run); "merge" is unequal at both (one event across the
    run).
    A second such run of min(run, 130) columns ends at column 2049, so that the event column is
    0 and 1 modulo 64; "plain" has scattered edits only."""
    e1, e2, run2 = end, REF_ROUND + 1, min(run, 130)
    assert e2 - run2 - 1 >= 0 and e2 + 2 < e1 - run - 2 and e1 + 2 < columns
    rng = np.random.default_rng(seed)
    cons = "".join(rng.choice(list("ACGT"), size=columns))
    ref = list(cons)
    keep = set()
    for e, n in ((e1, run), (e2, run2)):
        ref[e - n:e] = "-" * n
        keep |= set(range(e - n - 2, e + 3))
    rows = {"ref": "".join(ref)}
    for name in ("start", "merge", "insert", "plain"):
        row = list(ref)
        _scatter(rng, row, ref, cons, keep, 6)
        for e, n in ((e1, run), (e2, run2)):
            if name == "start":   # a deletion: REF and POS of its record come from below the run
                row[e] = "-"
            if name == "merge":
                row[e] = _OTHER[cons[e]]
            if name == "merge":
                row[e - n - 1] = _OTHER[cons[e - n - 1]]
            if name == "insert":
                row[e - n:e] = cons[e - n:e]
        rows[name] = "".join(row)
    return rows, cons


def check_gapped_rows(rows, columns, run, end=STARTS_ROUND):
    ref = rows["ref"]
    assert all(len(r) == columns for r in rows.values())
    assert end % WORD == 0 and (REF_ROUND + 1) % WORD == 1
    for e, n in ((end, run), (REF_ROUND + 1, min(run, 130))):
        lo = e - n - 1   # the compared column below the run
        assert ref[e - n:e] == "-" * n and ref[lo] != "-" and ref[e] != "-"
        for name, row in rows.items():
            if name not in ("ref", "insert"):
                assert row[e - n:e] == "-" * n, name
        start, merge, insert = rows["start"], rows["merge"], rows["insert"]
        assert _equal(ref, start, lo) and start[e] == "-" and _before(ref, start, e) == lo
        assert _differs(ref, merge, lo) and _differs(ref, merge, e) and _before(ref, merge, e) == lo
        assert "-" not in insert[e - n:e] and _equal(ref, insert, lo) and _equal(ref, insert, e)
        assert any(len(a) == n + 1 and len(r) == 1 for _, r, a in scan(ref, insert))
        if e % WORD == 0:   # every whole word of the run lies between the event and column `lo`
            assert e // WORD - (lo + WORD) // WORD == n // WORD
    if run >= STARTS_ROUND:   # a whole k_vcf_starts round without a compared column
        r0 = end - run
        assert r0 % STARTS_ROUND == 0 and run == STARTS_ROUND
        assert all(_skipped(ref, rows["start"], i) and _skipped(ref, rows["merge"], i) for i in range(r0, end))


_IUPAC = "ACGTRYSWKMBDHVN"


def many_alts_rows(tips: int, seed: int = 0):
    """(rows, consensus): reference "r" = ACGT, tips A c1 c2 T over 150 of the 196 pairs of
    ambiguity codes (c1 != C, c2 != G), and a tip equal to the reference: one line with 150 ALTs."""
    pairs = [a + b for a in _IUPAC if a != "C" for b in _IUPAC if b != "G"]
    rng = np.random.default_rng(seed)
    pick = [pairs[int(i)] for i in rng.permutation(len(pairs))[:150]]
    rows = {"r": "ACGT"}
    for k in range(tips):
        rows[f"s{k:03d}"] = "A" + pick[k % 150] + "T"
    rows["same"] = "ACGT"
    return rows, "ACGT"


def check_many_alts_rows(rows):
    """One line; genotypes of one, two and three digits among the first 256 samples (one scan
    round of k_vcf_text_write) and after them; 9 | 10 and 99 | 100 both occur; a prefix that
    takes the prefix copy loop round more than once."""
    table, skipped = records(rows, "r")
    assert skipped == 0 and list(table) == [(2, b"CG")]
    alts = sorted(table[(2, b"CG")])
    assert len(alts) >= 150
    samples = sorted((n for n in rows if n != "r"), key=lambda s: s.encode())
    assert len(samples) >= 301
    gt = dict.fromkeys(samples, 0)
    for k, a in enumerate(alts):
        for name in table[(2, b"CG")][a]:
            gt[name] = k + 1
    seq = [gt[s] for s in samples]
    assert 0 in seq and {9, 10, 99, 100} <= set(seq) and max(seq) == len(alts)
    for part in (seq[:256], seq[256:]):
        assert {len(str(g)) for g in part if g} == {1, 2, 3}
    prefix = "\t".join(["r", "2", "0", "CG", ",".join(a.decode() for a in alts), ".", ".", ".", "."])
    assert len(prefix) > 256
    return len(alts), len(samples), len(prefix)


def many_records_rows(columns: int, tips: int, seed: int):
    """(rows, consensus): a reference ("ref") without gaps; behind every tenth column each tip
    has a one-base substitution or a deletion of 4, 5 or 6 bases, drawn per tip and position, so
    that several REFs at one POS share their first four bytes and differ behind them."""
    rng = np.random.default_rng(seed)
    cons = "".join(rng.choice(list("ACGT"), size=columns))
    rows = {"ref": cons}
    for t in range(tips):
        row = list(cons)
        for p in range(0, columns - 8, 10):
            kind = int(rng.integers(0, 4))
            if kind == 0:
                row[p + 1] = "ACGT"[("ACGT".index(cons[p + 1]) + int(rng.integers(1, 4))) % 4]
            else:
                row[p + 1:p + 4 + kind] = "-" * (3 + kind)
        rows[f"t{t:02d}"] = "".join(row)
    return rows, cons


def check_many_records_rows(rows):
    """At least 8192 records (eight sort pieces of 1024) and at least 100 (POS, REF[:4]) keys
    that more than one line carries; returns (records, lines, shared keys)."""
    assert "-" not in rows["ref"]
    table, skipped = records(rows, "ref")
    nrec = sum(len(t) for alts in table.values() for t in alts.values())
    keys = Counter((pos, r[:4]) for pos, r in table)
    shared = sum(1 for v in keys.values() if v > 1)
    assert skipped == 0 and nrec >= 8192 and shared >= 100
    assert any(len(alts) > 1 for alts in table.values())
    return nrec, len(table), shared


def no_record_rows():
    """[(rows, consensus, reference)]: every tip equal to the reference (no event), and tips whose
    every event closes with REF == ALT (events, no record)."""
    rng = np.random.default_rng(7)
    cons = "".join(rng.choice(list("ACGT"), size=130))
    row = list(cons)
    for i in (0, 3, 63, 64, 65, 129):
        row[i] = "-"
    row = "".join(row)
    same = {"r": row, "a": row, "b": row, "c": row}
    units = 40
    swap = {"r": "AC-T" * units, "a": "A-CT" * units, "b": "AC-T" * units, "c": "A-CT" * units}
    return [(same, cons, "r"), (swap, "ACCT" * units, "r")]


def check_no_record_rows(cases):
    (same, _, ref0), (swap, _, ref1) = cases
    assert len(same) >= 3 and all(r == same[ref0] for r in same.values()) and "-" in same[ref0]
    assert records(same, ref0) == ({}, 0) and records(swap, ref1) == ({}, 0)
    ref = swap[ref1]
    assert any(_differs(ref, r, i) for r in swap.values() for i in range(len(ref)))   # events
    assert any(r == ref for n, r in swap.items() if n != ref1)


# The parameters of the GPU tests (tests/test_gpu_vcf.py); tests/test_vcf_cases.py runs every
# check over them without a GPU.
ROUND_CASES = [   # (columns, reference name, ref_gap): every edge - 1, edge, edge + 1
    (1023, "a_ref", None), (1024, "z_ref", -1), (1025, "t003_ref", 0),
    (4095, "z_ref", 0), (4096, "t003_ref", None), (4097, "a_ref", -1),
    (8191, "t003_ref", -1), (8192, "a_ref", 0), (8193, "z_ref", None),
    (1025, "a_ref", None), (1025, "z_ref", -1), (4097, "z_ref", None), (4097, "t003_ref", 0),
    (8193, "t003_ref", -1), (8193, "a_ref", 0)]
GAPPED_CASES = [   # (columns, run, end of the run)
    (4200, 63, STARTS_ROUND), (4200, 64, STARTS_ROUND), (4200, 65, STARTS_ROUND),
    (4200, 130, STARTS_ROUND), (8210, STARTS_ROUND, 2 * STARTS_ROUND)]
MANY_ALTS_TIPS = 300
MANY_RECORDS = (8300, 12, 5)   # (columns, tips, seed)
