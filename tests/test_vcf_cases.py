"""The VCF case builders (tests/_vcf_cases.py) over the parameters of tests/test_gpu_vcf.py: the
shapes planted at the kernels' constants are present, checked without a GPU."""
import pytest

from _vcf_cases import (GAPPED_CASES, MANY_ALTS_TIPS, MANY_RECORDS, ROUND_CASES, ROUND_EDGES, STARTS_ROUND,
                        check_gapped_rows, check_many_alts_rows, check_many_records_rows, check_no_record_rows,
                        check_round_rows, gapped_rows, many_alts_rows, many_records_rows, no_record_rows,
                        round_rows)
from _vcf_ref import scan, vcf


@pytest.mark.parametrize("columns,ref_name,ref_gap", ROUND_CASES)
def test_round_rows(columns, ref_name, ref_gap):
    rows, cons = round_rows(columns, seed=columns, ref_name=ref_name, ref_gap=ref_gap)
    assert len(cons) == columns and "-" not in cons
    check_round_rows(rows, ref_name, columns, ref_gap)


def test_round_cases_cover_every_edge():
    columns = {c for c, _, _ in ROUND_CASES}
    assert columns == {e + d for e in ROUND_EDGES for d in (-1, 0, 1)}
    for e in ROUND_EDGES:   # the edge column exists from e + 1 columns on: every variant there
        assert {g for c, _, g in ROUND_CASES if c == e + 1} == {None, -1, 0}
    assert {n[0] for _, n, _ in ROUND_CASES} == {"a", "t", "z"}


@pytest.mark.parametrize("columns,run,end", GAPPED_CASES)
def test_gapped_rows(columns, run, end):
    rows, cons = gapped_rows(columns, run, seed=run, end=end)
    assert len(cons) == columns and "-" not in cons
    check_gapped_rows(rows, columns, run, end)
    # what the reference makes of the shapes: "start" opens an event at `end` anchored below the
    # run, "merge" has one record from below the run to `end`
    ref = rows["ref"]
    pos = sum(c != "-" for c in ref[:end]) + 1
    lo = end - run - 1
    assert (pos - 1, ref[lo] + ref[end], ref[lo]) in scan(ref, rows["start"])
    assert not any(p == pos for p, _, _ in scan(ref, rows["merge"]))
    assert any(p == pos - 1 and len(r) == 2 and len(a) == 2 for p, r, a in scan(ref, rows["merge"]))


def test_gapped_cases_cover_the_runs():
    assert [r for _, r, _ in GAPPED_CASES] == [63, 64, 65, 130, 4096]
    assert all(c >= 8200 and e == 2 * STARTS_ROUND for c, r, e in GAPPED_CASES if r == 4096)


def test_many_alts_rows():
    rows, _ = many_alts_rows(MANY_ALTS_TIPS)
    assert check_many_alts_rows(rows) == (150, 301, 466)
    data = vcf(rows, "r")[0].split("\n")[5:-1]
    assert len(data) == 1 and data[0].split("\t")[:4] == ["r", "2", "0", "CG"]


def test_many_records_rows():
    rows, _ = many_records_rows(*MANY_RECORDS)
    nrec, lines, shared = check_many_records_rows(rows)
    assert nrec // 8 >= 1024   # pm_vcf.cpp: the third doubling of the pieces needs R / 8 >= kPiece = 1024


def test_no_record_rows():
    cases = no_record_rows()
    check_no_record_rows(cases)
    for rows, _, reference in cases:
        assert len(vcf(rows, reference)[0].split("\n")) == 6   # the header's five lines
