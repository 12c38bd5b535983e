"""The Python VCF reference (tests/_vcf_ref.py) pinned to src/vcf.cpp:177-382 by hand cases;
the GPU tests compare pm_vcf with it."""
import pytest

from _vcf_ref import mask_date, scan, vcf

# (reference row, tip row, records as (POS, REF, ALT))
CASES = [
    ("ACGT", "ACGT", []),
    ("ACGT", "ATGT", [(2, "C", "T")]),
    ("ACGT", "A-GT", [(1, "AC", "A")]),
    ("A-GT", "ACGT", [(1, "A", "AC")]),
    ("-CGT", "ACGT", [(1, "C", "AC")]),
    ("ACGT", "-CGT", [(1, "A", "")]),
    ("ACGT", "ACG-", [(3, "GT", "G")]),
    ("ACGT", "ATTT", [(2, "CG", "TT")]),
    ("AC-T", "A-CT", []),
    ("-C-T", "ACGT", [(1, "C", "AC"), (2, "T", "GT")]),
    ("AC-T", "ACGT", [(2, "C", "CG")]),
    ("A-CT", "A--T", [(1, "AC", "A")]),
    ("ACGT", "A-TT", [(1, "ACG", "AT")]),
    ("AC-GT", "A-CTT", [(3, "G", "T")]),
    # columns that are gaps in both rows, inside and in front of an event
    ("AC-GT", "AT-TT", [(2, "CG", "TT")]),                   # one event across the both-gap column
    ("A--CT", "A---T", [(1, "AC", "A")]),                    # the anchor from before a both-gap run
    ("AC--T", "AC-GT", [(2, "C", "CG")]),                    # ... and an insertion behind it
    ("-C-GT", "AC-TT", [(1, "C", "AC"), (2, "G", "T")]),     # after the leading insertion the strings are
    ("-C-GT", "AC--T", [(1, "C", "AC"), (2, "G", "")]),      # empty: no anchor across the both-gap column
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_hand_case(case):
    ref, tip, want = CASES[case]
    assert scan(ref, tip) == want


def test_whole_text_one_line():
    text, skipped = vcf({"r": "ACGT", "s1": "ATGT", "s2": "AGGT", "s3": "ACGT"}, "r")
    lines = text.split("\n")
    assert skipped == 0 and lines[-1] == ""
    assert lines[0] == "##fileformat=VCFv4.2" and lines[1].startswith("##fileDate=")
    assert lines[2] == "##source=PanMATv2.0-beta" and lines[3] == "##reference=r"
    assert lines[4] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\ts3"
    assert text.endswith("FORMAT\ts1\ts2\ts3\nr\t2\t0\tC\tG,T\t.\t.\t.\t.\t2\t1\t0\n")
    assert len(lines) == 7


def test_two_refs_at_one_pos():
    text, _ = vcf({"r": "ACGT", "a": "ATGT", "b": "AT-T"}, "r")
    data = text.split("\n")[5:-1]
    assert data == ["r\t2\t0\tC\tT\t.\t.\t.\t.\t1\t0", "r\t2\t1\tCG\tT\t.\t.\t.\t.\t0\t1"]


def test_empty_alt_prints_a_dot():
    text, _ = vcf({"r": "ACGT", "a": "-CGT"}, "r")
    assert text.split("\n")[5] == "r\t1\t0\tA\t.\t.\t.\t.\t.\t1"


def test_empty_ref_prints_a_dot():
    # an insertion open at the last column with nothing before it: REF is empty
    text, _ = vcf({"r": "-C-", "a": "ACG", "b": "-C-", "c": "-A-"}, "r")
    data = text.split("\n")[5:-1]
    assert data[0].split("\t")[:5] == ["r", "1", "0", "C", "A,AC"]
    assert data[1].split("\t")[:5] == ["r", "2", "1", ".", "G"]
    assert data[0].split("\t")[9:] == ["2", "0", "1"] and data[1].split("\t")[9:] == ["1", "0", "0"]


def test_skipped_tip_is_a_zero_column():
    text, skipped = vcf({"r": "ACGT", "a": "ATGT", "b": "ACG"}, "r")
    assert skipped == 1
    assert text.split("\n")[5] == "r\t2\t0\tC\tT\t.\t.\t.\t.\t1\t0"


def test_mask_date():
    text, _ = vcf({"r": "A", "a": "C"}, "r")
    assert mask_date(text).split("\n")[1] == "##fileDate="
