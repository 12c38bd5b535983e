"""The amino-acid case builders (tests/_aa_cases.py) over the parameters of tests/test_gpu_aa.py:
the shapes planted at the kernels' constants are present and every listed window is defined,
checked without a GPU."""
import pytest

import _aa_ref
from _aa_cases import (MANY_BLOCKS_WINDOWS, WIDE_CASES, WIDE_ERRORS, WIDE_IDS, WIDE_STRANDS, WIDE_WINDOWS,
                       check_five_digit_case, check_many_blocks_case, check_many_nodes_case, check_wide_case,
                       check_wide_errors, five_digit_case, many_blocks_case, many_nodes_case, wide_case, wide_required)


def _defined(pm, start, end):
    """The reference's result of a window that must be defined: neither ArgError nor Unsupported, a root codon."""
    want = _aa_ref.aa(pm, start, end)
    assert want[1] >= 1 and want[0].startswith("node_id\taa_mutations\n"), (start, end)
    return want


@pytest.mark.parametrize("strands,ids,slots", WIDE_CASES)
def test_wide_case(strands, ids, slots):
    pm = wide_case(strands, ids, slots)
    windows = WIDE_WINDOWS[strands, slots]
    assert len(set(windows)) == len(windows)
    check_wide_case(pm, strands, ids, slots, windows)   # (a) to (f)
    lines = set()
    for start, end in windows:
        text = _defined(pm, start, end)[0]
        assert "\nsame\t" not in text and "\nroot\t" not in text
        lines |= {line.partition("\t")[0] for line in text.split("\n")[1:-1]}
    # every mutated node prints a line in some window, the internal node (the derived tip's row) among them
    assert lines == set(pm.names) - {"root", "same"}


@pytest.mark.parametrize("strands,ids,slots", WIDE_CASES)
def test_wide_errors(strands, ids, slots):
    pm = wide_case(strands, ids, slots)
    windows = WIDE_ERRORS[strands, slots]
    check_wide_errors(pm, strands, slots, windows)
    for start, end in windows:
        with pytest.raises(_aa_ref.ArgError, match="root window"):
            _aa_ref.aa(pm, start, end)
    assert not set(windows) & set(WIDE_WINDOWS[strands, slots])


def test_wide_cases_cover_the_ground():
    assert {(s, k) for s, _, k in WIDE_CASES} == set(WIDE_WINDOWS) == set(WIDE_ERRORS)
    assert WIDE_STRANDS == ["+-+", "-+-", "---"] and WIDE_IDS == [(0, 1, 2), (0, 2, 5)]
    need = set().union(*(wide_required(*case) for case in WIDE_CASES))
    assert {t[0] for t in need} == set("abcdef")
    assert len(wide_required("+-+", (0, 2, 5), True)) == len(need)   # one case needs everything
    # the issue's probe windows that this layout defines
    assert {(63, 127), (64, 330), (65, 700), (255, 511), (256, 600), (5, 1070), (722, 730), (361, 420), (362, 700)} \
        <= set(WIDE_WINDOWS["+-+", True])
    assert {(0, 64), (63, 127), (64, 330), (255, 511), (257, 1000), (5, 1070), (722, 730), (725, 1000)} <= set(WIDE_WINDOWS["-+-", True])


def test_many_blocks_case():
    pm = many_blocks_case()
    check_many_blocks_case(pm, MANY_BLOCKS_WINDOWS)
    assert {(439, 462), (448, 451), (890, 902), (3, 895), (434, 898)} <= set(MANY_BLOCKS_WINDOWS)
    kinds = set()
    for start, end in MANY_BLOCKS_WINDOWS:
        text = _defined(pm, start, end)[0]
        kinds |= {line.partition("\t")[0] for line in text.split("\n")[1:-1]}
    assert kinds == {"snps", "lost", "shift"}


def test_five_digit_case():
    pm, start, end = five_digit_case()
    check_five_digit_case(_defined(pm, start, end))


def test_many_nodes_case():
    pm, start, end = many_nodes_case()
    check_many_nodes_case(pm)
    text, ref_codons, unlocated = _defined(pm, start, end)
    assert ref_codons == 12 and unlocated == 0 and text.count("\n") > 200
