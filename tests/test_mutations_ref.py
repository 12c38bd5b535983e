"""tests/_mutations_ref.py pinned to Tree::printMutationsNew (src/panman.cpp:3699-4057) by
hand-derived expectations: the issue's case byte for byte, a reverse-strand root block, a block the
root does not hold, the root's base printed for a reverse parent, a parent without the block, the
dropped single-base types, a kept substitution over a '-', and both error classes."""
import pytest

import _mutations_ref
from _mutations_cases import ARG_ERRORS, HAND, UNSUPPORTED, issue_case, reverse_root_case, text_of


@pytest.mark.parametrize("name", list(HAND))
def test_hand_case(name):
    pm, want, odd = HAND[name]()
    assert _mutations_ref.print_mutations(pm) == (text_of(pm, want), odd)


def test_issue_case_bytes():
    pm, _, _ = issue_case()
    assert _mutations_ref.print_mutations(pm)[0] == (
        "Substitutions:\tr\t\nInsertions:\tr\t\nDeletions:\tr\t\n"
        "Substitutions:\ta\t > C2G > G3T\nInsertions:\ta\t > g5T > g5T\nDeletions:\ta\t > 7G > 8T\n"
        "Substitutions:\tb\t\nInsertions:\tb\t > 4A\nDeletions:\tb\t\n"
        "Substitutions:\tc\t > G2A > -10T\nInsertions:\tc\t\nDeletions:\tc\t > g5T\n")


def test_reverse_root_map():
    """The coordinates of every cell of a reverse block, written out: the sentinel first (a gap),
    then positions descending, a position's main character before its slots."""
    pm, _, _ = reverse_root_case()
    root = _mutations_ref.NodeState(pm, [0], 0, {0})
    coord, gap = _mutations_ref.root_map(root)
    assert coord == {(0, 4, -1): 0, (0, 3, -1): 0, (0, 2, -1): 1, (0, 2, 0): 2, (0, 1, -1): 3, (0, 0, -1): 4}
    assert [cell for cell, g in gap.items() if g] == [(0, 4, -1)]


def test_absent_block_keeps_its_consensus():
    """A node that does not hold a block: the path's nucleotide mutations are not applied to it."""
    pm, _, _ = HAND["issue"]()
    b = pm.index("b")
    state = _mutations_ref.NodeState(pm, [0, b], 0, {0})
    assert not state.held[0] and "".join(main for main, _ in state.seq[0]) == "ACGTACGTACx"
    assert state.seq[0][4][1] == ["-", "-"]


@pytest.mark.parametrize("name", list(ARG_ERRORS))
def test_arg_error(name):
    with pytest.raises(_mutations_ref.ArgError):
        _mutations_ref.print_mutations(ARG_ERRORS[name]())


@pytest.mark.parametrize("name", list(UNSUPPORTED))
def test_unsupported(name):
    with pytest.raises(_mutations_ref.Unsupported):
        _mutations_ref.print_mutations(UNSUPPORTED[name]())
