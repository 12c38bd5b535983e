"""The planted shapes of tests/_mutations_cases.py are there, proved from tests/_mutations_ref.py
alone (no GPU): every case runs, none is Unsupported or skipped, and between them they hold every
kind of entry and every skip rule."""
import pytest

import _mutations_cases as cases
import _mutations_ref


def test_hand_cases_hold_every_rule():
    tags = set()
    for build in cases.HAND.values():
        tags |= cases.tags_of(build()[0])
    assert {("S", "plain"), ("I", "plain"), ("I", "g"), ("D", "plain"), ("D", "g"), "D over -", "dropped", "S skipped: not held",
            "S skipped: old -", "old from the root", "parent not held", "odd", ("root", "held", "forward"),
            ("root", "held", "reverse"), ("root", "absent", "forward")} <= tags


def test_random_cases():
    cases.check_random_cases()


def test_entry_count_case():
    cases.check_entry_count_case()


def test_long_text_case():
    cases.check_long_text_case()


def test_straddle_case():
    cases.check_straddle_case()


def test_digits_case():
    cases.check_digits_case()


def test_root_map_case():
    cases.check_root_map_case()


@pytest.mark.parametrize("name", list(cases.ARG_ERRORS) + list(cases.UNSUPPORTED))
def test_error_cases_raise(name):
    build, exc = ((cases.ARG_ERRORS[name], _mutations_ref.ArgError) if name in cases.ARG_ERRORS
                  else (cases.UNSUPPORTED[name], _mutations_ref.Unsupported))
    with pytest.raises(exc):
        _mutations_ref.print_mutations(build())
