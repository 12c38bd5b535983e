"""Every builder of tests/_usher_cases.py holds the shape it claims, proved on the CPU from the
restatement's own output (tests/_usher_ref.py)."""
import pytest

import _usher_cases

CHECKS = sorted(n for n in dir(_usher_cases) if n.startswith("check_"))


@pytest.mark.parametrize("name", CHECKS)
def test_case_has_its_shape(name):
    getattr(_usher_cases, name)()


def test_every_builder_is_checked():
    assert len(CHECKS) == 10
