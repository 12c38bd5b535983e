"""The launchers' timer spans and run.* phase values over every input of _launch_matrix.py, read
through the public API, against tests/golden/run_launch_counts.json (recorded with
tools/run_launch_counts.py before launch_fitch / launch_sankoff shared pm_schedule.cpp): a launch
sequence that changes shows here, and tests/test_schedule_host.py holds the schedule to the same
file without a GPU."""
import pytest

import _launch_matrix as lm
import panman_amd

pytestmark = pytest.mark.gpu

TREES = lm.tree_set()


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    return lm.load_golden()


@pytest.mark.parametrize("k", range(len(TREES)), ids=[name for name, _ in TREES])
def test_launch_counts(engine, golden, k):
    name, tree = TREES[k]
    got = lm.walk_tree(engine, name, tree)
    assert len(got) == len(lm.CONFIGS)
    for entry, rows in got.items():
        assert rows == golden[entry], (entry, lm.COUNTS, rows, golden[entry])
