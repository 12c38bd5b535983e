"""GPU parity for FASTA replay (and reroot, which alone reads the rows of absent blocks) on the
planted inputs of tests/_replay_shapes.py: each sits on one of the replay kernels' capacities
or tile edges (pm_replay.hip: kDfsUnionCap, the 64-node chunk and its super-rounds, the LDS
ring, the 8-tile workgroup group, kOvrCap, kRestoreRanges, the DfsLds block table, kDfsPCap /
kDfsOCap, kFastNodes / kFastEdits, the formatter's grid and its wrap / rotation rules), as
test_replay_shapes.py asserts on the CPU with the census of the same builders.  Every case
checks through the phase log which kernel ran, that replay_flatten laid out the columns,
edits and leaf groups the census counts, and -- for the depth-first kernel -- that exactly
the (leaf, tile) rows the census predicts were rebuilt after an undo-stack overflow.

Reference: Tree::printFASTAUltraFast (src/fasta.cpp:1981-2099), Tree::reroot
(src/reroot.cpp:4-262), as restated by the oracle."""
import pytest
import torch

import panman_amd
from _panmat import tree_dump
from _replay_shapes import CASES, _c_names, built, records
from panman_amd._lib import phase_report, phase_reset

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_fasta_edge_vs_oracle(engine, oracle, name):
    case = CASES[name]
    pm, c = built(name)
    for aligned in (True, False):
        phase_reset()
        text = engine.fasta(pm, aligned)
        ph = dict(phase_report())
        assert ph["replay.max_depth"] == case.depth == c.max_depth, ph
        assert ph["replay.dfs_groups"] == (len(c.groups) if case.dfs else 0), ph    # 0: k_replay
        if case.groups is not None:
            assert ph["replay.dfs_groups"] == case.groups
        assert engine.replay_shape() == (len(c.leaves), c.columns, c.edits)
        if case.dfs:
            assert ph["replay.dfs_rebuilds"] == c.rebuilds(), ph
            if case.rebuild is not None:
                assert (ph["replay.dfs_rebuilds"] > 0) == case.rebuild, ph
        assert records(text) == records(oracle.fasta(pm, aligned)), aligned


@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n].reroot))
def test_reroot_restored_rows_vs_oracle(engine, oracle, name):
    """A block absent at a leaf prints as dashes (or nothing), whatever its row bytes hold;
    reroot reads those bytes (k_rows_to_codes), so a wrong restore shows here and only here."""
    case = CASES[name]
    pm, c = built(name)
    assert not any(m[1] != -1 for lst in pm.nuc_muts for m in lst)      # no secondary-block mutations
    for leaf in _c_names(pm, case.reroot):
        phase_reset()
        f = engine.reroot(pm, leaf)
        try:
            ph = dict(phase_report())
            assert ph["replay.max_depth"] == case.depth and (ph["replay.dfs_groups"] > 0) == case.dfs, ph
            assert tree_dump(f) == oracle.reroot(pm, leaf), leaf
        finally:
            f.close()


@pytest.mark.parametrize("aligned", [True, False])
def test_fasta_fd_streams_the_same_text_from_two_devices(engine, tmp_path, aligned):
    """pm_fasta_multi_fd with shards on two different devices: each shard's text streams from
    its own device (stage buffer and events created there) in leaf order."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    from panman_amd.synth import c5_panmat
    pm = c5_panmat(leaves=37, blocks=12, mean_len=900, seed=5)
    want = engine.fasta(pm, aligned).encode()
    path = tmp_path / "out.fa"
    for devices in ([0, 1], [1, 0, 1]):
        with open(path, "wb") as f:
            assert panman_amd.engine.fasta_multi_fd(pm, aligned, devices, f.fileno()) == len(want)
        assert path.read_bytes() == want, devices
