"""bench.py's driver contract: a plain run prints the headline line only (`--steps` timed steps,
`ms_per_step`), and `--dump-outputs DIR` writes what a caller of the timed path receives --
checked at a reduced size against the same workload run through the Engine API."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_rows_is_fixed_sorted_and_in_range():
    import bench
    assert np.array_equal(bench.sample_rows(5), np.arange(5))
    assert np.array_equal(bench.sample_rows(bench.DUMP_ROWS), np.arange(bench.DUMP_ROWS))
    n = 3 * bench.DUMP_ROWS + 1
    rows = bench.sample_rows(n)
    assert rows.shape == (bench.DUMP_ROWS,) and rows.min() >= 0 and rows.max() < n
    assert (np.diff(rows) >= 0).all()
    assert np.array_equal(rows, bench.sample_rows(n))


@pytest.mark.parametrize("argv, env, full", [
    (["--gpus", "1", "--steps", "20", "--warmup", "5"], None, False),
    (["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", "d"], None, False),
    (["--no-cpu", "--with", "none", "--e2e"], None, False),   # they choose among --full's parts, no more
    (["--full"], None, True),
    (["--gpus", "1"], "1", True),    # the environment default the tools/ scripts export
    (["--gpus", "1"], "0", False),
    (["--gpus", "1"], "", False),
])
def test_full_is_off_unless_asked_for(monkeypatch, argv, env, full):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    if env is None:
        monkeypatch.delenv(bench.FULL_ENV, raising=False)
    else:
        monkeypatch.setenv(bench.FULL_ENV, env)
    assert bench.parse().full is full


def test_tool_scripts_that_run_the_benchmark_ask_for_the_full_line():
    """Every tools/*.sh that runs bench.py reads keys of the full line (roofline, commands,
    secondary) or profiles the full run: each names --full or exports the environment default."""
    import glob
    import re

    import bench
    scripts = [p for p in sorted(glob.glob(os.path.join(ROOT, "tools", "*.sh")))
               if re.search(r"^[^#\n]*python3? bench\.py", open(p).read(), re.M)]
    assert len(scripts) >= 20
    for p in scripts:
        text = open(p).read()
        calls = re.findall(r"^[^#\n]*python3? bench\.py[^\n]*", text, re.M)
        exported = re.search(rf"^export {bench.FULL_ENV}=1\b", text, re.M)
        assert exported or all("--full" in c for c in calls), os.path.basename(p)


def run_bench(*argv):
    """One plain bench.py run in a fresh process; returns its single JSON line."""
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", bench.FULL_ENV)}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + [str(a) for a in argv],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["ms_per_step"] > 0 and line["higher_is_better"] is True
    for key in ("roofline", "cpu_baseline", "parity_sample", "end_to_end", "commands", "secondary"):
        assert key not in line
    return line


def test_write_outputs_names_and_shapes(tmp_path):
    import bench
    d = tmp_path / "a" / "b"
    shapes = bench.write_outputs(str(d), {"x": np.arange(6, dtype=np.float64).reshape(2, 3), "y": np.ones(4, np.float32)})
    assert shapes == {"x": [2, 3], "y": [4]}
    assert np.array_equal(np.load(d / "x.npy"), np.arange(6.0).reshape(2, 3))
    assert np.load(d / "y.npy").dtype == np.float32


@pytest.mark.gpu
@pytest.mark.parametrize("leaves, sites", [
    (3000, 1001),      # fewer records than the sample size: every row written, checked against the oracle
    (40009, 12007),   # more records than the sample size: the seeded sample of the rows
])
def test_plain_run_line_and_dumped_outputs(tmp_path, oracle, leaves, sites):
    import bench
    import panman_amd
    out = tmp_path / "dump"
    line = run_bench("--steps", 3, "--warmup", 1, "--leaves", leaves, "--sites", sites, "--dump-outputs", out)
    n_nodes = 2 * leaves - 1
    assert line["value"] == pytest.approx(sites * n_nodes / (line["ms_per_step"] * 1e-3), rel=1e-9)

    # the same seeded workload through the API
    off, idx, root = panman_amd.random_join_tree(leaves, seed=1)
    eng = panman_amd.Engine(0)
    eng.tree_upload(off, idx, root)
    eng.synth_columns(0, sites, seed=2)
    eng.run(panman_amd.MODE_FITCH)
    want = eng.mutations()
    score, root_code = eng.site_results()
    small = want.shape[0] <= bench.DUMP_ROWS
    assert small == (leaves == 3000) and want.shape[0] > 0
    if small:   # an independent reference: the CPU oracle on the same leaf codes
        codes = eng.leaf_codes(0, sites, leaves)
        cons = eng.consensus(0, sites)
        names = [f"s{i}" if i < leaves else f"node_{i}" for i in range(n_nodes)]
        node_row = np.full(n_nodes, -1, np.int32)
        node_row[:leaves] = np.arange(leaves)
        _, ref = oracle.csr_columns(off, idx, root, names, codes, node_row, cons, None, algo=0, threads=4)
        assert ref.shape == want.shape and (ref == want).all()
    eng.close()
    got = {name: np.load(out / f"{name}.npy") for name in line["outputs"]}
    assert sorted(got) == ["mutation_count", "mutations_sample", "site_root_code", "site_score"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["mutation_count"].tolist() == [want.shape[0]] == [line["config"]["mutations_total"]]
    rows = bench.sample_rows(want.shape[0])
    assert got["mutations_sample"].shape == (min(want.shape[0], bench.DUMP_ROWS), 4)
    assert np.array_equal(got["mutations_sample"], want[rows].astype(np.float64))
    assert np.array_equal(got["site_score"], score.astype(np.float64))
    assert np.array_equal(got["site_root_code"], root_code.astype(np.float32))
    # Fitch: a site's score is the number of its records below the root
    assert np.array_equal(score, np.bincount(want[want[:, 0] != root][:, 1], minlength=sites))


@pytest.mark.gpu
@pytest.mark.parametrize("leaves, blocks, mean_len", [
    (37, 12, 900),      # text shorter than the sample size: every byte written, records checked against the oracle
    (60, 40, 1500),     # a longer text: the seeded sample of its bytes
])
def test_plain_replay_run_line_and_dumped_text(tmp_path, oracle, leaves, blocks, mean_len):
    import bench
    import panman_amd
    from panman_amd.synth import c5_panmat
    out = tmp_path / "dump"
    line = run_bench("--mode", "replay", "--steps", 3, "--warmup", 1, "--replay-leaves", leaves,
                     "--replay-blocks", blocks, "--replay-block-len", mean_len, "--dump-outputs", out)
    assert line["unit"] == "leaf*column/s"

    # the same seeded PanMAT through the API
    pm = c5_panmat(leaves=leaves, blocks=blocks, mean_len=mean_len)
    eng = panman_amd.Engine(0)
    eng.replay_prepare(pm)
    n_leaves, cols, _ = eng.replay_shape()
    eng.replay_run()
    text = eng.replay_format(True)
    eng.close()
    assert n_leaves == leaves
    assert line["value"] == pytest.approx(leaves * cols / (line["ms_per_step"] * 1e-3), rel=1e-9)
    want = np.frombuffer(text.encode(), np.uint8)
    small = want.size <= bench.DUMP_ROWS
    assert small == (leaves == 37)
    if small:   # an independent reference: the CPU oracle's records
        assert sorted(text.split(">")) == sorted(oracle.fasta(pm, True).split(">"))
    got = {name: np.load(out / f"{name}.npy") for name in line["outputs"]}
    assert sorted(got) == ["fasta_bytes", "fasta_sample"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["fasta_bytes"].tolist() == [want.size]
    assert got["fasta_sample"].shape == (min(want.size, bench.DUMP_ROWS),)
    assert np.array_equal(got["fasta_sample"], want[bench.sample_rows(want.size)].astype(np.float32))
