"""The launch schedule of a pm_run (panman_amd/csrc/pm_schedule.cpp over the planner) as a
stand-alone program under AddressSanitizer (with its leak checker) and UBSan:
tests/schedule_host_check.cpp, built with g++ and run as a child process.  It checks the
hand-written step lists of three tiny trees and the schedule's invariants over every input of
_launch_matrix.py; its timer-span counts and run.* values must be the ones recorded from the
launchers on a GPU (tests/golden/run_launch_counts.json), and those inputs must reach every step
kind.  CPU only; nothing is loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

import _launch_matrix as lm
from test_plan_host import CSRC, FLAGS, ROOT, write_trees

SOURCES = [os.path.join(ROOT, "tests", "schedule_host_check.cpp")] + [
    os.path.join(CSRC, f) for f in ("pm_schedule.cpp", "pm_plan.cpp", "pm_cluster.cpp", "pm_hostpar.cpp", "pm_synth_tree.cpp")]
KINDS = {"fork", "join", "span", "up_band", "up_mixed", "up_wide", "up_narrow", "up_sweep", "up_parts", "up_merge", "down_sweep",
         "down_band", "down_level", "down_group", "down_packed", "tail", "tail_packed"}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_schedule_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "schedule_host_check")
    objects = [str(tmp_path / (os.path.basename(src) + ".o")) for src in SOURCES]
    jobs = [subprocess.Popen(["g++"] + FLAGS + ["-c", src, "-o", obj], stderr=subprocess.PIPE, text=True)
            for src, obj in zip(SOURCES, objects)]
    for job in jobs:
        _, err = job.communicate()
        assert job.returncode == 0, err
    built = subprocess.run(["g++"] + FLAGS + objects + ["-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    configs = str(tmp_path / "configs.txt")
    with open(configs, "w") as f:
        for name, cfg in lm.CONFIGS:
            f.write(name + " " + " ".join(str(v) for v in lm.option_values(cfg)) + "\n")
    ran = subprocess.run([exe, configs] + write_trees(tmp_path), capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr
    got, kinds = {}, None
    for line in ran.stdout.splitlines():
        words = line.split()
        if words[0] == "counts":
            flat = [int(w) for w in words[2:]]
            got[words[1]] = [flat[k:k + len(lm.COUNTS)] for k in range(0, len(flat), len(lm.COUNTS))]
        elif words[0] == "kinds":
            kinds = set(words[1:])
    # fidelity to the launchers the golden was recorded from, for every entry it holds
    golden = lm.load_golden()
    assert len(golden) == len(lm.CONFIGS) * len(lm.tree_set())
    for entry, rows in golden.items():
        assert got[entry] == rows, (entry, got[entry], rows)
    # ... and those inputs reach every step kind
    assert kinds == KINDS, KINDS - kinds
