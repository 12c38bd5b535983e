"""The tree planner (panman_amd/csrc/pm_plan.cpp over pm_plan.h, with the sweeps' schedule of
pm_cluster.cpp) as a stand-alone program under AddressSanitizer (with its leak checker) and UBSan:
tests/plan_host_check.cpp, built with g++ and run as a child process.  It checks the hand-written
plans of three tiny trees, every argument error, and the plan's invariants over the trees written
here and the library's two generators, under four sweep settings each.  CPU only; nothing is
loaded into this interpreter."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _shapes
import _trees

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "panman_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"]
SOURCES = [os.path.join(ROOT, "tests", "plan_host_check.cpp")] + [
    os.path.join(CSRC, f) for f in ("pm_plan.cpp", "pm_cluster.cpp", "pm_hostpar.cpp", "pm_synth_tree.cpp")]


def tree_set():
    """(name, (off, idx, root)) of every tree the check plans."""
    trees = [(f"edge_{k}", _shapes.edge_tree(degrees, unary_every=unary))
             for k, (degrees, unary) in enumerate([(_shapes.MAIN_DEGREES, 7), (_shapes.MAIN_DEGREES, 0),
                                                   (_shapes.WIDE_DEGREES, 0)])]
    trees += [(f"ladder_{h}", _shapes.ladder(h)) for h in (31, 32, 33, 64, 65, 129)]
    trees += [(f"fat_{n}", _shapes.fat_cluster(n)) for n in (63, 64, 65)]
    trees.append(("fat_five_live", _shapes.fat_cluster(0, five_live=True)))
    trees += [(f"star_{w}", _shapes.star_with_sibling(w)) for w in (255, 256, 257)]
    for leaves in (2, 3, 50, 3000):
        for max_children in (2, 4, 40, 300):
            rng = np.random.default_rng(1000 * leaves + max_children)
            trees.append((f"random_{leaves}_{max_children}", _trees.random_tree(leaves, rng, max_children=max_children)))
    return trees


def write_trees(directory):
    """Each tree as a text file: "N root n_off n_idx", the offsets, the indices."""
    paths = []
    for name, (off, idx, root) in tree_set():
        path = os.path.join(str(directory), name + ".tree")
        with open(path, "w") as f:
            f.write(f"{off.shape[0] - 1} {int(root)} {off.shape[0]} {idx.shape[0]}\n")
            f.write(" ".join(str(int(x)) for x in off) + "\n")
            f.write(" ".join(str(int(x)) for x in idx) + "\n")
        paths.append(path)
    return paths


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_plan_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "plan_host_check")
    # (the five files side by side: under the sanitizers the check alone compiles for a while)
    objects = [str(tmp_path / (os.path.basename(src) + ".o")) for src in SOURCES]
    jobs = [subprocess.Popen(["g++"] + FLAGS + ["-c", src, "-o", obj], stderr=subprocess.PIPE, text=True)
            for src, obj in zip(SOURCES, objects)]
    for job in jobs:
        _, err = job.communicate()
        assert job.returncode == 0, err
    built = subprocess.run(["g++"] + FLAGS + objects + ["-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    paths = write_trees(tmp_path)
    ran = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    # the digests do not depend on the number of host threads
    digests = []
    for threads in ("1", "4"):
        env = dict(os.environ, PM_HOST_THREADS=threads)
        out = subprocess.run([exe, "--digest"] + paths, capture_output=True, text=True, env=env)
        assert out.returncode == 0, out.stderr
        digests.append(out.stdout)
    assert digests[0] == digests[1]
    assert digests[0].count("== ") == 4 * (len(paths) + 2)
