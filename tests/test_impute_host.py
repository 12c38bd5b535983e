"""The host plan of pm_impute (panman_amd/csrc/pm_impute_plan.cpp over pm_impute_plan.h) as a stand-alone program
under AddressSanitizer (with its leak checker) and UBSan: tests/impute_host_check.cpp, built with g++ and run as
a child process.  It replays the candidate lists and winners of the hand cases of tests/_impute_cases.py (at the
distances of tests/test_impute_ref.py, which pins the same lists by hand) and of a planted random case, then its
built-in checks: path steps, block folds, the drifting strand, the winner rule and every argument error.  CPU
only; nothing is loaded into this interpreter."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _impute_cases as cases
import _impute_ref as ref
from _trees import parse_newick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "panman_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SOURCES = [os.path.join(ROOT, "tests", "impute_host_check.cpp"), os.path.join(CSRC, "pm_impute_plan.cpp")]


def case_set():
    out = [(name, make(), 5) for name, make in cases.HAND.items()]
    for length, distance in ((0.5, 0), (0.5, -1), (1.0, 1), (1.0, 2), (1.0, 3)):
        out.append((f"sibling_{length}_{distance}", cases.sibling_donor(length), distance))
        out.append((f"grandparent_{length}_{distance}", cases.grandparent_donor(length), distance))
    nwk = "".join(f"(s{i}," for i in range(29)) + "s29" + ")" * 29 + ";"
    names, off, idx, root = parse_newick(nwk)
    for distance in (0, 2, 5):
        out.append((f"planted_{distance}", cases.planted(np.random.default_rng(3), names, off, idx, root), distance))
    return out


def write_case(path, pm, distance):
    trace, scores = {}, {}
    _, plan, _ = ref.impute(pm, distance, trace, scores)
    winner = {}
    for line in plan.splitlines():
        f = line.split("\t")
        if len(f) == 6 and f[1] not in ("B", "N"):
            winner[f[0]] = -1 if f[3] == "." else pm.index(f[3])
    with open(path, "w") as f:
        f.write(f"{pm.num_nodes} {pm.root} {distance} {int(pm.branch_length is not None)}\n")
        f.write(" ".join(str(int(x)) for x in pm.child_offsets) + "\n")
        f.write(" ".join(str(int(x)) for x in pm.child_index) + "\n")
        if pm.branch_length is not None:
            f.write(" ".join(repr(float(x)) for x in pm.branch_length) + "\n")
        blocks = [(v,) + b for v in range(pm.num_nodes) for b in pm.block_muts[v]]
        f.write(f"B {len(blocks)}\n" + "".join(" ".join(str(int(x)) for x in b) + "\n" for b in blocks))
        muts = [(v, m[0], m[2], m[3], m[4], m[5]) for v in range(pm.num_nodes) for m in pm.nuc_muts[v]]
        f.write(f"M {len(muts)}\n" + "".join(" ".join(str(int(x)) for x in m) + "\n" for m in muts))
        f.write(f"A {len(trace)}\n")
        for name in sorted(trace, key=pm.index):
            cands = " ".join(str(pm.index(c)) for c in trace[name])
            nuc = " ".join(str(s[0]) for s in scores.get(name, []))
            f.write(f"{pm.index(name)} {cands} | {nuc} | {winner[name]}\n")
    return len(trace), sum(len(c) for c in trace.values())


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_impute_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "impute_host_check")
    built = subprocess.run(["g++"] + FLAGS + SOURCES + ["-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    paths, attempts, pairs = [], 0, 0
    for name, pm, distance in case_set():
        paths.append(str(tmp_path / (name + ".case")))
        a, p = write_case(paths[-1], pm, distance)
        attempts += a
        pairs += p
    assert attempts >= 30 and pairs >= 30   # the files do carry candidates to compare
    ran = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert f"{len(paths)} case files and the built-in checks passed" in ran.stdout
