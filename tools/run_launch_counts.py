"""Records tests/golden/run_launch_counts.json: per input of tests/_launch_matrix.py, the timer
spans pm_kernel_times reports for the post-order, pre-order and tail classes and the run.* phase
values of one pm_run, graph off.  Only the public Python API is used, so the file can be recorded
at any commit: tests/test_gpu_launch_counts.py and tests/test_schedule_host.py then hold later
launchers to it.  Run from the repository root on a GPU:
    python tools/run_launch_counts.py [OUTPUT]"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import panman_amd

import _launch_matrix as lm

t0 = time.time()
engine = panman_amd.Engine(0)
entries = {}
for name, tree in lm.tree_set():
    entries.update(lm.walk_tree(engine, name, tree))
    print(f"{name}: {time.time() - t0:.1f} s", flush=True)
engine.close()
if len(sys.argv) > 1:
    lm.GOLDEN = sys.argv[1]
lm.write_golden(entries)
print(f"{len(entries)} entries x {len(lm.SITES) * len(lm.PRESENT) * len(lm.MODES)} runs -> {lm.GOLDEN}")
