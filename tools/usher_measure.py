"""pm_to_usher phase times on a synthetic PanMAT: c5_panmat(LEAVES, BLOCKS, MEAN_LEN, seed SEED),
written as a PanMAN and loaded again; one warming call, five timed calls, median and min-max of the wall time and
of every phase, the record count and the size of the bytes.  Seed 5 at 100 50 10000 is the input of
tools/mutations_measure.py.  No host comparator exists.  Run from the repository root:
    python tools/usher_measure.py LEAVES BLOCKS MEAN_LEN [SEED]"""
import os, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import numpy as np
import panman_amd
from panman_amd.panmat import PanmanFile, write_panman
from panman_amd.synth import c5_panmat

leaves, blocks, mean_len = (int(a) for a in sys.argv[1:4])
seed = int(sys.argv[4]) if len(sys.argv) > 4 else 5
def say(*a):
    print(*a, flush=True)
eng = panman_amd.Engine(0)
d = tempfile.mkdtemp()
pm = c5_panmat(leaves=leaves, blocks=blocks, mean_len=mean_len, seed=seed)
write_panman(d + "/in.panman", [pm], compress=False)
f = PanmanFile(d + "/in.panman")
st = f.view(0)
data, records = eng.to_usher(st)   # the warming call
say("leaves", leaves, "blocks", blocks, "mean_len", mean_len, "seed", seed, "nodes", pm.num_nodes, "build", panman_amd.build_id())
say("out_bytes", len(data), "records", records)
walls, phases = [], {}
for rep in range(5):
    panman_amd.phase_reset()
    t0 = time.time()
    got = eng.to_usher(st)
    walls.append(time.time() - t0)
    assert got == (data, records)
    for name, s in panman_amd.phase_report():
        if name.startswith(("usher.", "replay.", "fasta.")):
            phases.setdefault(name, []).append(s)
eng.close()
def line(name, v):
    say(f"{name}\tmedian {np.median(v):.6f}\tmin {min(v):.6f}\tmax {max(v):.6f}")
line("wall_s", walls)
for name, v in phases.items():
    line(name, v)
