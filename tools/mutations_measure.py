"""pm_print_mutations phase times on a synthetic PanMAT: c5_panmat(LEAVES, BLOCKS, MEAN_LEN),
written as a PanMAN and loaded again; one warming call, five timed calls, median and min-max of the wall time and
of every phase, the entry count and the text size.
The generator's seed is the first from 3 on at which the call is defined (a node that inverts a block it does not
hold is PM_ERR_UNSUPPORTED, see include/panman_gpu.h).  No host comparator exists.  Run from the repository root:
    python tools/mutations_measure.py LEAVES BLOCKS MEAN_LEN"""
import os, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import numpy as np
import panman_amd
from panman_amd.panmat import PanmanFile, write_panman
from panman_amd.synth import c5_panmat

leaves, blocks, mean_len = (int(a) for a in sys.argv[1:4])
def say(*a):
    print(*a, flush=True)
eng = panman_amd.Engine(0)
d = tempfile.mkdtemp()
text = None
for seed in range(3, 19):   # the warming call, and the search for a defined tree
    pm = c5_panmat(leaves=leaves, blocks=blocks, mean_len=mean_len, seed=seed)
    write_panman(d + "/in.panman", [pm], compress=False)
    f = PanmanFile(d + "/in.panman")
    st = f.view(0)
    try:
        text, odd = eng.print_mutations(st)
        break
    except panman_amd.PanmanError as e:
        say("seed", seed, "refused:", str(e)[:160])
        f.close()
if text is None:
    sys.exit("no defined tree")
say("leaves", leaves, "blocks", blocks, "mean_len", mean_len, "seed", seed, "nodes", pm.num_nodes, "build", panman_amd.build_id())
say("text_bytes", len(text), "lines", text.count("\n"), "printed_entries", text.count(" > "), "odd_substitutions", odd)
walls, phases = [], {}
for rep in range(5):
    panman_amd.phase_reset()
    t0 = time.time()
    got = eng.print_mutations(st)
    walls.append(time.time() - t0)
    assert got[0] == text
    for name, s in panman_amd.phase_report():
        if name.startswith(("mutations.", "replay.", "fasta.")):
            phases.setdefault(name, []).append(s)
eng.close()
def line(name, v):
    say(f"{name}\tmedian {np.median(v):.6f}\tmin {min(v):.6f}\tmax {max(v):.6f}")
line("wall_s", walls)
for name, v in phases.items():
    line(name, v)
