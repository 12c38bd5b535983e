"""pm_aa phase times on a synthetic PanMAT: c5_panmat(LEAVES, BLOCKS, MEAN_LEN) and a window of
WINDOW coordinates, written as a PanMAN and loaded again; one warming call, five timed calls, median and min-max
of the wall time and of every phase; then tools/aa_host (build it first, see its head) over the same file, its
text compared with the device's.
The window starts at the first multiple of WINDOW at which the call is defined (a reverse-strand block inside the
window that is shorter than block 0 is PM_ERR_UNSUPPORTED, see include/panman_gpu.h).  Run from the repository root:
    python tools/aa_measure.py LEAVES BLOCKS MEAN_LEN WINDOW"""
import os, subprocess, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import numpy as np
import panman_amd
from panman_amd.panmat import PanmanFile, write_panman
from panman_amd.synth import c5_panmat

leaves, blocks, mean_len, window = (int(a) for a in sys.argv[1:5])
def say(*a):
    print(*a, flush=True)
pm = c5_panmat(leaves=leaves, blocks=blocks, mean_len=mean_len)
d = tempfile.mkdtemp()
write_panman(d + "/in.panman", [pm], compress=False)
f = PanmanFile(d + "/in.panman")
st = f.view(0)
eng = panman_amd.Engine(0)
say("leaves", leaves, "blocks", blocks, "mean_len", mean_len, "nodes", pm.num_nodes, "build", panman_amd.build_id())
start = None
for k in range(16):   # the warming call, and the search for a defined window
    try:
        text, codons, lost = eng.aa(st, k * window, (k + 1) * window)
        start = k * window
        break
    except panman_amd.PanmanError as e:
        say("window", k * window, "refused:", str(e)[:160])
if start is None:
    sys.exit("no defined window")
say("window", start, start + window, "ref_codons", codons, "unlocated", lost, "text_bytes", len(text), "lines", text.count("\n") - 1)
walls, phases = [], {}
for rep in range(5):
    panman_amd.phase_reset()
    t0 = time.time()
    got = eng.aa(st, start, start + window)
    walls.append(time.time() - t0)
    assert got[0] == text
    for name, s in panman_amd.phase_report():
        if name.startswith(("aa.", "replay.", "fasta.")):
            phases.setdefault(name, []).append(s)
eng.close()
def line(name, v):
    say(f"{name}\tmedian {np.median(v):.6f}\tmin {min(v):.6f}\tmax {max(v):.6f}")
line("wall_s", walls)
for name, v in phases.items():
    line(name, v)
if os.path.exists("tools/aa_host"):
    r = subprocess.run(["tools/aa_host", d + "/in.panman", str(start), str(start + window), d + "/host.tsv"], capture_output=True, text=True)
    say(r.stdout.strip(), r.stderr.strip())
    if r.returncode == 0:
        say("host text equals the device text:", open(d + "/host.tsv").read() == text)
