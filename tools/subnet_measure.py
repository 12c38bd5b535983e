"""pm_subnet phase times on a synthetic PanMAT: a random-join tree whose nucleotide mutations are
the Fitch records of seeded columns, every other tip requested; then tools/subnet_host_fold (build it first, see
its head) over the same PanMAN and request.  Run from the repository root:
    python tools/subnet_measure.py LEAVES SITES"""
import os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import panman_amd
from _trees import names_for
from panman_amd.panmat import PanMAT

leaves, sites = int(sys.argv[1]), int(sys.argv[2])
def say(*a):
    print(*a, flush=True)
off, idx, root = panman_amd.random_join_tree(leaves, seed=3)
eng = panman_amd.Engine(0)
eng.tree_upload(off, idx, root)
eng.synth_columns(0, sites, seed=2)
eng.run(panman_amd.MODE_FITCH)
rec = eng.mutations()
n = off.shape[0] - 1
say("leaves", leaves, "sites", sites, "nodes", n, "records", rec.shape[0], "build", panman_amd.build_id())
node, site, typ, code = (rec[:, k].astype(np.int64) for k in range(4))
snp = np.array([3, 5, 4], np.uint8)[typ]
names = names_for(off)
pm = PanMAT(names, off, idx, root)
words = (sites + 7) // 8
seq = np.full(words, 0x11111111, np.uint32)
if sites % 8: seq[-1] = (0x11111111 >> (4 * (8 - sites % 8))) << (4 * (8 - sites % 8))
bm_off = np.zeros(n + 1, np.int64); bm_off[root + 1:] = 1
pm.set_arrays(block_primary=np.zeros(1, np.int32), block_seq_offsets=np.array([0, words], np.int64), block_seq=seq,
              gap_primary=np.zeros(0, np.int32), gap_offsets=np.zeros(1, np.int64), gap_position=np.zeros(0, np.uint32),
              gap_length=np.zeros(0, np.uint32), block_mut_offsets=bm_off, block_mut_primary=np.zeros(1, np.int32),
              block_mut_info=np.ones(1, np.uint8), block_mut_inversion=np.zeros(1, np.uint8),
              nuc_mut_offsets=np.concatenate([[0], np.cumsum(np.bincount(node, minlength=n))]).astype(np.int64),
              nuc_mut_primary=np.zeros(len(node), np.int32), nuc_mut_secondary=np.full(len(node), -1, np.int32),
              nuc_mut_position=site.astype(np.int32), nuc_mut_gap_position=np.full(len(node), -1, np.int32),
              nuc_mut_info=(16 + snp).astype(np.uint8), nuc_mut_nucs=(code << 20).astype(np.uint32))
st, keep = pm.as_struct()
tips = [names[v] for v in range(n) if off[v] == off[v + 1]][::2]
for rep in range(3):
    panman_amd.phase_reset()
    t0 = time.time()
    f = eng.subnet(st, tips)
    dt = time.time() - t0
    v = f.view(0)
    say("rep", rep, "wall_s", round(dt, 4), "new_nodes", v.num_nodes,
        " ".join(f"{k}={s:.4f}" for k, s in panman_amd.phase_report() if k.startswith("subnet.")))
    f.close()
eng.close()
import subprocess, tempfile
from panman_amd.panmat import write_panman
d = tempfile.mkdtemp()
write_panman(d + "/in.panman", [pm], compress=False)
open(d + "/ids.txt", "w").write(" ".join(tips) + "\n")
r = subprocess.run(["tools/subnet_host_fold", d + "/in.panman", d + "/ids.txt"], capture_output=True, text=True)
say(r.stdout.strip(), r.stderr.strip())
