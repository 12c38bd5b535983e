"""GPU subnetwork extraction (pm_subnet; src/subnet.cpp:3-135, src/panman.cpp:2033-2085, :2233-2372) against
the plain-Python restatement tests/_subnet_ref.py, which merges one node at a time and re-consolidates at
every merge as the reference does, where pm_subnet folds every coordinate of a chain once.  Dumps are
compared whole (Newick with names and summed lengths, block mutations sorted per node, NucMut records in
list order); the kernels' edges are hand-built chains at the smallest sizes where they can go wrong."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import _subnet_ref as ref
import panman_amd
from _panmat import _parse_labelled, parse_records, random_panmat, tree_dump
from _trees import names_for, parse_newick, to_newick
from panman_amd._lib import header_symbols, load
from panman_amd.panmat import PanMAT, PanmanFile, write_panman

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "bin", "panmanUtils")
S, I, D = ref.NSNPS, ref.NSNPI, ref.NSNPD
SUBSETS = ["one_tip", "siblings", "opposite", "every_other", "all", "internal_and_tip", "root"]


@pytest.fixture(scope="module")
def engine():
    e = panman_amd.Engine(0)
    yield e
    e.close()


def _gpu_dump(engine, pm, ids):
    f = engine.subnet(pm, ids)
    try:
        return ref.sorted_blocks(tree_dump(f))
    finally:
        f.close()


def _check(engine, pm, ids):
    """The GPU's dump, after it matched the restatement's."""
    got = _gpu_dump(engine, pm, ids)
    assert got == ref.dump(*ref.subnet(pm, ids))
    return got


def _records(dump, name):
    """(position, gap position, info, nucs) of a node's NucMut lines."""
    out = []
    for line in dump.splitlines():
        f = line.split("\t")
        if f[0] == name and f[1] == "N":
            out.append((int(f[3]), int(f[4]), int(f[5]), int(f[6], 16)))
    return out


# ---- record parity on random PanMATs ------------------------------------------------------------------

def _caterpillar(leaves):
    nwk = "".join(f"(s{i}," for i in range(leaves - 1)) + f"s{leaves - 1}" + ")" * (leaves - 1) + ";"
    return parse_newick(nwk)


def _random_join(leaves, seed):
    off, idx, root = panman_amd.random_join_tree(leaves, seed=seed)
    return parse_newick(to_newick(off, idx, root, names_for(off)))


@pytest.fixture(scope="module", params=["join40", "caterpillar70"])
def random_case(request):
    """A random PanMAT (no block mutation below the root, so no seed meets a raising block pair) and the
    restatement's dump of every standard request, computed once."""
    names, off, idx, root = _random_join(40, 5) if request.param == "join40" else _caterpillar(70)
    rng = np.random.default_rng(40 if request.param == "join40" else 70)
    pm = random_panmat(rng, off, idx, root, names, block_rate=0, options=True)
    pm.branch_length = rng.integers(1, 50, size=len(names)).astype(np.float32) / 8
    sets = ref.standard_subsets(pm)
    return pm, sets, {k: ref.dump(*ref.subnet(pm, ids)) for k, ids in sets.items()}


@pytest.mark.parametrize("which", SUBSETS)
def test_records_match_the_restatement(engine, random_case, which):
    pm, sets, want = random_case
    assert _gpu_dump(engine, pm, sets[which]) == want[which]


def test_without_branch_lengths(engine, random_case):
    pm, sets, _ = random_case
    bare = copy.copy(pm)
    bare.branch_length = None
    newick = _check(engine, bare, sets["every_other"]).splitlines()[0]
    assert ":1.000000" in newick and newick.endswith(":0.000000;")   # the Newick parser's defaults


def test_batch_size_does_not_change_the_result(engine, random_case):
    """Batches of whole new nodes of at most 64 bases (most chains of the caterpillar alone hold more, and get
    a batch of their own) against the default, one batch."""
    pm, sets, want = random_case
    try:
        engine.set_subnet_batch_entries(64)
        for which in ("every_other", "opposite", "one_tip"):
            assert _gpu_dump(engine, pm, sets[which]) == want[which]
    finally:
        engine.set_subnet_batch_entries(1 << 25)
    with pytest.raises(panman_amd.PanmanError, match="PM_OPT_SUBNET_BATCH_ENTRIES"):
        engine.set_subnet_batch_entries(0)


# ---- the kernels' edges on hand-built chains ------------------------------------------------------------

def _spine(depth, block_lens=(400,), gaps=()):
    """A caterpillar of `depth` internal nodes; returns the PanMAT and the chain node_1 .. node_depth, t<depth>
    (node ids, top first) that a request for the deepest tip merges into one node."""
    nwk = "".join(f"(t{i}," for i in range(depth)) + f"t{depth}" + ")" * depth + ";"
    names, off, idx, root = parse_newick(nwk)
    pm = PanMAT(names, off, idx, root)
    for b, n in enumerate(block_lens):
        pm.add_block(b, ("ACGT" * (n // 4 + 1))[:n])
        pm.add_block_mut(root, b, True, False)
    for b, slots in gaps:
        pm.add_gaps(b, slots)
    chain = [pm.index(f"node_{k}") for k in range(1, depth + 1)] + [pm.index(f"t{depth}")]
    return pm, chain


def test_segment_longer_than_a_wave(engine):
    """68 merged nodes all mutate one coordinate: one fold segment of 68 entries, walked by one lane."""
    pm, chain = _spine(67)
    types = [S, I, D]
    for k, v in enumerate(chain):
        pm.add_nuc_mut(v, 0, 33, -1, types[(k * 7 + k // 3) % 3], [[1, 2, 4, 8][k % 4]])
    assert len(chain) == 68
    dump = _check(engine, pm, ["t67"])
    assert dump.splitlines()[0] == "newick\tt67" and len(_records(dump, "t67")) <= 1


def test_segments_and_runs_across_a_thread_block(engine):
    """The same chain with 340 expanded bases: every node also substitutes four positions of a run 272 long,
    and the 68-entry segment sits at position 240, across the 256th sorted entry."""
    pm, chain = _spine(67)
    for k, v in enumerate(chain):
        pm.add_nuc_mut(v, 0, 240, -1, S if k % 5 else D, [[1, 2, 4, 8][k % 4]])
        pm.add_nuc_mut(v, 0, 4 * k, -1, ref.NS, [8, 4, 2, 1])
    dump = _check(engine, pm, ["t67"])
    recs = _records(dump, "t67")
    # (position 240 folds 69 entries: one survivor, or none after an insertion met a deletion)
    assert sum(r[2] >> 4 for r in recs) in (271, 272) and [r[2] >> 4 for r in recs[:3]] == [6, 6, 6]


def test_runs_of_5_6_7_12_13_across_boundaries(engine):
    """248 isolated substitutions, then runs of 5, 6, 7, 12 and 13 (the run of 6 holds the 256th survivor), a
    run that ends at block 0's last position and one that starts at block 1's first: cut at 6, never joined."""
    pm, chain = _spine(2, block_lens=(700, 40))
    top, low = chain[0], chain[2]
    for k in range(248):
        pm.add_nuc_mut(top if k % 2 else low, 0, 2 * k, -1, S, [1])
    at = 500
    for n in (5, 6, 7, 12, 13):
        for k in reversed(range(n)):   # (list order is not coordinate order)
            pm.add_nuc_mut(low if k % 3 else top, 0, at + k, -1, S, [2])
        at += n + 1
    for k in range(4):
        pm.add_nuc_mut(top, 0, 696 + k, -1, S, [4])
        pm.add_nuc_mut(low, 1, k, -1, S, [4])
    dump = _check(engine, pm, ["t2"])
    lens = [r[2] >> 4 for r in _records(dump, "t2")]
    assert lens == [1] * 248 + [5, 6, 6, 1, 6, 6, 6, 6, 1, 4, 4]


def test_restart_and_vanish_at_a_segment_end(engine):
    pm, chain = _spine(3)
    a, b, c = chain[0], chain[1], chain[3]
    for v, typ in ((a, I), (b, D), (c, I)):   # I, D, I: one insertion, the last one's code
        pm.add_nuc_mut(v, 0, 10, -1, typ, [8 if v == c else 1])
    for v, typ in ((a, I), (c, D)):           # I, D: gone, at the end of its segment
        pm.add_nuc_mut(v, 0, 11, -1, typ, [1])
    for v, typ in ((a, S), (b, I), (c, D)):   # S, I, D: a deletion
        pm.add_nuc_mut(v, 0, 12, -1, typ, [2])
    dump = _check(engine, pm, ["t3"])
    assert _records(dump, "t3") == [(10, -1, (1 << 4) + I, 8 << 20), (12, -1, (1 << 4) + D, 2 << 20)]


def test_gap_entries_break_a_main_run(engine):
    pm, chain = _spine(2, gaps=[(0, [(20, 3)])])
    pm.add_nuc_mut(chain[0], 0, 20, -1, ref.NS, [1, 2])       # main positions 20 and 21
    pm.add_nuc_mut(chain[2], 0, 20, 0, ref.NS, [4, 8])        # gap slots (20, 0) and (20, 1)
    dump = _check(engine, pm, ["t2"])
    assert [(r[0], r[1], r[2]) for r in _records(dump, "t2")] == [(20, -1, (1 << 4) + S), (20, 0, (2 << 4) + ref.NS),
                                                                 (21, -1, (1 << 4) + S)]


def test_stable_sort_the_lower_node_wins(engine):
    """Two chain nodes write different codes at one coordinate with the same type: the fold takes the later
    entry, so the lower node's code survives only if the sort kept equal keys in entry order."""
    pm, chain = _spine(2)
    for pos in range(60, 66):
        pm.add_nuc_mut(chain[0], 0, pos, -1, S, [1])
        pm.add_nuc_mut(chain[2], 0, pos, -1, S, [8])
    assert _records(_check(engine, pm, ["t2"]), "t2") == [(60, -1, (6 << 4) + ref.NS, 0x888888)]


def test_nothing_merges_nothing_launches(engine):
    """Every tip of a binary tree requested: all lists verbatim and not one launch; a merging request launches."""
    names, off, idx, root = _random_join(12, 3)
    pm = random_panmat(np.random.default_rng(12), off, idx, root, names, block_rate=0.3, options=False)
    tips = [pm.names[v] for v in pm.leaves()]
    engine.set_profiling(True)
    try:
        engine.kernel_times()
        f = engine.subnet(pm, tips)
        assert engine.kernel_times()[1][3] == 0
        assert tree_dump(f) == ref.dump(pm, f.newick(0), sort_blocks=False)
        f.close()
        plain = random_panmat(np.random.default_rng(13), off, idx, root, names, block_rate=0, options=False)
        engine.subnet(plain, tips[:1]).close()
        assert engine.kernel_times()[1][3] > 0
    finally:
        engine.set_profiling(False)


def test_one_tip_and_root_only(engine, random_case):
    pm, _, _ = random_case
    tip = pm.names[pm.leaves()[3]]
    assert _check(engine, pm, [tip, tip]).splitlines()[0] == "newick\t" + tip
    assert _check(engine, pm, [pm.names[pm.root]]).splitlines()[0] == "newick\t" + pm.names[pm.root]


# ---- sequences, files, the command ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def sars(engine):
    """tests/golden/sars_20 built on the GPU.  (Its genomes differ in length, so it has no MSA build; the
    PanGraph build of sars_20.json is the suite's sars_20 PanMAN.)"""
    text = open(os.path.join(GOLD, "sars_20.json")).read()
    f = engine.pangraph_build(text, open(os.path.join(GOLD, "sars_20.nwk")).read())
    want = {al: parse_records(engine.fasta(f.view(0), al)) for al in (True, False)}
    yield f, want
    f.close()


@pytest.mark.parametrize("which", ["one_tip", "opposite", "every_other", "all", "internal_and_tip"])
def test_extraction_keeps_every_kept_tip_sequence(engine, sars, which):
    f, want = sars
    pm = f.to_panmat(0)
    ids = ref.standard_subsets(pm)[which]
    kept = {pm.names[v] for v in pm.leaves()} & set(ids)
    g = engine.subnet(f.view(0), ids)
    try:
        for aligned in (True, False):
            got = parse_records(engine.fasta(g.view(0), aligned))
            assert kept <= set(got)
            for name in sorted(kept):
                assert got[name] == want[aligned][name], (name, aligned)
    finally:
        g.close()


def _as_loaded(dump):
    """`dump` as it reads after a write and a load: the stored Newick text is kept as written, and the loader
    names the internal nodes node_<k> in pre-order whatever their labels (src/panman.cpp:310-450).  The file
    holds a node's mutations grouped by block, blocks ascending (src/panman.cpp:2857-2887), so a list that was
    copied verbatim comes back in that order, list order kept within a block."""
    lines = dump.splitlines()
    names, kids, _ = _parse_labelled(lines[0][7:])
    new, k = {}, 0
    for v, n in enumerate(names):
        if kids[v]:
            k += 1
            new[n] = f"node_{k}"
    by_node = {}
    for line in lines[1:]:
        name, _, rest = line.partition("\t")
        by_node.setdefault(new.get(name, name), []).append(rest)
    def grouped(rest):   # ("B" lines first, as they are; then "N" lines by block, stably)
        return sorted(rest, key=lambda r: (r[0] == "N", int(r.split("\t")[1]) if r[0] == "N" else 0))

    return "\n".join(lines[:1] + [f"{n}\t{r}" for n in sorted(by_node) for r in grouped(by_node[n])]) + "\n"


def test_round_trip_through_the_file(engine, random_case, tmp_path):
    pm, sets, want = random_case
    f = engine.subnet(pm, sets["every_other"])
    path = str(tmp_path / "sub.panman")
    f.write(path)
    f.close()
    g = PanmanFile(path)
    try:
        assert ref.sorted_blocks(tree_dump(g)) == _as_loaded(want["every_other"])
    finally:
        g.close()


def _run(args, cwd):
    if not os.path.exists(CLI):
        pytest.fail(f"{CLI} missing: run `make`")
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def test_command_end_to_end(engine, random_case, tmp_path):
    pm, sets, _ = random_case
    path = str(tmp_path / "in.panman")
    write_panman(path, [pm, pm])
    loaded = PanmanFile(path)
    ids = [sets["every_other"], sets["opposite"]]
    want = []
    for i in range(2):
        f = engine.subnet(loaded.view(i), ids[i])
        want.append(_as_loaded(ref.sorted_blocks(tree_dump(f))))
        f.close()
    loaded.close()
    (tmp_path / "ids.txt").write_text("".join(f"{i} " + " ".join(ids[i]) + "\n" for i in (1, 0)))
    r = _run(["-I", path, "--subnet", "-i", "ids.txt", "-o", "sub"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert re.search(r"\nParallel Subnetwork Extract execution time: \d+ nanoseconds\n", r.stdout)
    g = PanmanFile(str(tmp_path / "panman" / "sub.panman"))
    try:
        assert len(g) == 2
        assert [ref.sorted_blocks(tree_dump(g, i)) for i in range(2)] == want
    finally:
        g.close()
    (tmp_path / "ids.txt").write_text("0 " + " ".join(ids[0]) + "\n")
    r = _run(["-I", path, "-b", "-i", "ids.txt", "-o", "sub2"], tmp_path)
    assert r.returncode != 0 and "tree 1" in r.stderr and not (tmp_path / "panman" / "sub2.panman").exists()
    (tmp_path / "ids.txt").write_text("0 nope\n1 " + " ".join(ids[1]) + "\n")
    r = _run(["-I", path, "-b", "-i", "ids.txt", "-o", "sub3"], tmp_path)
    assert r.returncode != 0 and "don't exist" in r.stderr


# ---- errors and the binding --------------------------------------------------------------------------------

def test_unknown_and_empty_requests(engine, random_case):
    pm, _, _ = random_case
    with pytest.raises(panman_amd.PanmanError, match="Some of the specified node identifiers don't exist!!!"):
        engine.subnet(pm, [pm.names[pm.leaves()[0]], "nope"])
    with pytest.raises(panman_amd.PanmanError, match="rc=-1"):
        engine.subnet(pm, [])


def test_secondary_blocks(engine):
    """Refused on a merged chain, as pm_reroot refuses them; copied on a node that merges with nothing."""
    pm, chain = _spine(2)
    pm.add_nuc_mut(chain[1], 0, 5, -1, S, [2], secondary=3)
    with pytest.raises(panman_amd.PanmanError, match="rc=-4.*secondary blocks"):
        engine.subnet(pm, ["t2"])
    f = engine.subnet(pm, ["t0", "t1", "t2"])
    try:
        a = f.to_panmat(0)._arrays
        assert list(a["nuc_mut_secondary"]) == [3] and list(a["nuc_mut_position"]) == [5]
    finally:
        f.close()


@pytest.mark.parametrize("old,new,words", [
    ((1, 0), (1, 0), "Block insertion followed by insertion doesn't make sense"),
    ((0, 0), (0, 0), "Block deletion followed by inversion or deletion doesn't make sense"),
    ((0, 0), (0, 1), "Block deletion followed by inversion or deletion doesn't make sense"),
    ((0, 1), (1, 0), "Block inversion followed by insertion doesn't make sense")])
def test_raising_block_pairs(engine, old, new, words):
    pm, chain = _spine(2, block_lens=(40, 40))
    pm.block_muts[chain[0]] = [(0, 1, 0)]   # the root inserts block 0 only: `old` is block 1's first mutation
    pm.add_block_mut(chain[0], 1, *old)
    pm.add_block_mut(chain[2], 1, *new)
    with pytest.raises(panman_amd.PanmanError, match=re.escape(words)):
        engine.subnet(pm, ["t2"])
    with pytest.raises(ValueError, match=re.escape(words)):
        ref.subnet(pm, ["t2"])


def test_coordinate_outside_its_block_is_an_error(engine):
    pm, chain = _spine(2, block_lens=(40,), gaps=[(0, [(7, 2)])])
    pm.add_nuc_mut(chain[2], 0, 7, 1, ref.NI, [1, 2])   # gap slots 1 and 2 of a slot range of 2
    with pytest.raises(panman_amd.PanmanError, match="rc=-1.*gap-slot"):
        engine.subnet(pm, ["t2"])
    pm.nuc_muts[chain[2]] = []
    pm.add_nuc_mut(chain[0], 0, 39, -1, ref.NS, [1, 2, 4])   # positions 39, 40 (the sentinel) and 41
    with pytest.raises(panman_amd.PanmanError, match="rc=-1.*beyond the block"):
        engine.subnet(pm, ["t2"])


def test_symbol_is_exported_and_bound():
    assert "pm_subnet" in header_symbols() and hasattr(load(), "pm_subnet")
    assert "PM_OPT_SUBNET_BATCH_ENTRIES 24" in open(os.path.join(ROOT, "include", "panman_gpu.h")).read()
