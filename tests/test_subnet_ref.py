"""The plain-Python restatement of subnetwork extraction (tests/_subnet_ref.py; src/subnet.cpp:3-135,
src/panman.cpp:2033-2085, :2233-2372), pinned without a GPU: the replaceMutation and block tables entry
by entry, the regrouping rule at its edges, and the property that extraction leaves every kept tip's
FASTA record (aligned and unaligned) unchanged.  Plus the --subnet command's argument checks."""
import json
import os
import subprocess

import numpy as np
import pytest

import _subnet_ref as ref
from _pangraph import flatten
from _panmat import parse_records
from _trees import parse_newick
from panman_amd.panmat import PanMAT, from_msa_dump, write_panman

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLI = os.path.join(os.path.dirname(GOLD.rsplit(os.sep, 1)[0]), "bin", "panmanUtils")


def _run(args, cwd):
    if not os.path.exists(CLI):
        pytest.fail(f"{CLI} missing: run `make`")
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


S, I, D = ref.NSNPS, ref.NSNPI, ref.NSNPD


def _snp(typ, pos, code, gap=-1, primary=0):
    return (primary, -1, pos, gap, (1 << 4) + typ, code << 20)


@pytest.mark.parametrize("old,new,want", [
    (S, S, S), (S, I, S), (S, D, D),
    (I, S, I), (I, I, I), (I, D, None),
    (D, S, I), (D, I, S), (D, D, D)])
def test_replace_mutation_table(old, new, want):
    got = ref.replace_mutation((old, 1), (new, 2))
    assert got == (None if want is None else (want, 2))   # always the new code
    # ... and the same through a consolidation of two records at one coordinate
    out = ref.consolidate_nuc([_snp(old, 7, 1), _snp(new, 7, 2)])
    assert out == ([] if want is None else [_snp(want, 7, 2)])


def test_insertion_deletion_insertion_restarts():
    assert ref.consolidate_nuc([_snp(I, 3, 1), _snp(D, 3, 0), _snp(I, 3, 4)]) == [_snp(I, 3, 4)]
    # (without the restart the deletion's result would meet the insertion: D, I -> S)
    assert ref.consolidate_nuc([_snp(I, 3, 1), _snp(D, 3, 0)]) == []


@pytest.mark.parametrize("n,want", [(6, [6]), (7, [6, 1]), (13, [6, 6, 1])])
def test_substitution_runs_are_cut_at_six(n, want):
    codes = [1, 2, 4, 8] * 4
    out = ref.consolidate_nuc([_snp(S, 10 + k, codes[k]) for k in reversed(range(n))])
    assert [(r[4] >> 4) for r in out] == want
    assert [r[2] for r in out] == [10 + 6 * k for k in range(len(want))]
    for k, r in enumerate(out):
        length = want[k]
        assert r[4] & 7 == (ref.NS if length > 1 else S)
        assert [(r[5] >> (4 * (5 - i))) & 15 for i in range(length)] == codes[6 * k:6 * k + length]


def test_gap_entries_break_a_main_run():
    """(p, -1) sorts before (p, 0), (p, 1), so the gap entries at p split p from p + 1."""
    p = 20
    out = ref.consolidate_nuc([_snp(S, p, 1), _snp(S, p + 1, 2), _snp(S, p, 4, gap=0), _snp(S, p, 8, gap=1)])
    assert [(r[2], r[3], r[4]) for r in out] == [(p, -1, (1 << 4) + S), (p, 0, (2 << 4) + ref.NS), (p + 1, -1, (1 << 4) + S)]


def test_gap_slots_that_are_not_adjacent_split():
    out = ref.consolidate_nuc([_snp(I, 5, 1, gap=0), _snp(I, 5, 2, gap=2), _snp(I, 5, 4, gap=3)])
    assert [(r[3], r[4]) for r in out] == [(0, (1 << 4) + I), (2, (2 << 4) + ref.NI)]


INS, INS_INV, DEL, INV = (1, 0), (1, 1), (0, 0), (0, 1)


@pytest.mark.parametrize("old,new,want", [
    (INS, DEL, []), (INS, INV, [INS_INV]), (INS_INV, INV, [INS]), (DEL, INS, []), (INV, DEL, [DEL]), (INV, INV, [])])
def test_block_table_valid_pairs(old, new, want):
    assert ref.consolidate_blocks([(3,) + old, (3,) + new]) == [(3,) + w for w in want]


@pytest.mark.parametrize("old,new,words", [
    (INS, INS, "insertion followed by insertion"), (DEL, DEL, "deletion followed by inversion or deletion"),
    (DEL, INV, "deletion followed by inversion or deletion"), (INV, INS, "inversion followed by insertion")])
def test_block_table_raising_pairs(old, new, words):
    with pytest.raises(ValueError, match=words):
        ref.consolidate_blocks([(3,) + old, (3,) + new])


def test_block_lists_sorted_and_restart():
    got = ref.consolidate_blocks([(5,) + INS, (2,) + DEL, (5,) + DEL, (5,) + INS_INV])
    assert got == [(2,) + DEL, (5,) + INS_INV]


# ---- sequence invariance: the restatement, independently of any GPU code --------------------------

def _random_join_newick(rng, tips):
    pool = [f"t{i}" for i in range(tips)]
    while len(pool) > 1:
        a, b = sorted(rng.choice(len(pool), size=2, replace=False), reverse=True)
        x, y = pool.pop(a), pool.pop(b)
        pool.append(f"({x},{y})")
    return pool[0] + ";"


def _random_msa(seed, tips=12, columns=60):
    rng = np.random.default_rng(seed)
    nwk = _random_join_newick(rng, tips)
    base = rng.choice(list("ACGT"), size=columns)
    rows = {}
    for i in range(tips):
        s = base.copy()
        f = rng.random(columns) < 0.3
        s[f] = rng.choice(list("ACGT-N-"), size=f.sum())
        rows[f"t{i}"] = "".join(s)
    return nwk, "".join(f">{k}\n{v}\n" for k, v in rows.items())


def _sars(oracle):
    """tests/golden/sars_20: its 20 genomes differ in length, so the MSA builder refuses sars_20.fa
    ("sequence lengths don't match"); the PanGraph builder makes the PanMAT from sars_20.json, as
    everywhere else in the suite."""
    nwk = open(os.path.join(GOLD, "sars_20.nwk")).read()
    flat = flatten(json.load(open(os.path.join(GOLD, "sars_20.json"))))
    return ref.panmat_from_m3_dump(oracle.pangraph(flat, nwk), nwk)


@pytest.fixture(scope="module", params=["sars_20", 1, 2, 3])
def built(request, oracle):
    """A PanMAT a builder made (its lists are consistent with the sequences, which lists drawn
    regardless of state are not: there an insertion-then-deletion that cancels changes the sequence in
    the reference too), and every tip's records."""
    if request.param == "sars_20":
        pm = _sars(oracle)
    else:
        nwk, msa = _random_msa(request.param)
        names, off, idx, root = parse_newick(nwk)
        pm = from_msa_dump(oracle.msa_build(nwk, msa, "", mode=0), names, off, idx, root)
    return pm, {al: parse_records(oracle.fasta(pm, al)) for al in (True, False)}


@pytest.mark.parametrize("which", ["one_tip", "siblings", "opposite", "every_other", "all", "internal_and_tip", "root"])
def test_extraction_keeps_every_kept_tip_sequence(oracle, built, which):
    pm, want = built
    ids = ref.standard_subsets(pm)[which]
    sub, _ = ref.subnet(pm, ids)
    tips = {pm.names[v] for v in pm.leaves()}
    kept = tips & set(ids)
    if which == "root":
        assert sub.num_nodes == 1 and sub.names == [pm.names[pm.root]]
    if which == "one_tip":
        assert sub.num_nodes == 1 and sub.names == ids
    sub_tips = {sub.names[v] for v in sub.leaves()}
    assert kept <= sub_tips and (sub_tips - kept <= set(ids))
    for aligned in (True, False):
        got = parse_records(oracle.fasta(sub, aligned))
        for name in sorted(kept):
            assert got[name] == want[aligned][name], (which, name, aligned)


def test_unknown_and_empty_requests():
    names, off, idx, root = parse_newick("((a,b),c);")
    pm = PanMAT(names, off, idx, root)
    with pytest.raises(ValueError, match="don't exist"):
        ref.subnet(pm, ["a", "nope"])
    with pytest.raises(ValueError):
        ref.subnet(pm, [])


# ---- the command's argument checks (no GPU: they come before the context is made) -----------------

def test_cli_subnet_is_a_command(tmp_path):
    r = _run(["-I", "x.panman", "--subnet"], tmp_path)
    assert r.returncode != 0 and "not part of the GPU path" not in r.stderr and "unrecognised" not in r.stderr


def test_cli_subnet_requires_output_and_input_file(tmp_path):
    names, off, idx, root = parse_newick("((a,b),c);")
    pm = PanMAT(names, off, idx, root)
    pm.add_block(0, "ACGTACGT")
    pm.add_block_mut(root, 0, True, False)
    path = str(tmp_path / "in.panman")
    write_panman(path, [pm])
    r = _run(["-I", path, "--subnet"], tmp_path)
    assert r.returncode != 0 and "Output file not provided!" in r.stderr
    r = _run(["-I", path, "-b", "-o", "sub"], tmp_path)
    assert r.returncode != 0 and "Input file not provided!" in r.stderr
    (tmp_path / "ids.txt").write_text("1 a b\n")
    r = _run(["-I", path, "--subnet", "-i", "ids.txt", "-o", "sub"], tmp_path)
    assert r.returncode != 0 and "tree 0" in r.stderr
