"""The plain-Python restatement of the N imputation (tests/_impute_ref.py) against answers worked out by hand on
the seven-node tree of tests/_impute_cases.py: ((a,b)p,(c,d)q)r, block 0 = ACGTACGTAC with 4 gap slots at
positions 3 and 7.  Record lines are "block position gap info nucs"; info = length << 4 | type with NS 0, ND 1,
NI 2, NSNPS 3, NSNPI 4, NSNPD 5; codes A 1, C 2, G 4, T 8, N 15.  CPU only."""
import pytest

import _impute_cases as cases
import _impute_ref as ref


def run(pm, distance=5):
    trace = {}
    out, plan, stats = ref.impute(pm, distance, trace)
    return out, plan.splitlines(), stats, trace


def records(pm, name):
    return [(m[2], m[3], m[4], m[5]) for m in pm.nuc_muts[pm.index(name)]]


def unchanged_but(pm, out, *names):
    return all(out.nuc_muts[v] == pm.nuc_muts[v] for v in range(pm.num_nodes) if pm.names[v] not in names) and \
        out.block_muts == pm.block_muts


def test_ns_all_n_is_erased():
    # a: NS [N N] at 1: erased, nothing comes back; both bases count.
    pm = cases.ns_all_n()
    out, plan, stats, _ = run(pm)
    assert records(out, "a") == [] and unchanged_but(pm, out, "a")
    assert stats == {"imputed_bases": 2, "insertion_nodes": 0, "moves_found": 0, "pairs": 0} and plan == []


def test_ns_partial_comes_back_as_snps_in_place():
    # a: S(0 G), NS(4: A N C N), S(9 G).  The NS is erased; A and C come back where it stood as NSNPS records
    # (info 0x13) at 4 + 0 and 4 + 2; 4 - 2 = 2 bases count.
    out, _, stats, _ = run(cases.ns_partial_main())
    assert records(out, "a") == [(0, -1, 0x13, 0x400000), (4, -1, 0x13, 0x100000), (6, -1, 0x13, 0x200000), (9, -1, 0x13, 0x400000)]
    assert stats["imputed_bases"] == 2
    # in gap slots the slot moves, not the position: slots 0 + 0 and 0 + 2 of position 3
    out, _, stats, _ = run(cases.ns_partial_gap())
    assert records(out, "a") == [(3, 0, 0x13, 0x100000), (3, 2, 0x13, 0x200000)]
    assert stats["imputed_bases"] == 2


def test_nsnps_n_is_erased():
    out, _, stats, _ = run(cases.nsnps_n())
    assert records(out, "a") == [] and stats["imputed_bases"] == 1


def test_n_in_insertion_stays_and_is_an_attempt():
    # a: I(3g0: A N): no substitution, so the list stays; the run holds an N, so a is an attempt; nobody else
    # holds the run: no candidate, no winner.
    pm = cases.n_in_insertion()
    out, plan, stats, trace = run(pm)
    assert unchanged_but(pm, out)
    assert plan == ["a\t1\t0\t.\t-1\t0"] and trace == {"a": []}
    assert stats == {"imputed_bases": 0, "insertion_nodes": 1, "moves_found": 0, "pairs": 0}


def test_root_is_never_visited():
    # the root's NS [N] stays and its insertion of N is no attempt (src/impute.cpp:98 starts below the root)
    pm = cases.root_n()
    out, plan, stats, _ = run(pm)
    assert unchanged_but(pm, out) and plan == []
    assert stats == {"imputed_bases": 0, "insertion_nodes": 0, "moves_found": 0, "pairs": 0}


def test_merge_a_substitution_between_does_not_end_a_run():
    # a: I(3g0: A N), S(0: C), I(3g2: G) is one run (3, slot 0) of 3 with one N; b holds it as one record, not
    # all N: a candidate.  Path: b's list inverted (a deletion of slots 0..2), then a's.  Per cell: slot 0 D, I A
    # -> S A; slot 1 D, I N -> S N; slot 2 D, I G -> S G; position 0: S C.  Sorted and regrouped: S(0: C),
    # NS(3g0: A N G); the N is imputed away, A and G come back.  4 bases before, 3 after: 1.
    _, plan, stats, trace = run(cases.merge_last_run_only())
    assert trace == {"a": ["b"]}
    assert plan == ["a\t1\t1\tb\t1\t0", "a\tN\t0\t0\t-1\t19\t200000", "a\tN\t0\t3\t0\t19\t100000", "a\tN\t0\t3\t2\t19\t400000"]
    assert stats == {"imputed_bases": 0, "insertion_nodes": 1, "moves_found": 1, "pairs": 1}


def test_merge_only_the_last_run_is_a_target():
    # a: I(5: N), I(3g2: A), I(6: C) stays three runs (the third would continue the first), so the N-bearing run
    # is (5, main) of 1, which b holds.  Path: D(5), then a's list: 5: D, I N -> S N, imputed away; the other two
    # insertions stay, sorted (3, slot 2) before (6, main).  3 bases before, 2 after: 1.
    _, plan, _, trace = run(cases.merge_only_last_is_target())
    assert trace == {"a": ["b"]}
    assert plan == ["a\t1\t1\tb\t1\t0", "a\tN\t0\t3\t2\t20\t100000", "a\tN\t0\t6\t-1\t20\t200000"]


def test_merge_main_head_ignores_the_gap_position():
    # a: I(5: N A), I(7g3: C): the head is at gap -1 and 7 - 5 == 2: one run (5, main) of 3, which b holds as
    # I(5: A C G).  Path: D(5..7), then a's list: 5: S N, imputed away; 6: S A; 7: the deletion stays (code 0);
    # 7 slot 3: I C.  3 bases before, 3 after: improvement 0, which beats -1.
    _, plan, _, trace = run(cases.merge_main_head_ignores_gap())
    assert trace == {"a": ["b"]}
    assert plan == ["a\t1\t1\tb\t0\t0", "a\tN\t0\t6\t-1\t19\t100000", "a\tN\t0\t7\t-1\t21\t000000", "a\tN\t0\t7\t3\t20\t200000"]


def test_merge_gap_head_ignores_the_position():
    # a: I(3g0: N A), I(7g2: C): the head is in a slot and 2 - 0 == 2: one run (3, slot 0) of 3, which b holds as
    # I(3g0: A C G).  Path: D(3g0..2), then a's list: slot 0: S N, imputed away; slot 1: S A; slot 2: D stays;
    # 7 slot 2: I C.  Improvement 0.
    _, plan, _, trace = run(cases.merge_gap_head_ignores_position())
    assert trace == {"a": ["b"]}
    assert plan == ["a\t1\t1\tb\t0\t0", "a\tN\t0\t3\t1\t19\t100000", "a\tN\t0\t3\t2\t21\t000000", "a\tN\t0\t7\t2\t20\t200000"]


def test_sibling_donor():
    # a: I(3g0: N N N), S(0: C); b: I(3g0: A C G), S(9: G over C).  Path: b inverted -- D(3g0..2), S(9: C) -- then
    # a's list.  Slots: D, I N -> S N three times, all imputed away; S(0: C) and S(9: C) stay.  4 - 2 = 2.
    _, plan, stats, trace = run(cases.sibling_donor())
    assert trace == {"a": ["b"]}
    assert plan == ["a\t1\t1\tb\t2\t0", "a\tN\t0\t0\t-1\t19\t200000", "a\tN\t0\t9\t-1\t19\t200000"]
    assert stats == {"imputed_bases": 0, "insertion_nodes": 1, "moves_found": 1, "pairs": 1}


def test_donor_alone_gives_the_run_length():
    # with nothing else on the path the new list is empty: the improvement is the run's 3 bases; b and c both
    # give 3 and the first in walk order (p, then b, then up to r, q, c) keeps the place: `>` is strict
    _, plan, stats, trace = run(cases.tie_first_wins())
    assert trace == {"a": ["b", "c"]}
    assert plan == ["a\t1\t2\tb\t3\t0"]
    assert stats == {"imputed_bases": 0, "insertion_nodes": 1, "moves_found": 1, "pairs": 2}


def test_donor_through_the_grandparent():
    # c holds the run.  Path: c inverted, q (empty) inverted, then p's list S(1: T) as it is, then a's.  3 - 1 = 2.
    _, plan, _, trace = run(cases.grandparent_donor())
    assert trace == {"a": ["c"]}
    assert plan == ["a\t1\t1\tc\t2\t0", "a\tN\t0\t1\t-1\t19\t800000"]


@pytest.mark.parametrize("length,distance,sibling,cousin", [
    (0.5, 0, ["b"], ["c"]),     # int(0 - 0.5) is 0 at every step: the walk goes on
    (0.5, -1, [], []),          # below 0 at the start
    (1.0, 1, ["b"], []),        # p 1, b 0; r 0, q -1
    (1.0, 2, ["b"], []),        # r 1, q 0, c -1
    (1.0, 3, ["b"], ["c"]),     # r 2, q 1, c 0
])
def test_distance_edges(length, distance, sibling, cousin):
    assert run(cases.sibling_donor(length), distance)[3] == {"a": sibling}
    assert run(cases.grandparent_donor(length), distance)[3] == {"a": cousin}


def test_block_ratchet():
    # b: (2, 0).  c: nuc 3, but c's inversion of block 1 stays on the path: 0 - 1 = -1 < 0, refused.
    _, plan, _, trace = run(cases.block_ratchet())
    assert trace == {"a": ["b", "c"]}
    assert plan == ["a\t1\t2\tb\t2\t0", "a\tN\t0\t9\t-1\t19\t200000"]


def test_block_deletion_inverted_and_cancelled():
    # c deletes block 1: inverted, an insertion; a's own deletion cancels it: 1 - 0 = 1.
    _, plan, _, _ = run(cases.block_swap())
    assert plan == ["a\t1\t1\tc\t3\t1"]


def test_a_cell_written_twice_is_refused():
    pm = cases.base()
    cases.mut(pm, "a", 0, 1, -1, cases.NS, [cases.A, cases.C])
    cases.mut(pm, "a", 0, 2, -1, cases.NSNPS, [cases.G])
    with pytest.raises(ValueError, match="a cell written twice in one list"):
        ref.impute(pm)
