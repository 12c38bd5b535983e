"""The Python restatement of the GFA construction (tests/_gfa_in_ref.py) pinned by hand cases
worked from the reference's source (src/panman.cpp:728-819, :6060-6197; src/chaining.cpp), and
the fixed seeds of its random inputs checked for the two order ambiguities."""
import numpy as np
import pytest

from _gfa_in_ref import (AMBIGUOUS_SEEDS, UNAMBIGUOUS_SEEDS, Ambiguous, aligned_codes, block_order, build, chaining,
                         parse, random_gfa)

BI, BD = 1, 0


def gfa_text(segments: dict, paths: dict) -> str:
    return "".join(f"S\t{k}\t{v}\n" for k, v in segments.items()) + \
        "".join(f"P\t{k}\t{v}\t*\n" for k, v in paths.items())


CASE1 = (gfa_text({"s1": "ACG", "s2": "TT", "s3": "GAC"}, {"a": "s1+,s2+,s3+", "b": "s1+,s3+"}), "(a,b);")
CASE2 = (gfa_text({"A": "AAC", "B": "CCG", "C": "GGT", "D": "TTA", "E": "ACGT"},
                  {"a": "A+,B+,C+,D+,E+", "b": "D+,E+,A+,B+,C+"}), "(a,b);")
CASE3 = (gfa_text({"s1": "ACG", "s2": "TTG"}, {"a": "s1+,s2+", "b": "s1+,s2-"}), "(a,b);")


def test_parse_records_and_path_order():
    text = "H\tVN:Z:1.0\nS\tx\tAC\n\nS\tx\tGG\nL\tx\t+\tx\t+\t0M\nP\tb\tx+,x-\t*\nP\tB\tx-\t*\nP\tb\tx-\t*\nW\tignored\n"
    nodes, paths = parse(text)
    assert nodes == {"x": "GG"}                                             # a later duplicate wins
    assert paths == [("B", [("x", False)]), ("b", [("x", False)])]          # byte order; the later "b" wins


def test_case1_a_skipped_segment(oracle):
    b = build(*CASE1)
    assert b.blocks == ["ACG", "TT", "GAC"]
    assert b.rows["a"].tolist() == [1, 1, 1] and b.rows["b"].tolist() == [1, 0, 1]
    assert b.records(oracle) == {("node_1", 0, BI, 0), ("node_1", 2, BI, 0), ("a", 1, BI, 0)}


def test_case2_a_rearrangement(oracle):
    nodes, paths = parse(CASE2[0])
    chain, best = chaining([s for s, _ in paths[0][1]], [s for s, _ in paths[1][1]])
    assert best == (106, (2, 4)) and chain == [(2, 4), (1, 3), (0, 2)]
    order, seqs = block_order(paths)
    assert order == ["D", "E", "A", "B", "C", "D", "E"]
    assert seqs == [[2, 3, 4, 5, 6], [0, 1, 2, 3, 4]]
    b = build(*CASE2)
    assert b.blocks == [nodes[s] for s in order] and len(b.blocks) == 7
    assert b.rows["a"].tolist() == [0, 0, 1, 1, 1, 1, 1] and b.rows["b"].tolist() == [1, 1, 1, 1, 1, 0, 0]
    recs = b.records(oracle)
    assert {r for r in recs if r[0] == "node_1"} == {("node_1", k, BI, 0) for k in (2, 3, 4)}
    assert {r for r in recs if r[0] == "a"} == {("a", 5, BI, 0), ("a", 6, BI, 0)}
    assert {r for r in recs if r[0] == "b"} == {("b", 0, BI, 0), ("b", 1, BI, 0)}


def test_case3_a_reverse_strand(oracle):
    b = build(*CASE3)
    assert b.rows["a"].tolist() == [1, 1] and b.rows["b"].tolist() == [1, 2]
    assert b.records(oracle) == {("node_1", 0, BI, 0), ("node_1", 1, BI, 0), ("b", 1, BD, 1)}


def test_the_walk_stops_at_a_step_behind_it():
    """The two-pointer walk as written: a step whose block lies behind p1 is never met, nor any after."""
    assert aligned_codes(5, [1, 3], [True, False]).tolist() == [0, 1, 0, 2, 0]
    assert aligned_codes(5, [2, 1, 4], [True, True, True]).tolist() == [0, 0, 1, 0, 0]
    assert aligned_codes(3, [], []).tolist() == [0, 0, 0]


def test_a_first_path_without_steps_and_an_unmatched_path():
    order, seqs = block_order([("a", []), ("b", [("x", True), ("y", True)]), ("c", [("z", True)])])
    assert order == ["x", "y", "z"] and seqs == [[], [0, 1], [2]]


def test_ambiguities_raise():
    with pytest.raises(Ambiguous):   # b repeats x: equal-x points
        build(gfa_text({"x": "A", "y": "C"}, {"a": "x+,y+", "b": "x+,x+"}), "(a,b);")
    with pytest.raises(Ambiguous):   # a swap: (0, 1) and (1, 0) both score 10
        build(gfa_text({"x": "A", "y": "C"}, {"a": "x+,y+", "b": "y+,x+"}), "(a,b);")


@pytest.mark.parametrize("seed", UNAMBIGUOUS_SEEDS)
def test_fixed_seeds_are_unambiguous(seed):
    text, newick = random_gfa(seed)
    b = build(text, newick)
    segments = sum(line.startswith("S\t") for line in text.split("\n"))
    assert 5 <= segments <= 40 and 8 <= b.codes.shape[0] <= 30
    assert b.codes.shape[1] == len(b.blocks) >= 5
    assert (b.codes == 2).any() and (b.codes == 0).any()


def test_the_seeds_cover_the_cases():
    built = [build(*random_gfa(seed)) for seed in UNAMBIGUOUS_SEEDS]
    texts = [random_gfa(seed)[0] for seed in UNAMBIGUOUS_SEEDS]
    assert any(len(b.blocks) > sum(line.startswith("S\t") for line in t.split("\n")) for b, t in zip(built, texts))   # moved runs
    assert any((np.diff(b.off) > 2).any() for b in built) and any((np.diff(b.off) <= 2).all() for b in built)       # polytomies
    assert any(((b.node_row < 0) & (np.diff(b.off) == 0)).any() for b in built)                                      # leaves without a path
    for seed in AMBIGUOUS_SEEDS:
        with pytest.raises(Ambiguous):
            build(*random_gfa(seed))
