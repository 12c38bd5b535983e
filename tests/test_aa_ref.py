"""tests/_aa_ref.py, the literal restatement of Tree::extractAminoAcidTranslations
(src/aaTrans.cpp:185-304) that pm_aa is compared against, pinned by hand-derived cases: the codon
table, the windows and strings of tests/_aa_cases.py, the error cases, and the order-free form of
the merge (the one the kernels use) against the literal two-pointer loop.  CPU only."""
import numpy as np
import pytest

import _aa_ref
from _aa_cases import HAND, issue_case, random_case, RANDOM, reverse_case, short_block0_case, slot_end_case, slot_start_case, \
    absent_case, text_of, unsupported_case
from _maf_ref import _parents, _path


def _state(pm, name):
    max_id = max(b for b, _ in pm.blocks)
    return _aa_ref.NodeState(pm, _path(pm, _parents(pm), pm.index(name)), max_id, {b for b, _ in pm.blocks})


def _window(pm, name, start, end):
    s = _state(pm, name)
    return _aa_ref.window(s, _aa_ref.locate(s, start), _aa_ref.locate(s, end))


def test_codon_table():
    t = _aa_ref.CODON_TABLE
    assert len(t) == 64 and all(len(c) == 3 and set(c) <= set("ACGT") for c in t)
    assert t["ATG"] == "Met" and t["TGG"] == "Trp"
    assert {c for c, a in t.items() if a == "*"} == {"TAA", "TAG", "TGA"}
    count = {}
    for a in t.values():
        count[a] = count.get(a, 0) + 1
    assert count["Leu"] == count["Ser"] == count["Arg"] == 6 and count["Met"] == count["Trp"] == 1
    assert len(count) == 21 and sum(count.values()) == 64
    assert {a: n for a, n in count.items() if n == 4} == dict.fromkeys(["Val", "Pro", "Thr", "Ala", "Gly"], 4)
    assert count["Ile"] == 3 and t["GAT"] == "Asp" and t["AAG"] == "Lys" and t["CCT"] == "Pro" and t["GGG"] == "Gly"


@pytest.mark.parametrize("name", list(HAND))
def test_hand_case(name):
    pm, start, end, want, ref_codons = HAND[name]()
    assert _aa_ref.aa(pm, start, end) == (text_of(pm, want), ref_codons, 0)


def test_issue_case_windows():
    pm, start, end, _, _ = issue_case()
    assert _window(pm, "r", start, end) == "ATGGCCTAA"
    assert _window(pm, "b", start, end) == "ATG-CCTAAG"      # its own end lands on position 10
    assert _window(pm, "c", start, end) == "ATG---TAAGGG"
    assert _window(pm, "u", start, end) == "NTGGCCTAA"
    assert _aa_ref.codons("ATGGCCTAA") == (["Met", "Ala", "*"], [0, 3, 6], [2, 5, 8])
    assert _aa_ref.codons("ATG---TAAGGG") == (["Met", "*", "Gly"], [0, 6, 9], [2, 8, 11])
    assert _aa_ref.codons("NTGGCCTAA") == (["Trp", "Pro"], [1, 4], [3, 6])   # the last group is incomplete
    text, _, _ = _aa_ref.aa(pm, start, end)
    assert "r\t" not in text                                                 # the root prints no line


def test_slot_start_leaves_out_lower_slots():
    pm, start, end, _, _ = slot_start_case()
    s = _state(pm, "r")
    assert _aa_ref.locate(s, start) == (0, 2, 1) and _aa_ref.locate(s, end) == (0, 8, -1)
    assert _window(pm, "r", start, end) == "TGTAGCGT"    # position 5: slot 1 and the main character, not slot 0
    assert _window(pm, "r", 2, end) == "TTGTAGGCGT"      # from slot 0: every slot
    assert _window(pm, "r", 4, end) == "GTACGT"          # from a main character: no slot at all


def test_end_on_a_slot_is_an_error_window():
    pm, start, end, _, _ = slot_end_case()
    s = _state(pm, "e")
    assert _aa_ref.locate(s, end) == (0, 8, 0)
    assert _window(pm, "e", start, end) is None and _aa_ref.codons(None) == ([], [], [])
    assert _window(pm, "r", start, end) == "ATGGCCTA"


def test_reverse_block_windows():
    pm, start, end, _, _ = reverse_case()
    s = _state(pm, "r")
    assert s.forward == [False, True] and _aa_ref.locate(s, start) == (0, 4, -1)
    assert _window(pm, "r", start, end) == "CCGGGATGA"
    g = _state(pm, "g")
    assert g.forward == [False, False] and _aa_ref.locate(g, end) == (1, 1, -1)
    assert _window(pm, "g", start, end) == "CCGGGxAAAG"  # block 1 from block 0's last index: the sentinel
    pm, start, end, _, _ = short_block0_case()
    assert _window(pm, "r", start, end) == "ACGxGT"      # block 1 from index 3, not from its end


def test_absent_block_window():
    pm, start, end, _, _ = absent_case()
    assert _window(pm, "r", start, end) == "ATGAAAxCCCGGGxTT"
    assert _window(pm, "h", start, end) == "ATGAAAx-------TTTACGTC"


def test_wrapping_and_argument_errors():
    pm, _, _, _, _ = issue_case()                        # L = 13 on every node but b and c
    s = _state(pm, "r")
    assert _aa_ref.locate(s, 13) == (0, 0, -1) and _aa_ref.locate(s, 25) == (0, 12, -1)
    assert _aa_ref.locate(s, 26) is None and _aa_ref.locate(s, -1) is None
    assert _aa_ref.aa(pm, 13, 14) == ("", 0, 0)          # both wrap: the window "A", no codon, no header
    with pytest.raises(_aa_ref.ArgError):
        _aa_ref.aa(pm, 2, 13)                            # the end wraps in front of the start: the root's window is ERROR
    with pytest.raises(_aa_ref.ArgError):
        _aa_ref.aa(pm, 9, 9)
    with pytest.raises(_aa_ref.ArgError):
        _aa_ref.aa(pm, 9, 3)
    with pytest.raises(_aa_ref.ArgError):
        _aa_ref.aa(pm, 0, 26)                            # the root unlocated
    with pytest.raises(_aa_ref.ArgError):
        _aa_ref.aa(pm, -1, 5)
    # a node's end wraps: node c holds 10 bases, so 10 is its first base again and its window is empty
    text, ref_codons, unlocated = _aa_ref.aa(pm, 0, 10)
    assert ref_codons == 3 and unlocated == 0 and "c\tD:0;D:1;D:2;\n" in text
    # ... and 23 is not found on c (23 - 10 = 13 >= 10): counted, no line
    text, ref_codons, unlocated = _aa_ref.aa(pm, 14, 23)
    assert unlocated == 1 and "c\t" not in text and ref_codons == 3


def test_unsupported():
    pm, start, end = unsupported_case()
    with pytest.raises(_aa_ref.Unsupported):
        _aa_ref.aa(pm, start, end)
    assert _aa_ref.aa(pm, 0, 6)[1] == 2                  # the window ends inside block 0: defined
    pm, start, end, _, _ = issue_case()
    pm.add_nuc_mut(pm.index("a"), 0, 1, -1, 3, [8], secondary=0)
    with pytest.raises(_aa_ref.Unsupported):
        _aa_ref.aa(pm, start, end)


@pytest.mark.parametrize("leaves,k,seed", RANDOM)
def test_random_cases_are_defined(leaves, k, seed):
    pm, start, end = random_case(leaves, k, seed)
    text, ref_codons, unlocated = _aa_ref.aa(pm, start, end)    # neither Unsupported nor an argument error
    assert unlocated == 0 and 0 <= start < end


def test_random_cases_cover_the_ground():
    seen = set()
    for leaves, k, seed in RANDOM:
        pm, start, end = random_case(leaves, k, seed)
        text, ref_codons, _ = _aa_ref.aa(pm, start, end)
        for kind in "SID":
            if f"\t{kind}:" in text or f";{kind}:" in text:
                seen.add(kind)
        if any(ins == 0 and not inv for muts in pm.block_muts for _, ins, inv in muts):
            seen.add("absent")
        if any(gap != -1 and (info & 7) in (0, 2, 3, 4) for muts in pm.nuc_muts for _, _, _, gap, info, _ in muts):
            seen.add("slots")
    assert seen == {"S", "I", "D", "absent", "slots"}


def _literal(ref_starts, ref_ends, alt_starts):
    return _aa_ref.merge(ref_starts, ref_ends, alt_starts)


def _intervals(rng, n, span):
    """n codons inside [0, span): disjoint (start, end) pairs, end >= start + 2, ascending."""
    cuts = np.sort(rng.choice(span, size=2 * n, replace=False))
    starts, ends = [], []
    at = -1
    for k in range(n):
        s = max(int(cuts[2 * k]), at + 1)
        e = max(int(cuts[2 * k + 1]), s + 2)
        starts.append(s)
        ends.append(e)
        at = e
    return starts, ends


def test_order_free_merge_equals_the_loop():
    rng = np.random.default_rng(11)
    kinds = {"match": 0, "ins_before": 0, "ins_inside": 0, "del": 0}
    for trial in range(4000):
        n, m = int(rng.integers(0, 12)), int(rng.integers(0, 12))
        span = int(rng.integers(8 * max(n, m, 1), 40 * max(n, m, 1) + 1))
        ref_starts, ref_ends = _intervals(rng, n, span)
        alt_starts, _ = _intervals(rng, m, span)
        want = _literal(ref_starts, ref_ends, alt_starts)
        got = _aa_ref.merge_order_free(ref_starts, ref_ends, alt_starts)
        assert got == want, (ref_starts, ref_ends, alt_starts)
        matched = {q for q, _ in want[0]}
        kinds["match"] += len(want[0])
        kinds["del"] += len(want[2])
        for q, a in want[1]:
            inside = q - 1 in matched and q >= 1 and alt_starts[a] <= ref_ends[q - 1]
            kinds["ins_inside" if inside else "ins_before"] += 1
    assert all(v > 500 for v in kinds.values()), kinds
