"""Pin the Python GFA reference (tests/_gfa_ref.py) to src/gfa.cpp:3-500 by hand cases, and tie it
to the oracle's FASTA path by a round trip: the sequence a tip's "P" line spells is its unaligned
FASTA record."""
import pytest

from _gfa_cases import HAND, hand_panmat, random_case
from _gfa_ref import gfa, gfa_to_sequences
from _panmat import parse_records


@pytest.mark.parametrize("name", list(HAND))
def test_hand_case(name):
    case, want = HAND[name]
    assert gfa(hand_panmat(case)) == want


def test_reading_back_the_hand_cases():
    assert gfa_to_sequences(HAND["A_two_tips_one_chunk"][1]) == {"t0": "ACGT" * 8 + "ACGAACG", "t1": "ACGT" * 9 + "ACG"}
    # the reverse strand: the complement of "ACGT" * 9 + "ACG" read backwards
    assert gfa_to_sequences(HAND["B_reverse_strand_40_columns"][1])["t1"] == "CGT" + "ACGT" * 9
    assert gfa_to_sequences(HAND["C_chunk_strips_to_nothing"][1]) == {"t0": "TACGT", "t1": "ACGT"}
    assert gfa_to_sequences(HAND["D_chain_merges"][1]) == {"t0": "CCGT" + "ACGT" * 24, "t1": "ACGT" * 25}
    assert gfa_to_sequences(HAND["E_whole_blocks_with_an_inversion"][1]) == {"t0": "ACGGGGG", "t1": "ACGTTGGGG"}


ROUND_TRIP = [(60, 1), (60, 2), (60, 3)]   # (leaves, seed)


def broken_by(tip, notes):
    """The named reference rule that breaks this tip's own path, or None.
    "collision": one of its steps is a node the other strand made -- the start tuples of block
    0's reverse gap-slot chunks equal forward ones (gfa.cpp:253) -- and the path filter drops it
    (:446: finalNodes is keyed by the creator's strand).
    "&&": it passes a node of a merge that the && of :379 let through where the tips or the
    predecessors of the two nodes differ, so a text it needs is erased or one it does not is added."""
    steps = notes["paths"][tip]
    if any(notes["creator"][i] != strand for i, strand in steps):
        return "collision"
    if any(step in notes["loose"] for step in steps):
        return "&&"
    return None


def round_trip(pm, fasta_text, text, notes):
    """(compared, left out): every tip's sequence read back from the GFA equals its unaligned
    FASTA record; a tip is left out only when broken_by names the rule."""
    want = parse_records(fasta_text)
    got = gfa_to_sequences(text)
    compared = left_out = 0
    for t in pm.leaves():
        name = pm.names[t]
        if got[name] != want[name]:
            assert broken_by(t, notes) is not None, name
            left_out += 1
            continue
        compared += 1
    return compared, left_out


def test_round_trip_against_the_oracle(oracle):
    compared = left_out = 0
    for leaves, seed in ROUND_TRIP:
        pm = random_case(leaves, seed)
        notes = {}
        text = gfa(pm, notes)
        c, l = round_trip(pm, oracle.fasta(pm, False), text, notes)
        compared += c
        left_out += l
    print(f"compared {compared}, left out {left_out}")
    assert compared >= 100
    assert left_out * 20 <= compared + left_out
