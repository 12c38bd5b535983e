"""Pin the Python MAF reference (tests/_maf_ref.py) to src/maf.cpp:68-188 by hand cases, and tie
it to the oracle's FASTA path by the round trip of src/maf.cpp:4-66: the sequences read back
from the MAF text are the unaligned FASTA records."""
import pytest

from _maf_cases import HAND, hand_panmat, random_case
from _maf_ref import maf, maf_to_sequences
from _panmat import parse_records


@pytest.mark.parametrize("name", list(HAND))
def test_hand_case(name):
    case, want = HAND[name]
    assert maf(hand_panmat(case)) == want


def test_groups_order_by_unsigned_words():
    text = maf(hand_panmat(HAND["A"][0]))
    assert text.index("ATG-") < text.index("TA-T-")   # 0x12400000 before 0x88000000


def test_reading_back_the_hand_cases():
    assert maf_to_sequences(HAND["A"][1]) == {"t0": "ATGTAT", "t1": "CG"}
    assert maf_to_sequences(HAND["B_circular"][1]) == {"t0": "ATATGT", "t1": "CG"}   # rotated by 4
    assert maf_to_sequences(HAND["C_inverted"][1]) == {"t0": "TATATG", "t1": "CG"}
    assert maf_to_sequences(HAND["D_reverse_strand"][1]) == {"t0": "ATGATA", "t1": "CG"}


ROUND_TRIP = [(60, 1), (60, 2), (60, 3)]   # (leaves, seed)


def round_trip(pm, fasta_text, text):
    """(compared, left out): every tip's sequence read back from the MAF equals its unaligned
    FASTA record; a tip is left out only when its circular offset is >= its srcSize (the FASTA
    path ignores the offset there, the MAF path does not)."""
    want = parse_records(fasta_text)
    got = maf_to_sequences(text)
    src = {}
    for line in text.split("\n"):
        if line.startswith("s\t"):
            f = line.split("\t")
            src[f[1]] = int(f[5])
    compared = left_out = 0
    for t in pm.leaves():
        name = pm.names[t]
        if name not in src:   # holds no block: an empty record, no line
            assert want[name] == ""
            compared += 1
            continue
        assert src[name] == len(want[name])
        if pm.circular[t] >= 0 and pm.circular[t] >= src[name]:
            left_out += 1
            continue
        assert got[name] == want[name], name
        compared += 1
    return compared, left_out


def test_round_trip_against_the_oracle(oracle):
    compared = left_out = 0
    for leaves, seed in ROUND_TRIP:
        pm = random_case(leaves, seed)
        c, l = round_trip(pm, oracle.fasta(pm, False), maf(pm))
        compared += c
        left_out += l
    print(f"compared {compared}, left out {left_out}")
    assert compared >= 100
    assert left_out * 20 <= compared + left_out
