"""The restatement of panmanToUsher (tests/_usher_ref.py) pinned by hand: every expected byte string is
written out in tests/_usher_cases.py beside its case, with the lines of src/panman2usher.cpp it follows
-- a substitution over a consensus base, an insertion into a gap slot (ref and par absent), a deletion
run (mut_nuc 0, 1, 2, 3), an IUPAC code and code 0, the sentinel, a type-6 mutation, the empty node
12 00, the root's own list, a cell written twice in one list and again in a child, and block deletions
and inversions that change nothing."""
import pytest

import _usher_ref
from _usher_cases import HAND, NEWICK3, NEWICK4, block_mutations_case, without_block_mutations


@pytest.mark.parametrize("name", list(HAND))
def test_hand_case(name):
    pm, want = HAND[name]()
    got, count = _usher_ref.to_usher(pm)
    assert got == want, _usher_ref.first_difference(got, want)
    text, nodes = _usher_ref.decode(want)
    assert len(nodes) == pm.num_nodes and count == sum(map(len, nodes))
    assert text == _usher_ref.newick(pm)


def test_newick_field_lengths():
    assert NEWICK3[1] == len(NEWICK3) - 2 == 34 and NEWICK4[1] == len(NEWICK4) - 2 == 46


def test_empty_node_and_record_layout():
    """12 00 is an empty mutation_list; a record is 0a len (08 position) [10 ref] [18 par] 22 n bits."""
    assert _usher_ref.encode("x", [[]]) == b"\x0a\x01x\x12\x00"
    assert _usher_ref.encode_mut(300, 0, 15, [0, 3]) == bytes.fromhex("08ac02 180f 22020003")
    assert _usher_ref.decode(b"\x0a\x01x\x12\x00\x12\x07\x0a\x05\x08\x07\x22\x01\x00") == ("x", [[], [(7, 0, 0, [0])]])


def test_block_mutations_change_nothing():
    pm, want = block_mutations_case()
    assert any(pm.block_muts[v] for v in range(1, pm.num_nodes))
    assert _usher_ref.to_usher(without_block_mutations(pm))[0] == want


def test_refusals():
    from _usher_cases import ARG_ERRORS, UNSUPPORTED
    for build in ARG_ERRORS.values():
        with pytest.raises(_usher_ref.ArgError):
            _usher_ref.to_usher(build())
    for build in UNSUPPORTED.values():
        with pytest.raises(_usher_ref.Unsupported):
            _usher_ref.to_usher(build())
