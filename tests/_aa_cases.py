"""PanMATs for the amino-acid translation tests (tests/test_aa_ref.py on the CPU,
tests/test_gpu_aa.py and tests/test_cli_aa.py on the GPU): hand cases with their expected
results, the random cases and single-block stars for the kernels' edges."""
from __future__ import annotations

import numpy as np

import _aa_ref
from _maf_ref import _parents, _path
from _panmat import random_panmat
from _trees import names_for, random_tree
from panman_amd.panmat import PanMAT

A, C, G, T, N = 1, 2, 4, 8, 15
NS, ND, NI, SNP, SNP_INS, SNP_DEL = 0, 1, 2, 3, 4, 5   # nucleotide mutation types


def tree(spec: dict, root: str) -> PanMAT:
    """spec: {parent name: [child names]}; nodes are numbered in order of first mention, root first."""
    names = [root]
    for parent, kids in spec.items():
        for n in [parent] + kids:
            if n not in names:
                names.append(n)
    off, idx = [0], []
    for n in names:
        idx += [names.index(k) for k in spec.get(n, [])]
        off.append(len(idx))
    return PanMAT(names, np.array(off, np.int32), np.array(idx, np.int32), 0)


def _snp(pm, node, block, pos, code, gap=-1):
    pm.add_nuc_mut(pm.index(node), block, pos, gap, SNP, [code])


def issue_case():
    """One block, no gaps; a SNP, a single-base deletion, a run deletion, an N, an unchanged child."""
    pm = tree({"r": ["a", "b", "c", "u"], "u": ["d"]}, "r")
    pm.add_block(0, "ATGGCCTAAGGGG")
    pm.add_block_mut(0, 0, True, False)
    _snp(pm, "a", 0, 4, A)
    pm.add_nuc_mut(pm.index("b"), 0, 3, -1, SNP_DEL, [0])
    pm.add_nuc_mut(pm.index("c"), 0, 3, -1, ND, [0, 0, 0])
    _snp(pm, "u", 0, 0, N)
    want = {"a": "S:1:Asp;", "b": "S:1:Pro;S:2:Lys;", "c": "I:3:Gly;D:1;", "u": "S:0:Trp;S:1:Pro;D:2;",
            "d": "S:0:Trp;S:1:Pro;D:2;"}
    return pm, 0, 9, want, 3


def slot_start_case():
    """start on gap slot 1 of position 2; position 5 has slots 0 and 1 filled: its slot 0 is left out."""
    pm = tree({"r": ["x", "y"]}, "r")
    pm.add_block(0, "ACGTACGTAC")
    pm.add_gaps(0, [(2, 2), (5, 2)])
    pm.add_block_mut(0, 0, True, False)
    pm.add_nuc_mut(0, 0, 2, 0, NI, [T, T])
    pm.add_nuc_mut(0, 0, 5, 0, NI, [G, G])
    _snp(pm, "x", 0, 3, A)            # TGT AGC -> TGA AGC
    _snp(pm, "y", 0, 5, A, gap=0)     # the slot the walk leaves out: no change
    return pm, 3, 12, {"x": "S:0:*;"}, 2


def slot_end_case():
    """start a main position; node e's end falls on a filled gap slot: its window is ERROR."""
    pm = tree({"r": ["e", "f"]}, "r")
    pm.add_block(0, "ATGGCCTAAGGG")
    pm.add_gaps(0, [(8, 1)])
    pm.add_block_mut(0, 0, True, False)
    pm.add_nuc_mut(pm.index("e"), 0, 8, 0, SNP_INS, [C])
    _snp(pm, "f", 0, 1, C)            # ATG -> ACG
    return pm, 0, 8, {"e": "D:0;D:1;", "f": "S:0:Thr;"}, 2


def reverse_case():
    """Block 0 on the reverse strand starts the window; node g also reverses block 1, whose walk
    then starts at block 0's last index: the sentinel, printed as a dash inside a codon."""
    pm = tree({"r": ["f", "g", "h"]}, "r")
    pm.add_block(0, "GGGCCC")
    pm.add_block(1, "ATGAAA")
    pm.add_block_mut(0, 0, True, True)
    pm.add_block_mut(0, 1, True, False)
    _snp(pm, "f", 0, 3, A)            # CCG -> CAG
    pm.add_block_mut(pm.index("g"), 1, False, True)
    _snp(pm, "h", 0, 2, T)            # CCG GGA -> CCT GGA: the same amino acids, no line
    return pm, 1, 10, {"f": "S:0:Gln;", "g": "S:2:Lys;"}, 3


def absent_case():
    """Node h lost block 1: seven dashes inside its window, and its own end lies further right."""
    pm = tree({"r": ["h", "i"]}, "r")
    pm.add_block(0, "ATGAAA")
    pm.add_block(1, "CCCGGG")
    pm.add_block(2, "TTTACGTCA")
    for b in range(3):
        pm.add_block_mut(0, b, True, False)
    pm.add_block_mut(pm.index("h"), 1, False, False)
    return pm, 0, 14, {"h": "I:4:Phe;I:4:Thr;D:2;D:3;"}, 4


def short_block0_case():
    """Block 1 on the reverse strand is longer than block 0: its walk starts at block 0's last
    index, inside it (defined, and not at its end)."""
    pm = tree({"r": ["k"]}, "r")
    pm.add_block(0, "ACG")
    pm.add_block(1, "TTTGGGCCC")
    pm.add_block_mut(0, 0, True, False)
    pm.add_block_mut(0, 1, True, True)
    _snp(pm, "k", 0, 0, G)
    return pm, 0, 10, {"k": "S:0:Ala;"}, 1


def unsupported_case():
    """Block 1 on the reverse strand is shorter than block 0: the reference indexes out of range."""
    pm = tree({"r": ["k"]}, "r")
    pm.add_block(0, "ACGTACGT")
    pm.add_block(1, "ACG")
    pm.add_block_mut(0, 0, True, False)
    pm.add_block_mut(0, 1, True, True)
    return pm, 0, 9


HAND = {"issue": issue_case, "slot_start": slot_start_case, "slot_end": slot_end_case, "reverse": reverse_case,
        "absent": absent_case, "short_block0": short_block0_case}


def text_of(pm, want: dict) -> str:
    """The text of `want` ({name: string}) in node-id order."""
    return "node_id\taa_mutations\n" + "".join(f"{n}\t{want[n]}\n" for n in pm.names if n in want)


def lengths(pm):
    """L of every node: the characters of its held blocks that are neither '-' nor 'x'."""
    parent = _parents(pm)
    max_id = max(b for b, _ in pm.blocks)
    is_block = {b for b, _ in pm.blocks}
    out = []
    for v in range(pm.num_nodes):
        s = _aa_ref.NodeState(pm, _path(pm, parent, v), max_id, is_block)
        out.append(sum((m not in "-x") + sum(ch not in "-x" for ch in sl)
                       for b, seq in enumerate(s.seq) if s.held[b] for m, sl in seq))
    return out


def random_case(leaves: int, k: int, seed: int, blocks: int = 6):
    """random_panmat with `blocks` blocks of k bases each (equal lengths keep every reverse-strand walk
    defined) and start < end below the smallest L of its nodes."""
    rng = np.random.default_rng(seed)
    off, idx, root = random_tree(leaves, rng, unary=0.1)
    pm = random_panmat(rng, off, idx, root, names_for(off), blocks=blocks, block_len=(k, k + 1))
    low = min(lengths(pm))
    assert low >= 2, (leaves, k, seed)
    start = int(rng.integers(0, low - 1))
    end = int(rng.integers(start + 1, low))
    return pm, start, end


RANDOM = [(1, 9, 1), (2, 9, 2), (30, 5, 3), (30, 17, 4), (30, 40, 5), (30, 40, 6), (2, 40, 7), (30, 64, 8)]


def star(names, length: int, seed: int, edits=()):
    """One block of `length` random bases under a root with the leaves `names`; every leaf gets
    a few SNPs, and `edits` adds (leaf name, position, type, codes) on top."""
    rng = np.random.default_rng(seed)
    pm = tree({"root": list(names)}, "root")
    pm.add_block(0, "".join(rng.choice(list("ACGT"), size=length)))
    pm.add_block_mut(0, 0, True, False)
    for n in names:
        for pos in sorted(set(rng.integers(0, length, size=max(2, length // 40)).tolist())):
            _snp(pm, n, 0, int(pos), int(rng.choice([A, C, G, T])))
    for name, pos, typ, codes in edits:
        pm.add_nuc_mut(pm.index(name), 0, pos, -1, typ, list(codes))
    return pm
