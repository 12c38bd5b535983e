"""Plain-Python restatement of the reference's N imputation for one tree (Tree::imputeNs, src/impute.cpp:4-337,
up to the plan of moves; NucMut(other, i), Coordinate, IndelPosition::mergeIndels, src/panman.hpp:233-248 and
:316-426; MutationList::invertMutations, src/panman.cpp:2374-2420; getSequenceFromReference for the root,
:4779-4900) over a list-built PanMAT.

It is the literal walk: one running sequence as a dict per cell, every list applied on the way down and undone
from originalNucs on the way up, the tables as dicts (whose insertion order is list order, where the reference's
is its hash maps'), the recursive findNearbyInsertions that builds MutationLists by concatenation, std::find and
erase for every imputed substitution.  It is NOT the replayed rows read at the parent, nor the (node, candidate)
pairs with path steps folded once per coordinate, that pm_impute runs on the GPU.  That the two agree is what the
GPU tests check.  Attempts are taken in node-id order and block lists come out sorted by block id (the
reference's orders are its hash maps'); the moves are not applied."""
from __future__ import annotations

import copy
import sys

import numpy as np

from _subnet_ref import consolidate_blocks, consolidate_nuc
from panman_amd.panmat import PanMAT

NS, ND, NI, NSNPS, NSNPI, NSNPD = 0, 1, 2, 3, 4, 5
N = 15
LETTERS = "-ACMGRSVTWYHKDBN"          # getNucleotideFromCode; anything else: '-'
CODES = {c: i for i, c in enumerate(LETTERS) if i}   # getCodeFromNucleotide; anything else: 0


def length(m):
    return m[4] >> 4


def mtype(m):
    return m[4] & 7


def code(m, i):
    return (m[5] >> (4 * (5 - i))) & 15


def is_sub(m):
    return mtype(m) in (NS, NSNPS)


def is_ins(m):
    return mtype(m) in (NI, NSNPI)


def coordinate(m, i=0):
    """Coordinate(nm, offset): (nucPosition, nucGapPosition, primaryBlockId, secondaryBlockId)."""
    return (m[2] + i, m[3], m[0], m[1]) if m[3] == -1 else (m[2], m[3] + i, m[0], m[1])


def snp_of(m, i):
    """NucMut(other, i) (src/panman.hpp:233-248)."""
    pos, gap = (m[2] + i, m[3]) if m[3] == -1 else (m[2], m[3] + i)
    return (m[0], m[1], pos, gap, NSNPS + (1 << 4), code(m, i) << 20)


def impute_substitution(lst, m):
    """imputeSubstitution (:205-225) on a Python list, in place; the bases dropped."""
    at = lst.index(m)
    del lst[at]
    n = length(m)
    if mtype(m) == NS:
        snps = [snp_of(m, i) for i in range(length(m)) if code(m, i) != N]
        lst[at:at] = snps
        n -= len(snps)
    return n


def impute_all_substitutions(lst):
    """imputeAllSubstitutionsWithNs (:227-241)."""
    for i in range(len(lst) - 1, -1, -1):
        m = lst[i]
        if is_sub(m) and any(code(m, j) == N for j in range(length(m))):
            impute_substitution(lst, m)


def invert(nuc, blk, original, was_inv):
    """MutationList::invertMutations on copies."""
    out = []
    for m in nuc:
        t, info = mtype(m), m[4]
        if t == NSNPI:
            out.append(m[:4] + (info + NSNPD - NSNPI, 0))
        elif t in (NSNPD, NSNPS):
            info += NSNPI - NSNPD if t == NSNPD else 0
            out.append(m[:4] + (info, original[coordinate(m)] << 20))
        elif t == NI:
            out.append(m[:4] + (info + ND - NI, 0))
        else:
            info += NI - ND if t == ND else 0
            nucs = 0
            for i in range(length(m)):
                nucs += original[coordinate(m, i)] << (4 * (5 - i))
            out.append(m[:4] + (info, nucs))
    blocks = []
    for b, ins, inv in blk:
        if ins:
            blocks.append((b, 0, 0))             # convertToDeletion
        elif not inv:
            was_inv[b]                           # wasBlockInv.at(...): the state convertToInsertion is handed ...
            blocks.append((b, 1, inv))           # ... and assigns to its own parameter: the member stays false
        else:
            blocks.append((b, ins, inv))
    return out, blocks


class _Tables:
    pass


def _fill_tables(pm):
    """fillImputationLookupTables (:81-203) with the undo of :121-139."""
    off, idx, root = pm.child_offsets, pm.child_index, pm.root
    kids = lambda v: [int(c) for c in idx[off[v]:off[v + 1]]]
    seq = {}
    for b, words in pm.blocks:
        n = 0
        for w in words:
            stop = False
            for k in range(8):
                c = (w >> (4 * (7 - k))) & 15
                if c == 0:
                    stop = True
                    break
                seq[(b, n, -1)] = LETTERS[c]
                n += 1
            if stop:
                break
        seq[(b, n, -1)] = "x"
    for b, slots in pm.gaps:
        for pos, ln in slots:
            for g in list(seq):
                if g[0] == b and g[1] == pos and g[2] != -1:
                    del seq[g]              # (resize: a later entry of a position replaces an earlier one)
            for g in range(ln):
                seq[(b, pos, g)] = "-"
    exists, strand = {}, {}
    for b, ins, inv in pm.block_muts[root]:
        if ins:
            exists[b], strand[b] = True, not inv
        elif inv:
            strand[b] = not strand.get(b, True)
        else:
            exists[b], strand[b] = False, True
    for m in pm.nuc_muts[root]:
        if not exists.get(m[0], False):
            continue
        n = length(m) if mtype(m) < 3 else 1
        for i in range(n):
            pos, gap, b, _ = coordinate(m, i)
            seq[(b, pos, gap)]   # the cell exists
            seq[(b, pos, gap)] = "-" if mtype(m) in (ND, NSNPD) else LETTERS[code(m, i)]
    t = _Tables()
    t.substitutions, t.insertions, t.original, t.was_inv = [], {root: {}}, {root: {}}, {root: {}}

    def cell(c):
        return (c[2], c[0], c[1])

    def helper(v):
        runs = []
        t.original[v] = {}
        for m in pm.nuc_muts[v]:
            ns = 0
            for i in range(length(m)):
                c = code(m, i)
                at = coordinate(m, i)
                ns += c == N
                if at in t.original[v]:
                    raise ValueError("a cell written twice in one list")
                t.original[v][at] = CODES.get(seq[cell(at)], 0)
                seq[cell(at)] = LETTERS[c]
            if is_sub(m):
                if ns > 0:
                    t.substitutions.append((v, m))
            elif is_ins(m):
                head = runs[-1][0] if runs else None
                # mergeIndels (src/panman.hpp:408-421): [pos, gap, blk, sec, length]
                if head is not None and head[2] == m[0] and head[3] == m[1] and (
                        (head[1] == -1 and m[2] - head[0] == head[4]) or (head[1] != -1 and m[3] - head[1] == head[4])):
                    head[4] += length(m)
                    runs[-1][1] += ns
                else:
                    runs.append([[m[2], m[3], m[0], m[1], length(m)], ns])
        t.insertions[v] = {}
        for head, ns in runs:
            t.insertions[v].setdefault(tuple(head), ns)   # std::inserter into a map does not overwrite
        t.was_inv[v] = {}
        for b, ins, inv in pm.block_muts[v]:
            if not ins and not inv:
                t.was_inv[v][b] = not strand.get(b, True)
        for c in kids(v):
            helper(c)
        for m in pm.nuc_muts[v]:
            for i in range(length(m)):
                at = coordinate(m, i)
                seq[cell(at)] = LETTERS[t.original[v][at]]
        for b, ins, inv in pm.block_muts[v]:
            if inv:
                strand[b] = not strand.get(b, True)

    for c in kids(root):
        helper(c)
    return t


def impute(pm: PanMAT, max_distance: int = 5, trace: dict | None = None, scores: dict | None = None):
    """(the PanMAT with the imputed lists, the plan text, the stats); `trace` receives per attempt (by name) its
    candidates' names in walk order, `scores` their (nucImprovement, blockImprovement)."""
    assert getattr(pm, "_arrays", None) is None, "use a list-built PanMAT"
    sys.setrecursionlimit(100000)
    for lst in pm.nuc_muts:
        for m in lst:
            if m[1] != -1:
                raise ValueError("secondary blocks")
            if length(m) > 6:
                raise ValueError("nucleotide run longer than 6")
    off, idx = pm.child_offsets, pm.child_index
    kids = lambda v: [int(c) for c in idx[off[v]:off[v + 1]]]
    parent = {pm.root: None}
    for v in range(pm.num_nodes):
        for c in kids(v):
            parent[c] = v
    bl = (lambda v: np.float32(0)) if pm.branch_length is None else (lambda v: np.float32(pm.branch_length[v]))
    t = _fill_tables(pm)
    out = copy.copy(pm)
    out.nuc_muts = [list(lst) for lst in pm.nuc_muts]
    out.block_muts = [list(lst) for lst in pm.block_muts]
    imputed = 0
    for v, m in t.substitutions:
        imputed += impute_substitution(out.nuc_muts[v], m)

    def nearby(v, muts_to_n, allowed, ignore):
        """findNearbyInsertions (:288-337): [(node, (nuc list, block list))]."""
        found = []
        if v is None or allowed < 0:
            return found
        for key in muts_to_n:
            if key in t.insertions[v]:
                if t.insertions[v][key] < key[4]:
                    found.append((v, ([], [])))
                break
        for c in kids(v):
            if c != ignore:
                below = nearby(c, muts_to_n, int(np.float32(allowed) - bl(c)), v)
                if below:
                    add = invert(out.nuc_muts[c], out.block_muts[c], t.original[c], t.was_inv[c])
                    found += [(n, (l[0] + add[0], l[1] + add[1])) for n, l in below]
        if parent[v] != ignore:
            for n, l in nearby(parent[v], muts_to_n, int(np.float32(allowed) - bl(v)), v):
                found.append((n, (l[0] + out.nuc_muts[v], l[1] + out.block_muts[v])))
        return found

    lines, attempts, moves, pairs = [], 0, 0, 0
    for v in range(pm.num_nodes):
        with_n = [k for k, ns in t.insertions[v].items() if ns > 0]
        if not with_n:
            continue
        attempts += 1
        best_nuc, best_blk, best_parent, best_muts = -1, 0, None, None
        cands = nearby(parent[v], with_n, max_distance, v)
        pairs += len(cands)
        if trace is not None:
            trace[pm.names[v]] = [pm.names[n] for n, _ in cands]
        for n, l in cands:
            nuc = consolidate_nuc(l[0] + out.nuc_muts[v])
            impute_all_substitutions(nuc)
            blk = consolidate_blocks(l[1] + out.block_muts[v])
            nuc_imp = sum(length(m) for m in out.nuc_muts[v]) - sum(length(m) for m in nuc)
            blk_imp = len(out.block_muts[v]) - len(blk)
            if scores is not None:
                scores.setdefault(pm.names[v], []).append((nuc_imp, blk_imp))
            if nuc_imp > best_nuc and blk_imp >= best_blk:
                best_nuc, best_blk, best_parent, best_muts = nuc_imp, blk_imp, n, (nuc, blk)
        name = pm.names[v]
        if best_parent is None:
            lines.append(f"{name}\t{len(with_n)}\t{len(cands)}\t.\t-1\t0")
            continue
        moves += 1
        lines.append(f"{name}\t{len(with_n)}\t{len(cands)}\t{pm.names[best_parent]}\t{best_nuc}\t{best_blk}")
        lines += [f"{name}\tB\t{b}\t{int(ins)}\t{int(inv)}" for b, ins, inv in best_muts[1]]
        lines += [f"{name}\tN\t{p}\t{pos}\t{gap}\t{info}\t{nucs:06x}" for p, _, pos, gap, info, nucs in best_muts[0]]
    stats = {"imputed_bases": imputed, "insertion_nodes": attempts, "moves_found": moves, "pairs": pairs}
    return out, "".join(l + "\n" for l in lines), stats


def newick_of(pm: PanMAT) -> str:
    """Tree::getNewickString: lengths with "%f"; without lengths 1, the root 0."""
    off, idx = pm.child_offsets, pm.child_index

    def ln(v):
        if pm.branch_length is None:
            return ":%f" % (0.0 if v == pm.root else 1.0)
        return ":%f" % float(pm.branch_length[v])

    def rec(v):
        ks = [int(c) for c in idx[off[v]:off[v + 1]]]
        if not ks:
            return pm.names[v] + ln(v)
        return "(" + ",".join(rec(k) for k in ks) + ")" + pm.names[v] + ln(v)

    sys.setrecursionlimit(100000)
    return pm.names[pm.root] if off[pm.root] == off[pm.root + 1] else rec(pm.root) + ";"


def dump(pm: PanMAT) -> str:
    """tests/_panmat.py tree_dump of a list-built PanMAT, each node's block lines sorted."""
    from _subnet_ref import dump as subnet_dump
    return subnet_dump(pm, newick_of(pm))
