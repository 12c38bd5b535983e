"""A plain-Python restatement of panmanToUsher (src/panman2usher.cpp:564-604; the walk getNodeDFS,
:282-562; the --toUsher command, src/panmanUtils.cpp:1205-1240), working from a list-built PanMAT alone.

The reference is undefined as written: it indexes globalCoords_t and pseudoRoot while both are empty
vectors (:565-569).  This restates what its code does with both sized to the largest block id + 1.

The walk is the reference's: depth first with one dictionary of running characters keyed by cell
(block, position, slot), a node's changes undone after its subtree.  There are no rows and no replay
here, so nothing is shared with the product's method.  Block mutations are never read (:294-333 only
track them).  The bytes are proto3 as the Protobuf C++ library writes Parsimony::data (usher.proto):
fields in number order, zero scalars left out, repeated int32 packed.

The deviations pm_to_usher documents: a secondary block and a mutation on an id that holds no block
raise Unsupported; a mutation element (types 0 to 5) whose cell does not exist raises ArgError, where
the reference indexes out of bounds."""
from __future__ import annotations

from _protobuf import f_bytes, f_varint, varint

NUC = "-ACMGRSVTWYHKDBN"        # getNucleotideFromCode (src/panman.cpp:41-76): anything else, 0 included, is '-'
CODE = {c: i for i, c in enumerate(NUC) if i}   # getCodeFromNucleotide (:78-113): anything else, '-' and 'x' included, is 0


class ArgError(ValueError):
    """PM_ERR_ARG: a mutation whose cell does not exist."""


class Unsupported(ValueError):
    """PM_ERR_UNSUPPORTED: secondary blocks; a mutation on an id that holds no block."""


def _lists(pm):
    if getattr(pm, "_arrays", None) is not None:
        from _maf_ref import _Lists
        return _Lists(pm)
    return pm


def pseudo_root(pm):
    """getPseudoRoot (:53-90) and getCoordMap (:3-51): ({cell: character}, {cell: position}); the
    cells of a block are, per position, its gap slots ascending and then its main character, blocks
    in ascending id."""
    cells = {}          # block -> [[main, slots]]
    for b, words in pm.blocks:
        seq = cells.setdefault(b, [])
        end = False
        for w in words:
            for k in range(8):
                code = (w >> (4 * (7 - k))) & 15
                if code == 0:
                    end = True
                    break
                seq.append([NUC[code], 0])
            if end:
                break
        seq.append(["x", 0])
    for b, slots in pm.gaps:
        for pos, length in slots:
            cells[b][pos][1] = length            # resize: the last length given wins
    char, position = {}, {}
    index = 1
    for b in sorted(cells):
        for j, (main, slots) in enumerate(cells[b]):
            for k in range(slots):
                char[b, j, k] = "-"
                position[b, j, k] = index
                index += 1
            char[b, j, -1] = main
            position[b, j, -1] = index
            index += 1
    return char, position


def mut_nuc(code: int):
    """get_nuc_vec_from_id (:278-280): the set bits of the code, 0 as 15 (get_nuc(0) is 'N')."""
    code = code or 15
    return [k for k in range(4) if code >> k & 1]


def node_lists(pm):
    """Per node in depth-first pre-order (children in stored order): [(position, ref, par, [mut_nuc])]."""
    pm = _lists(pm)
    if any(secondary != -1 for muts in pm.nuc_muts for _, secondary, *_ in muts):
        raise Unsupported("secondary blocks")
    root_char, position = pseudo_root(pm)
    is_block = {b for b, _ in pm.blocks}
    for muts in pm.nuc_muts:                     # refusals come before any output
        for b, _, pos, g, info, _ in muts:
            typ, length = info & 7, info >> 4
            if typ > 5:
                continue
            if b not in is_block:
                raise Unsupported("mutation on a missing block")
            for j in range(1 if typ >= 3 else length):
                cell = (b, pos, g + j) if g != -1 else (b, pos + j, -1)
                if g < -1 or cell not in position:
                    raise ArgError("mutation outside its block")
    sequence = dict(root_char)
    out = []

    def visit(v):
        mine, undo = [], []
        for b, _, pos, g, info, nucs in pm.nuc_muts[v]:
            typ, length = info & 7, info >> 4
            if typ > 5:
                continue
            for j in range(1 if typ >= 3 else length):
                cell = (b, pos, g + j) if g != -1 else (b, pos + j, -1)
                old = sequence[cell]
                if typ in (1, 5):                # newVal stays '-' (:344): the code of '-' is 0, so N's bits
                    new, bits = "-", mut_nuc(0)
                else:
                    new = NUC[(nucs >> (4 * (5 - j))) & 15]
                    bits = mut_nuc(CODE.get(new, 0))
                sequence[cell] = new
                undo.append((cell, old))
                mine.append((position[cell], CODE.get(root_char[cell], 0), CODE.get(old, 0), bits))
        out.append(mine)
        return undo

    stack = [(pm.root, None)]                    # (node, None) to enter, (None, undo list) to leave
    while stack:
        v, undo = stack.pop()
        if v is None:
            for cell, old in reversed(undo):
                sequence[cell] = old
            continue
        stack.append((None, visit(v)))
        for e in range(int(pm.child_offsets[v + 1]) - 1, int(pm.child_offsets[v]) - 1, -1):
            stack.append((int(pm.child_index[e]), None))
    return out


def newick(pm) -> str:
    """Tree::getNewickString (src/panman.cpp:1921-2029) as the PanMAN writer prints it: leaves
    "name:len", clades "(...)name:len", lengths with "%f" (1 for every node and 0 for the root when the
    PanMAT has none), ';' at the end; a single node is its bare identifier."""
    off, idx = pm.child_offsets, pm.child_index
    if off[pm.root] == off[pm.root + 1]:
        return pm.names[pm.root]
    lengths = getattr(pm, "branch_length", None)

    def label(v):
        length = (0.0 if v == pm.root else 1.0) if lengths is None else float(lengths[v])
        return pm.names[v] + (":%f" % length if length >= 0 else "")

    text, stack = [], [(pm.root, 0)]
    while stack:
        v, k = stack.pop()
        kids = [int(idx[e]) for e in range(off[v], off[v + 1])]
        if not kids:
            text.append(label(v))
        elif k == len(kids):
            text.append(")" + label(v))
        else:
            text.append("(" if k == 0 else ",")
            stack.append((v, k + 1))
            stack.append((kids[k], 0))
    return "".join(text) + ";"


def encode_mut(position, ref, par, bits) -> bytes:
    body = f_varint(1, position)
    if ref:
        body += f_varint(2, ref)
    if par:
        body += f_varint(3, par)
    return body + f_bytes(4, bytes(bits))        # (bits is never empty: a packed field of one byte each)


def encode(newick_text: str, lists) -> bytes:
    out = [f_bytes(1, newick_text.encode())]
    for muts in lists:
        out.append(f_bytes(2, b"".join(f_bytes(1, encode_mut(*m)) for m in muts)))
    return b"".join(out)


def to_usher(pm):
    """(bytes, mutation records)."""
    lists = node_lists(pm)
    return encode(newick(pm), lists), sum(len(m) for m in lists)


# ---- a small decoder, for readable failures -------------------------------------------------------------

def _read_varint(b, at):
    v = shift = 0
    while True:
        v |= (b[at] & 0x7F) << shift
        shift += 7
        at += 1
        if not b[at - 1] & 0x80:
            return v, at


def _fields(b):
    at = 0
    while at < len(b):
        k, at = _read_varint(b, at)
        if k & 7 == 0:
            v, at = _read_varint(b, at)
        elif k & 7 == 2:
            n, at = _read_varint(b, at)
            assert at + n <= len(b), "a field runs past its message"
            v, at = b[at:at + n], at + n
        else:
            raise ValueError(f"wire type {k & 7}")
        yield k >> 3, v


def decode(b: bytes):
    """(newick, [[(position, ref, par, [mut_nuc])]])."""
    text, nodes = None, []
    for f, v in _fields(b):
        if f == 1:
            text = v.decode()
        elif f == 2:
            muts = []
            for g, m in _fields(v):
                assert g == 1
                rec = {1: 0, 2: 0, 3: 0, 4: b""}
                for h, x in _fields(m):
                    rec[h] = x
                muts.append((rec[1], rec[2], rec[3], list(rec[4])))
            nodes.append(muts)
        else:
            raise ValueError(f"field {f}")
    return text, nodes


def first_difference(got: bytes, want: bytes) -> str:
    """Where two messages part, by node and record."""
    if got == want:
        return "equal"
    try:
        gt, gn = decode(got)
    except Exception as e:   # noqa: BLE001 -- whatever the bytes hold, the failure must still be named
        at = next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), min(len(got), len(want)))
        return f"the bytes do not decode ({e!r}); first differing byte {at} of {len(got)} against {len(want)}"
    wt, wn = decode(want)
    if gt != wt:
        return f"newick: got {gt[:80]!r}, want {wt[:80]!r}"
    for v in range(max(len(gn), len(wn))):
        a, b = (gn[v] if v < len(gn) else None), (wn[v] if v < len(wn) else None)
        if a == b:
            continue
        if a is None or b is None:
            return f"{len(gn)} nodes against {len(wn)}"
        for k in range(max(len(a), len(b))):
            x, y = (a[k] if k < len(a) else None), (b[k] if k < len(b) else None)
            if x != y:
                return f"node {v} (pre-order), record {k}: got {x}, want {y} ({len(a)} records against {len(b)})"
    return "the same records in other bytes (an encoding difference)"
