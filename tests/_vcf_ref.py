"""Plain-Python VCF extraction over aligned rows: the semantics of Tree::printVCFParallel
(src/vcf.cpp:177-382) that pm_vcf reproduces.  rows: {tip name: aligned row}."""
from __future__ import annotations

import re
import time


def scan(ref: str, tip: str) -> list[tuple[int, str, str]]:
    """(POS, REF, ALT) records of one tip against the reference row (equal lengths)."""
    assert len(ref) == len(tip)
    out = []
    R = A = ""
    ds = coord = 1
    for r, t in zip(ref, tip):
        if r == "-" and t == "-":
            continue
        if t == "-":
            if R == "" and A == "":
                ds = coord
            R += r
        elif r == "-":
            if R == "" and A == "":
                ds = coord
            A += t
        elif r != t:
            if R == A:
                R = A = ""
                ds = coord
            R += r
            A += t
        elif R == A:
            ds, R, A = coord, r, r          # the anchor
        elif R == "":
            out.append((coord, r, A + r))   # an insertion with nothing before it
            R = A = ""
        else:
            out.append((ds, R, A))
            ds, R, A = coord, r, r
        if r != "-":
            coord += 1
    if R != A:
        out.append((ds, R, A))
    return out


def records(rows: dict[str, str], reference: str):
    """({(POS, REF): {ALT: [tips]}}, skipped) over every tip but the reference."""
    ref = rows[reference]
    table: dict[tuple[int, bytes], dict[bytes, list[str]]] = {}
    skipped = 0
    for name, row in rows.items():
        if name == reference:
            continue
        if len(row) != len(ref):
            skipped += 1
            continue
        for pos, r, a in scan(ref, row):
            table.setdefault((pos, r.encode()), {}).setdefault(a.encode(), []).append(name)
    return table, skipped


def date_line() -> str:
    now = time.localtime()
    return f"##fileDate={now.tm_year}{now.tm_mon}{now.tm_mday}"


def vcf(rows: dict[str, str], reference: str) -> tuple[str, int]:
    """The VCF text and the number of skipped tips."""
    table, skipped = records(rows, reference)
    samples = sorted((n for n in rows if n != reference), key=lambda s: s.encode())
    out = ["##fileformat=VCFv4.2", date_line(), "##source=PanMATv2.0-beta", f"##reference={reference}",
           "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples)]
    for rid, (pos, r) in enumerate(sorted(table)):
        gt = dict.fromkeys(samples, 0)
        alts = sorted(table[(pos, r)])
        for k, a in enumerate(alts):
            for name in table[(pos, r)][a]:
                gt[name] = k + 1
        out.append("\t".join([reference, str(pos), str(rid), r.decode() or ".",
                              ",".join(a.decode() or "." for a in alts), ".", ".", ".", "."] +
                             [str(gt[s]) for s in samples]))
    return "\n".join(out) + "\n", skipped


def mask_date(text: str) -> str:
    return re.sub(r"^##fileDate=.*$", "##fileDate=", text, count=1, flags=re.M)
