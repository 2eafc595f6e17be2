#!/usr/bin/env python3
"""Fold the margins a GPU test run recorded (tests/margins.py: SSFM_MARGINS_FILE) into one row per kind of comparison.

    SSFM_MARGINS_FILE=raw.txt python -m pytest tests/test_signal_algebra_gpu.py -m gpu
    python tools/margins_digest.py raw.txt profiles/signal_ops_margins.txt

A kind is the record's `what` with the size (`n=...`), the tap count, the chunk size (`chunk=...`) and the fixture's case name taken out; its row carries the record with the
largest measured / bound of that kind, and how many records it stands for.  A third argument names a file whose text replaces the header's
description (it follows the record count; further lines start with `#`).

    python tools/margins_digest.py --table raw.txt profiles/fft_margins.txt tools/fft_margins_head.txt

`--table` (records whose `what` is "<section> <shape> <comparison>", tests/test_fft_edges_gpu.py): one line per shape instead of one per kind, the
comparisons side by side as columns of measured / bound, the columns named once per section."""
import collections
import re
import sys


def kind(what):
    what = re.sub(r"\b(n|taps|chunk|rows)=\d+ ", "", what)
    return re.sub(r"^(binary|reflected|scalar|pow|methods|filter|protocol)(_\w+)?/\S+", lambda m: m.group(1) + " fixtures", what)


HEAD = ("comparisons recorded by the GPU tests of the signal algebra on one MI355X, folded by tools/margins_digest.py: per kind of comparison,\n"
        "# the record with the largest measured / bound.  [ulp]: max |d| / (2^-52 |want|), of the modulus for complex values; [rad]: absolute;\n"
        "# [|d| / (...)]: elementwise against the stated product bound; otherwise max |d| / peak.  'numpy vs exact' rows are NumPy's own distance from\n"
        "# the exact restatement of unwrap (their bound column is what the device is then allowed).  Comparisons held to NumPy's bits record nothing.\n")


def main(src, dst, head=HEAD):
    rows, total = collections.OrderedDict(), 0
    for line in open(src):
        if line.startswith("#") or not line.strip():
            continue
        test, rest = line.rstrip("\n").split(" | ", 1)
        what, _steps, measured, bound, _ratio = rest.rsplit(" | ", 4)          # (`what` may hold a `|` of its own)
        m, b = float(measured), float(bound)
        r = m / b if b else 0.0
        total += 1
        k = kind(what.strip())
        count = rows[k][4] + 1 if k in rows else 1
        best = (m, b, r, test.split("::")[-1]) if k not in rows or r > rows[k][2] else rows[k][:4]
        rows[k] = (*best, count)
    with open(dst, "w") as f:
        f.write(f"# {total} " + head +
                "# kind | records | measured | bound | measured / bound | test of the worst record\n")
        for k, (m, b, r, t, count) in rows.items():
            f.write(f"{k} | {count} | {m:.3e} | {b:.3e} | {r:.3f} | {t}\n")
    print(total, "records,", len(rows), "kinds ->", dst)


# --table: what -> (section, shape, comparison)
TABLE = (r"^(A|B) (log2n=\d+ c\d+ E=\d+ Ef=\d+(?: \(default\))?) (.*)$", r"^(B split) (log2n=\d+ c\d+ R=\d+) (.*)$", r"^(C) (.*? log2n=\d+ c\d+) (.*)$",
         r"^(D) (len=\d+) (.*)$")


def table(src, dst, head=HEAD):
    sections, total = collections.OrderedDict(), 0          # section -> (columns, shape -> {column: worst ratio})
    for line in open(src):
        if line.startswith("#") or not line.strip():
            continue
        what, _steps, measured, bound, _ratio = line.rstrip("\n").split(" | ", 1)[1].rsplit(" | ", 4)
        m = next(filter(None, (re.match(rx, what.strip()) for rx in TABLE[1:] + TABLE[:1])))
        sec, shape, col = m.groups()
        cols, rows = sections.setdefault(sec, ([], collections.OrderedDict()))
        if col not in cols:
            cols.append(col)
        r = float(measured) / float(bound)
        row = rows.setdefault(shape, {})
        row[col] = max(row.get(col, 0.0), r)
        total += 1
    with open(dst, "w") as f:
        f.write(f"# {total} " + head)
        for sec, (cols, rows) in sections.items():
            f.write(f"# section {sec}: measured / bound, columns:\n" + "".join(f"#   {i + 1:2d} {c}\n" for i, c in enumerate(cols)))
            for shape, row in rows.items():
                f.write(f"{sec} {shape} | " + " ".join(f"{row[c]:.3g}" if c in row else "-" for c in cols) + "\n")
    print(total, "records ->", dst)


if __name__ == "__main__":
    if sys.argv[1] == "--table":
        table(sys.argv[2], sys.argv[3], *([open(sys.argv[4]).read()] if len(sys.argv) > 4 else []))
        sys.exit(0)
    main(sys.argv[1], sys.argv[2], *([open(sys.argv[3]).read()] if len(sys.argv) > 3 else []))
