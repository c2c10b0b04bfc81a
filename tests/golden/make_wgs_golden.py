"""Writes tests/golden/wgs_positions.json.gz: rows (pos, cigar, bpstart, bpend) -> (hit, st, en)
recorded from the reference's own functions.

    python tests/golden/make_wgs_golden.py <path to CRISPResso/CRISPRessoWGSCORE.py>

The two function definitions the reference's write_trimmed_fastq uses (get_reference_positions,
find_last) are taken out of that file as text and executed here, at generation time only; none
of the reference's text is kept.  The test that reads the file is tests/test_regions_model.py.
"""
import gzip
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

CIGARS = [
    (100, "3S4M2I4M1D3M2H"), (100, "5=3X2M"), (100, "15="), (100, "10=5M"), (200, "2H3S5M100N5M"), (300, "4M2P4M"),
    (400, "*"), (500, "20M"), (500, "1M1D1M1D1M1D1M"), (600, "2S3M1I2=1X1D2M1N3M"), (700, "3I4M"), (800, "4M3S"),
    (900, "12X3M2=4M"), (1000, "1M"),
]


def definition(text, name):
    """The source of the top-level function `name`."""
    lines = text.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("def %s(" % name))
    end = start + 1
    while end < len(lines) and (not lines[end].strip() or lines[end][0] in " \t"):
        end += 1
    return "\n".join(lines[start:end]) + "\n"


def main(path):
    text = open(path).read()
    ns = {"re": re}
    for name in ("find_last", "get_reference_positions"):
        exec(definition(text, name), ns)
    rows = []
    for pos, cigar in CIGARS:
        p = ns["get_reference_positions"](pos, cigar)
        span = [x for x in p if x is not None]
        lo, hi = (min(span) - 2, max(span) + 3) if span else (pos - 1, pos + 2)
        cand = sorted(set(range(lo, min(hi, lo + 9))) | set(range(max(lo, hi - 6), hi)))
        k = 0
        for s in cand:
            for e in cand:
                k += 1
                if k % 7 and not (s in p and e in p and k % 2):
                    continue
                hit = s in p and e in p
                rows.append([pos, cigar, s, e, bool(hit), p.index(s) if hit else None,
                             ns["find_last"](p, e) if hit else None])
    out = os.path.join(HERE, "wgs_positions.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as f:
        f.write(json.dumps({"rows": rows}).encode())
    print("%d rows (%d hits) -> %s" % (len(rows), sum(r[4] for r in rows), out))


if __name__ == "__main__":
    main(sys.argv[1])
