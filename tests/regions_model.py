"""The semantics of crispresso_amd/regions.py in plain Python, twice:

* :func:`walk_ops` -- per-op arithmetic, which is what the kernel does;
* :func:`positions` with the interpreter's own ``in``, ``index`` and slices on a per-base list,
  which is what a user of the reference gets (CRISPRessoWGSCORE.py:166-221).

A record here is a dict: ``name`` (bytes), ``flag``, ``ref_id``, ``pos`` (1-based, as in SAM
text), ``cigar`` (SAM text, ``*`` = none), ``seq`` (str, ``*`` = none) and ``qual`` (a list of
phred values, or None = missing).  A region is ``(ref_id, bpstart, bpend)``.
"""
import re

OPS = "MIDNSHP=X"
_OP_RE = re.compile(r"(\d+)([MIDNSHP=X])")


def parse_cigar(cigar):
    if cigar == "*":
        return []
    ops = [(int(n), op) for n, op in _OP_RE.findall(cigar)]
    assert "".join("%d%s" % x for x in ops) == cigar, cigar
    return ops


def op_class(op, eqx):
    """'both', 'query', 'ref' or None: what the op advances."""
    if op == "M" or (eqx and op in "=X"):
        return "both"
    if op in "IS":
        return "query"
    if op in "DN":
        return "ref"
    return None


def walk_ops(pos, cigar, bpstart, bpend, eqx=False):
    """(hit, st, en) by arithmetic on the ops; st / en are None when the position is not mapped."""
    q, st, en = 0, None, None
    for n, op in parse_cigar(cigar):
        c = op_class(op, eqx)
        if c == "both":
            if pos <= bpstart < pos + n:
                st = q + bpstart - pos
            if pos <= bpend < pos + n:
                en = q + bpend - pos
            pos += n
            q += n
        elif c == "query":
            q += n
        elif c == "ref":
            pos += n
    return st is not None and en is not None, st, en


def positions(pos, cigar, eqx=False):
    """One entry per query base: its reference position or None."""
    out = []
    for n, op in parse_cigar(cigar):
        c = op_class(op, eqx)
        if c == "both":
            out.extend(range(pos, pos + n))
            pos += n
        elif c == "query":
            out.extend([None] * n)
        elif c == "ref":
            pos += n
    return out


def walk_list(pos, cigar, bpstart, bpend, eqx=False):
    """(hit, st, en) with the interpreter's ``in`` and ``index`` on the per-base list."""
    p = positions(pos, cigar, eqx)
    if bpstart in p and bpend in p:
        return True, p.index(bpstart), len(p) - p[::-1].index(bpend) - 1
    return False, (p.index(bpstart) if bpstart in p else None), (p.index(bpend) if bpend in p else None)


def qual_text(qual):
    return "".join(chr(q + 33) for q in qual)


def has_seq(rec):
    return rec["seq"] != "*" and len(rec["seq"]) > 0 and rec["qual"] is not None


def extract(records, regions, eqx=False, walk=walk_ops):
    """{'hits': per region a list of (src, st, en, seq, qual, name), 'n_no_seq': int}."""
    hits = [[] for _ in regions]
    dropped = 0
    on_ref = {}
    for i, r in enumerate(records):
        if not (r["flag"] & 4 or r["ref_id"] < 0):
            on_ref.setdefault(r["ref_id"], []).append((i, r))
    for g, (ref_id, bpstart, bpend) in enumerate(regions):
        for i, r in on_ref.get(ref_id, ()):
            hit, st, en = walk(r["pos"], r["cigar"], bpstart, bpend, eqx)
            if not hit:
                continue
            if not has_seq(r):
                dropped += 1
                continue
            k = len(hits[g]) + 1
            hits[g].append((i, st, en, r["seq"][st:en].encode(), qual_text(r["qual"])[st:en].encode(),
                            r["name"] + b"_%d" % k))
    return {"hits": hits, "n_no_seq": dropped}


def demux(records, n_ref):
    hits = [[] for _ in range(n_ref)]
    dropped = 0
    for i, r in enumerate(records):
        if r["flag"] & 4 or r["ref_id"] < 0:
            continue
        if not has_seq(r):
            dropped += 1
            continue
        hits[r["ref_id"]].append((i, 0, len(r["seq"]), r["seq"].encode(), qual_text(r["qual"]).encode(), r["name"]))
    return {"hits": hits, "n_no_seq": dropped}


def fastq(hits):
    return b"".join(b"@%s\n%s\n+\n%s\n" % (h[5], h[3], h[4]) for h in hits)
