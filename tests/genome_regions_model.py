"""The semantics of crispresso_amd.regions.discover_regions in plain Python, twice:

* :func:`span_ops` -- per-op arithmetic with the run rule for ``=`` and ``X``, which is what the
  kernel does;
* :func:`span_text` -- on the CIGAR **text**, the way the reference's ``awk`` goes about it
  (CRISPRessoPooledCORE.py:1048-1059): split on the delimiter set, the leading number of a
  token, the character at the running offset.  The quirk of the default setting falls out of it
  without a special case.

and the order inside a region's file that the reference's ``sort`` leaves (:func:`line_key`):
its last-resort comparison of whole lines, bytewise under the C locale.

A record is the dict of tests/regions_model.py: ``name`` (bytes), ``flag``, ``ref_id``, ``pos``
(1-based), ``cigar`` (SAM text, ``*`` = none), ``seq`` (``*`` = none), ``qual`` (phred values or
None).
"""
import re

from tests import regions_model as rm

DELIMITERS = "MIDNSHP"


def span_ops(pos, cigar, eqx=False):
    """(bpstart, bpend) by arithmetic on the ops."""
    bpstart = bpend = pos

    def step(kind, n):
        nonlocal bpstart, bpend
        if kind == "S":
            if bpend == pos:
                bpstart -= n
            else:
                bpend += n
        elif kind not in "IH":
            bpend += n

    run = None          # the length that a run of ops the reference does not split on carries
    for n, op in rm.parse_cigar(cigar):
        if op in "=X":
            if eqx:
                op = "M"
            else:
                if run is None:
                    run = n
                continue
        if run is not None:
            n, run = run, None
        step(op, n)
    if run is not None:
        step("M", run)
    return bpstart, bpend


def leading_number(token):
    """What awk makes of a string used as a number (no sign, point or exponent occurs here)."""
    m = re.match(r"\d+", token)
    return int(m.group()) if m else 0


def span_text(pos, cigar):
    """(bpstart, bpend) the way the reference's awk computes them from the CIGAR text."""
    bpstart = bpend = pos
    n = 0
    for token in re.split("[%s]" % DELIMITERS, cigar):
        n += 1 + len(token)
        c = cigar[n - 1:n]                  # substr($6, n, 1): empty past the end
        if c == "S":
            if bpend == pos:
                bpstart -= leading_number(token)
            else:
                bpend += leading_number(token)
        elif c != "I" and c != "H":
            bpend += leading_number(token)
    return bpstart, bpend


def span_text_eqx(pos, cigar):
    """eqx_as_match on the text: = and X read as M."""
    return span_text(pos, cigar.replace("=", "M").replace("X", "M"))


def strand(flag):
    return b"-" if flag % 32 >= 16 else b"+"


def takes_part(r):
    return not (r["flag"] & 4) and r["ref_id"] >= 0


def discover(records, eqx=False, min_reads=0, span=None):
    """{'regions': [(ref_id, bpstart, bpend)] ascending, 'n_records': [...], 'hits': per region a
    list of (src, st, en, seq, qual, name) in record order ([] below min_reads), 'strand': per
    region a list of b'+' / b'-', 'n_no_seq', 'n_aligned', 'n_kept'}."""
    span = span or (lambda pos, cigar: span_ops(pos, cigar, eqx))
    by_key, dropped, aligned = {}, 0, 0
    for i, r in enumerate(records):
        aligned += (r["flag"] & 0x904) == 0
        if not takes_part(r):
            continue
        if not rm.has_seq(r):
            dropped += 1
            continue
        by_key.setdefault((r["ref_id"],) + tuple(span(r["pos"], r["cigar"])), []).append(i)
    regions = sorted(by_key)
    hits, strands = [], []
    for key in regions:
        src = by_key[key] if len(by_key[key]) >= min_reads else []
        hits.append([(i, 0, len(records[i]["seq"]), records[i]["seq"].encode(), rm.qual_text(records[i]["qual"]).encode(),
                      records[i]["name"]) for i in src])
        strands.append([strand(records[i]["flag"]) for i in src])
    return {"regions": regions, "n_records": [len(by_key[k]) for k in regions], "hits": hits, "strand": strands,
            "n_no_seq": dropped, "n_aligned": aligned, "n_kept": sum(map(len, by_key.values()))}


def line_key(strand_byte, hit):
    """What is left of the reference's intermediate line once chr_id, bpstart and bpend are equal:
    ``sort`` compares it bytewise under LC_ALL=C, tabs included."""
    return b"\t".join((strand_byte, hit[5], hit[3], hit[4]))


def reference_order(hits, strands):
    keys = [line_key(s, h) for s, h in zip(strands, hits)]
    return sorted(range(len(hits)), key=keys.__getitem__)


def fastq_reference_order(hits, strands):
    return b"".join(b"@%s\n%s\n+\n%s\n" % (hits[k][5], hits[k][3], hits[k][4]) for k in reference_order(hits, strands))


def region_name(ref_name, key):
    return "REGION_%s_%d_%d" % (ref_name, key[1], key[2])


def parse_sam(lines):
    """(refs, records) of SAM lines without header: the references in order of first appearance
    (length 0), ``*`` as reference -1."""
    refs, index, records = [], {}, []
    for line in lines:
        f = line.rstrip("\n").split("\t")
        if f[2] == "*":
            ref_id = -1
        else:
            if f[2] not in index:
                index[f[2]] = len(refs)
                refs.append((f[2], 0))
            ref_id = index[f[2]]
        qual = None if f[10] == "*" else [ord(c) - 33 for c in f[10]]
        records.append({"name": f[0].encode(), "flag": int(f[1]), "ref_id": ref_id, "pos": int(f[3]), "mapq": int(f[4]),
                        "cigar": f[5], "seq": f[9], "qual": qual})
    return refs, records
