"""Inputs and the check of the region extraction tests (tests/test_gpu_regions.py,
tests/test_regions_host.py, tests/test_regions_model.py): records as the dicts of
tests/regions_model.py, a small BAM writer (``struct`` + ``zlib``) that places BGZF block
boundaries at chosen byte offsets, writes stored blocks and can omit the EOF block, and the
comparison of a :class:`crispresso_amd.regions.RegionReads` with the model hit by hit.
"""
import struct
import zlib

import numpy as np

from tests import regions_model as rm

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
NIBBLES = "=ACMGRSVTWYHKDBN"


def rec(name, ref_id, pos, cigar, seq=None, qual=None, flag=0, mapq=30, noqual=False):
    """A record; seq / qual default to a pattern as long as the CIGAR's query bases."""
    if seq is None:
        n = sum(k for k, op in rm.parse_cigar(cigar) if op in "MIS=X")
        seq = "".join("ACGT"[(i * 7 + len(name) + i // 5) % 4] for i in range(n))
    if qual is None and seq != "*":
        qual = [(i * 11 + pos) % 42 for i in range(len(seq))]
    if noqual:
        qual = None
    return {"name": name if isinstance(name, bytes) else name.encode(), "flag": flag, "ref_id": ref_id, "pos": pos,
            "cigar": cigar, "seq": seq, "qual": qual, "mapq": mapq}


# ---- the BAM writer -------------------------------------------------------------------------

def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def record_bytes(r):
    ops = rm.parse_cigar(r["cigar"])
    seq = "" if r["seq"] == "*" else r["seq"]
    l_seq = len(seq)
    nib = [NIBBLES.index(c) for c in seq]
    if l_seq & 1:
        nib.append(0)
    packed = bytes(nib[i] * 16 + nib[i + 1] for i in range(0, len(nib), 2))
    qual = b"\xff" * l_seq if r["qual"] is None else bytes(r["qual"])
    assert len(qual) == l_seq
    span = sum(n for n, op in ops if op in "MDN=X")
    beg = r["pos"] - 1
    name = r["name"] + b"\0"
    body = struct.pack("<2i2B3H4i", r["ref_id"], beg, len(name), r.get("mapq", 30), reg2bin(beg, beg + max(span, 1)),
                       len(ops), r["flag"], l_seq, -1, -1, 0)
    body += name + b"".join(struct.pack("<I", n << 4 | rm.OPS.index(op)) for n, op in ops) + packed + qual
    return struct.pack("<i", len(body)) + body


def bam_plain(refs, records, text=b""):
    """The uncompressed BAM stream."""
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        out += [struct.pack("<i", len(name) + 1), name.encode() + b"\0", struct.pack("<i", length)]
    out += [record_bytes(r) for r in records]
    return b"".join(out)


def bgzf_block(data, stored=False):
    assert len(data) <= 65536
    co = zlib.compressobj(0 if stored else 6, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    bsize = 18 + len(comp) + 8
    assert bsize <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize - 1) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def bgzf(plain, cuts=None, stored=False, eof=True, block=0xFF00):
    """``plain`` as BGZF: block boundaries at the byte offsets ``cuts`` (and wherever a block
    would pass 64 KiB - 256), deflate level 0 when ``stored``, the EOF block when ``eof``."""
    edges = sorted({0, len(plain)} | {c for c in (cuts or ()) if 0 < c < len(plain)})
    out = []
    for a, b in zip(edges, edges[1:]):
        size = min(block, 60000) if stored else block      # (a stored block grows by 5 bytes per 64 KiB)
        for x in range(a, b, size):
            out.append(bgzf_block(plain[x:min(b, x + size)], stored))
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)


def sam_line(r, refs):
    seq = r["seq"] if r["seq"] not in ("", "*") else "*"
    qual = "*" if r["qual"] is None or seq == "*" else rm.qual_text(r["qual"])
    rname = refs[r["ref_id"]][0] if r["ref_id"] >= 0 else "*"
    return "\t".join(map(str, (r["name"].decode(), r["flag"], rname, r["pos"], r.get("mapq", 30), r["cigar"], "*", 0, 0,
                               seq, qual)))


# ---- the cases: (refs, records, regions) ----------------------------------------------------

REFS2 = [("chr1", 100000), ("chr2", 100000)]
CIGAR_A = "3S4M2I4M1D3M2H"          # at 100: [None x3, 100..103, None x2, 104..107, 109, 110, 111]


def all_pairs(ref_id, lo, hi):
    return [(ref_id, s, e) for s in range(lo, hi) for e in range(lo, hi)]


def cigar_edges():
    """Every (bpstart, bpend) around each CIGAR: first and last base of an M run, inside a D and
    an N gap, right after an I, behind leading S and H, P, = and X, 2,000 ops, no CIGAR."""
    records = [
        rec("a", 0, 100, CIGAR_A),
        rec("b", 0, 200, "2H3S5M100N5M"),
        rec("c", 0, 300, "4M2P4M"),
        rec("d", 0, 400, "5=3X2M"),
        rec("e", 0, 500, "15="),
        rec("f", 0, 600, "*", seq="ACGTA"),
        rec("g", 0, 1000, "1M1D" * 1000),
        rec("h", 0, 3000, "2S3M1I2=1X1D2M1N3M"),
    ]
    regions = all_pairs(0, 98, 114) + all_pairs(0, 198, 207) + [(0, s, e) for s in (200, 204, 205, 250, 304, 305)
                                                                 for e in (204, 205, 304, 305, 309, 310)]
    regions += all_pairs(0, 299, 309) + all_pairs(0, 399, 411) + [(0, 500, 514), (0, 500, 500), (0, 600, 600), (0, 600, 604)]
    regions += [(0, 1000, 2998), (0, 1000, 1000), (0, 1001, 1002), (0, 1500, 1600), (0, 1501, 1600), (0, 2998, 2998),
                (0, 2999, 2999), (0, 1000, 3000)]
    regions += all_pairs(0, 2999, 3012)
    return REFS2, records, regions


def slice_edges():
    """Python's slice rule: empty and reversed slices, all parities of (st, en), odd and even
    l_seq, 1-base reads, a 70,000-base read, en and st past l_seq, every nibble, phred 0 and 93."""
    records = [
        rec("even", 0, 10, "16M", seq=NIBBLES, qual=[0, 93] * 8),
        rec("odd", 0, 10, "15M", seq=NIBBLES[1:], qual=[93, 0] * 7 + [93]),
        rec("one", 0, 40, "1M", seq="G", qual=[93]),
        rec("long", 1, 1, "70000M", seq=("ACGTTGCAN" * 7778)[:70000], qual=[(i * 7) % 94 for i in range(70000)]),
        rec("short_seq", 0, 60, "20M", seq="ACGTACGTAC"),        # the CIGAR claims 20 bases, l_seq is 10
        rec("clipped", 0, 90, "5S10M", seq="ACGTACGTACGTACG"),
    ]
    regions = all_pairs(0, 9, 27)                                # every parity, empty, reversed, both records
    regions += [(0, 40, 40), (0, 39, 40), (0, 40, 41)]
    regions += [(1, 1, 70000), (1, 2, 69999), (1, 70000, 1), (1, 35001, 35002), (1, 1, 70001)]
    regions += [(0, 64, 77), (0, 69, 79), (0, 70, 79), (0, 75, 79), (0, 60, 69)]      # en / st cut to l_seq
    regions += [(0, 90, 99), (0, 91, 98)]
    return REFS2, records, regions


def record_filter():
    """Unmapped with a CIGAR, no reference, the same coordinates on another reference, records
    without sequence or qualities."""
    records = [
        rec("mapped", 0, 100, "20M"),
        rec("flag4", 0, 100, "20M", flag=4),
        rec("flag4_more", 0, 100, "20M", flag=4 | 1 | 64),
        rec("noref", -1, 100, "20M"),
        rec("other", 1, 100, "20M"),
        rec("noseq", 0, 100, "20M", seq="*"),
        rec("noqual", 0, 100, "20M", seq="ACGTACGTACGTACGTACGT", noqual=True),
        rec("noqual_miss", 0, 500, "20M", seq="ACGTACGTACGTACGTACGT", noqual=True),
        rec("reverse", 0, 100, "20M", flag=16),
        rec("mapped2", 0, 105, "20M"),
    ]
    regions = [(0, 105, 115), (1, 105, 115), (0, 100, 119), (-1, 105, 115), (5, 105, 115)]
    return REFS2, records, regions


def many_regions_one_record():
    records = [rec("r", 0, 1000, "100M"), rec("s", 0, 1010, "50M10D50M")]
    regions = [(0, 1000 + i, 1020 + i) for i in range(70)]
    return REFS2, records, regions


def many_records_one_region(n=3000):
    records = [rec("r%d" % i, 0, 500 + i % 37, "%dM" % (60 + i % 11)) for i in range(n)]
    regions = [(0, 540, 555), (0, 100, 200), (0, 540, 555), (1, 540, 555)]      # a hit, none, a duplicate, none
    return REFS2, records, regions


def random_case(n=500, n_regions=40, seed=1, n_ref=3, span=400):
    """Random CIGARs over n_ref references; the regions in no order, some twice."""
    rng = np.random.Generator(np.random.PCG64(seed))
    refs = [("ref%d" % k, span + 1000) for k in range(n_ref)]
    records = []
    for i in range(n):
        ops, last = [], ""
        for _ in range(int(rng.integers(1, 7))):
            op = "MMMMIDNS=XHP"[int(rng.integers(0, 12))]
            if op == last:
                continue
            ops.append("%d%s" % (int(rng.integers(1, 40)), op))
            last = op
        flag = 4 if rng.random() < 0.05 else (16 if rng.random() < 0.5 else 0)
        records.append(rec("q%d" % i, int(rng.integers(-1, n_ref)) if rng.random() < 0.1 else int(rng.integers(0, n_ref)),
                           int(rng.integers(1, span)), "".join(ops), flag=flag))
        if rng.random() < 0.03:
            records[-1]["qual"] = None
    regions = []
    for _ in range(n_regions):
        s = int(rng.integers(1, span))
        regions.append((int(rng.integers(0, n_ref)), s, s + int(rng.integers(-3, 30))))
    regions += regions[:3]
    return refs, records, regions


def table_past_lds(n_regions=5000):
    refs, records, _ = random_case(300, 1, seed=5, n_ref=2, span=2600)
    regions = [(k % 2, 1 + (k * 37) % 2500, 1 + (k * 37) % 2500 + 5 + k % 23) for k in range(n_regions)]
    return refs, records, regions


def demux_case():
    refs = [("amp%d" % k, 300) for k in range(12)]
    records = []
    for i in range(240):
        k = (i * 5) % 12
        if k == 7:
            k = -1 if i % 2 else 3           # reference 7 stays without reads
        records.append(rec("p%d" % i, k, 1 + i % 50, "%dM" % (30 + i % 9), flag=4 if i % 17 == 0 else 0))
    records[12]["seq"], records[12]["qual"] = "*", None
    records[13]["qual"] = None
    return refs, records


# ---- running and comparing ------------------------------------------------------------------

def got_hits(res):
    """A RegionReads in the model's form."""
    out = []
    for g in range(len(res)):
        a, b = int(res.region_offsets[g]), int(res.region_offsets[g + 1])
        (tb, off), (qb, qoff) = res.reads(g), res.quals(g)
        t, q, o = tb.tobytes(), qb.tobytes(), off.tolist()
        assert o == qoff.tolist() and len(o) == b - a + 1
        names = res.names(g)
        out.append([(int(res.src[a + k]), int(res.st[a + k]), int(res.en[a + k]), t[o[k]:o[k + 1]], q[o[k]:o[k + 1]],
                     names[k]) for k in range(b - a)])
    return {"hits": out, "n_no_seq": res.n_no_seq}


def mismatches(got, want, limit=8):
    """Lines that name the region and the hit that differ (empty when equal)."""
    bad = []
    if got["n_no_seq"] != want["n_no_seq"]:
        bad.append("n_no_seq: got %d, want %d" % (got["n_no_seq"], want["n_no_seq"]))
    if len(got["hits"]) != len(want["hits"]):
        return bad + ["%d regions, want %d" % (len(got["hits"]), len(want["hits"]))]
    for g, (a, b) in enumerate(zip(got["hits"], want["hits"])):
        if len(a) != len(b):
            bad.append("region %d: %d hits %s, want %d %s" % (g, len(a), [h[0] for h in a][:6], len(b), [h[0] for h in b][:6]))
        for k, (x, y) in enumerate(zip(a, b)):
            if x != y:
                f = [n for n, p, q in zip(("src", "st", "en", "text", "quals", "name"), x, y) if p != q]
                bad.append("region %d hit %d: %s differ: got %r, want %r" % (g, k, ",".join(f), tuple(v if not isinstance(v, bytes) else v[:40] for v in x), tuple(v if not isinstance(v, bytes) else v[:40] for v in y)))
        if len(bad) >= limit:
            break
    return bad
