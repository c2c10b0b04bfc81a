"""Inputs and the check of the demultiplexing tests (tests/test_demux_model.py,
tests/test_gpu_demux.py): amplicons and reads as lists of ``bytes`` with fixed seeds, and the
comparison of a :class:`crispresso_amd.demux.DemuxResult` with tests/demux_model.py read by read
and byte by byte.

Run as ``python -m tests.demux_cases <mode>`` it is the child process of the tests whose setting
is read when the context is created (CRISPR_NWD_TALLY_SLOTS, CRISPR_NWD_CHUNK): one JSON line
with what the run found.
"""
import functools
import hashlib
import json
import sys

import numpy as np

from crispresso_amd import synth
from tests import demux_model as dm
from tests.alleles_cases import pack

BASES = np.frombuffer(b"ACGT", np.uint8)


def bases(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return BASES[rng.integers(0, 4, n)].tobytes()


def substitute(seq, pos, to=None):
    """seq with the base at pos replaced (by the next of ACGT, or by ``to``)."""
    new = to if to is not None else b"ACGT"[(b"ACGT".index(seq[pos:pos + 1].upper()) + 1) % 4:][:1]
    return seq[:pos] + new + seq[pos + 1:]


def both(reads):
    """Each read once as given and once reverse-complemented."""
    return [x for r in reads for x in (r, dm.revcomp(r))]


def window_edges(k):
    """Reads of k - 1, k, k + 1 and 4096 bases and the empty read, from a long and a short
    amplicon, in both orientations."""
    amps = [bases(4200, 11), bases(200, 12), bases(180, 13)]
    reads = [b""]
    for n in (k - 1, k, k + 1):
        reads += [amps[0][100:100 + n], amps[1][7:7 + n], amps[2][180 - n:]]
    reads += [amps[0][:4096], amps[0][104:4200], substitute(amps[0][50:4146], 2000)]
    reads = both(reads) + [b"", b""]
    return amps, reads


def lane_stretches(k):
    """63..66 + k and 127..130 + k bases: 64..67 and 128..131 windows, so a lane's stretch of
    one, two or three windows ends inside the read; with a substitution that moves from read to
    read, so that every window's vote counts."""
    amp = [bases(400, 21), bases(400, 22)]
    reads = []
    for i, n in enumerate([63 + k, 64 + k, 65 + k, 66 + k, 127 + k, 128 + k, 129 + k, 130 + k]):
        for j, start in enumerate((0, 3, 400 - n)):
            r = amp[(i + j) % 2][start:start + n]
            reads += [r, substitute(r, (7 * i + 31 * j + k) % n), substitute(r, n - 1 - (5 * i + j) % k)]
    return amp, both(reads)


def breaks(k):
    """An N or a '-' at positions 0, k - 1, k, n - k and n - 1 of a read, an N inside an
    amplicon, lower-case reads and amplicons."""
    a0 = bases(150, 31)
    a1 = bases(150, 32)
    a1 = a1[:70] + b"N" + a1[71:]
    a2 = bases(150, 33).lower()
    amps = [a0, a1, a2]
    reads = []
    n = 90
    for amp in (a0, a1, a2):
        r = amp[30:30 + n]
        reads += [r, r.lower(), r.upper(), r.swapcase()]
        for pos in (0, k - 1, k, n - k, n - 1):
            reads += [substitute(r, pos, b"N"), substitute(r, pos, b"-"), substitute(r, pos, b"n")]
        reads.append(substitute(substitute(r, k, b"N"), n - k, b"-"))
    reads += [b"N" * 40, b"-" * k, a1[60:82], a1[71 - k:71 + k]]
    return amps, both(reads)


def palindrome():
    """An amplicon equal to its own reverse complement: its reads vote alike on both strands."""
    half = bases(60, 41)
    pal = half + dm.revcomp(half)
    other = bases(120, 42)
    return [pal, other], [pal, pal[10:100], other, dm.revcomp(other), pal[:50], half]


def ambiguity():
    """{name: (amplicons, reads)} of the four constructions."""
    a, b, c = bases(250, 51), bases(250, 52), bases(250, 53)
    near = substitute(substitute(substitute(a, 40), 120), 200)
    bridge = b[125:] + c[:125]
    out = {}
    out["three_bases"] = ([a, near, b], both([a, near, a[:100], near[:100], a[30:60], a[60:110], near[100:140], b]))
    out["bridge"] = ([b, c, bridge], both([b, c, bridge, b[:125], b[125:], c[:125], c[125:], b[100:150], c[100:150],
                                           bridge[100:150], bridge[117:133]]))
    out["identical"] = ([a, bytes(a), b], both([a, a[:80], b]))
    out["reverse_complement"] = ([a, dm.revcomp(a), b], both([a, a[20:90], b]))
    return out


def min_hits_reads(k, min_hits):
    """Reads with exactly min_hits - 1, min_hits and min_hits + 1 clean windows of the amplicon:
    that many + k - 1 of its bases between breaks and bases of no amplicon."""
    amp = bases(200, 61)
    junk = bases(60, 62)
    reads = []
    for m in (min_hits - 1, min_hits, min_hits + 1):
        core = amp[50:50 + k - 1 + m] if m > 0 else amp[50:50 + k - 1]
        reads += [core, b"N" + core + b"N", junk[:30] + b"N" + core + b"-" + junk[30:], core.lower()]
    return [amp, bases(200, 63)], both(reads)


def stitched(n_reads=40):
    """Reads stitched from 40-base pieces of 5 amplicons in turn (5 candidates and more): a tally
    of 2 slots overflows on every one of them."""
    amps = [bases(220, 70 + g) for g in range(6)]
    reads = []
    for i in range(n_reads):
        parts = [amps[(i + j) % 6][(7 * i + 13 * j) % 150:][:40 + (8 if j == i % 5 else 0)] for j in range(5)]
        if i % 3 == 1:
            parts[2] = dm.revcomp(parts[2])
        r = b"".join(parts)
        reads.append(dm.revcomp(r) if i % 2 else r)
    reads += [amps[0][:100], amps[3][50:150], b"", amps[5][:20]]       # and reads that fit any tally
    return amps, reads


def chunk_reads():
    """200 reads over 5 amplicons, with ties, misses and empty reads among them."""
    amps = [bases(180 + 10 * g, 80 + g) for g in range(5)]
    rng = np.random.Generator(np.random.PCG64(85))
    reads = []
    for i in range(200):
        g = int(rng.integers(0, 5))
        lo = int(rng.integers(0, 60))
        r = amps[g][lo:lo + int(rng.integers(10, 120))]
        if i % 7 == 3:
            r = substitute(r, len(r) // 2)
        if i % 11 == 5:
            r = r[:40] + amps[(g + 1) % 5][:40]
        if i % 13 == 6:
            r = b""
        if i % 17 == 8:
            r = bases(50, 900 + i)
        reads.append(dm.revcomp(r) if i % 2 else r)
    return amps, reads


def pooled_panel():
    """8 amplicons x 50 reads (the C2 edit mix), every odd read reverse-complemented, the
    amplicons' reads interleaved."""
    amps = synth.pooled_amplicons(8, seed=9)
    per = [synth.unpack(*synth.reads_from(a, 50, seed=300 + g)) for g, a in enumerate(amps)]
    reads = [per[g][i].encode() for i in range(50) for g in range(8)]
    reads = [dm.revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
    return amps, reads


@functools.lru_cache(maxsize=None)
def acceptance():
    """(amplicons, reads) of the oracle comparison: 8 pooled amplicons, a copy of amplicon 0 with
    bases 40, 120 and 200 substituted, amp1[125:] + amp2[:125]; 25 reads each, every odd read
    reverse-complemented."""
    amps = [a.encode() for a in synth.pooled_amplicons(8, seed=5)]
    assert len(amps[0]) > 200
    amps.append(substitute(substitute(substitute(amps[0], 40), 120), 200))
    amps.append(amps[1][125:] + amps[2][:125])
    reads = []
    for g, amp in enumerate(amps):
        reads += [r.encode() for r in synth.unpack(*synth.reads_from(amp.decode(), 25, seed=100 + g))]
    reads = [dm.revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
    assert len(amps) == 10 and len(reads) == 250
    return amps, reads


@functools.lru_cache(maxsize=None)
def acceptance_scores():
    """int array [read, amplicon, strand]: the needle oracle's score of every read, as given
    (strand 0) and reverse-complemented (strand 1), against every amplicon.  Computed once."""
    from oracle import oracle_py

    amps, reads = acceptance()
    buf, off = pack(reads + [dm.revcomp(r) for r in reads])
    n = len(reads)
    out = np.zeros((n, len(amps), 2), np.int64)
    for g, amp in enumerate(amps):
        res, _ = oracle_py.align_batch(amp.decode(), buf, off, nthreads=4)
        out[:, g, 0] = res["score"][:n]
        out[:, g, 1] = res["score"][n:]
    out.setflags(write=False)
    return out


def oracle_disagreements(which, strand):
    """The assigned reads whose (which, strand) is not among the pairs the oracle scores highest."""
    scores = acceptance_scores()
    bad = []
    for r, (g, s) in enumerate(zip(which, strand)):
        if g >= 0 and scores[r, g, s] != scores[r].max():
            bad.append((r, int(g), int(s), int(scores[r, g, s]), int(scores[r].max())))
    return bad


@functools.lru_cache(maxsize=None)
def unrelated(per=300):
    """(amplicons, reads, source): pooled_amplicons(12), `per` reads each, odd reads
    reverse-complemented."""
    amps = [a.encode() for a in synth.pooled_amplicons(12)]
    reads, source = [], []
    for g, amp in enumerate(amps):
        reads += [r.encode() for r in synth.unpack(*synth.reads_from(amp.decode(), per, seed=200 + g))]
        source += [g] * per
    reads = [dm.revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
    return amps, reads, source


def mismatches(got, want, limit=5):
    """What differs between a DemuxResult and the model's dict, naming the reads."""
    bad = []
    for name in ("which", "strand", "votes", "rival", "counts", "group_offsets", "order"):
        ours = np.asarray(getattr(got, name)).tolist()
        if ours != want[name]:
            diff = [i for i, (x, y) in enumerate(zip(ours, want[name])) if x != y][:limit]
            bad.append(f"{name}: {len(ours)} vs {len(want[name])}; first differences at "
                       + ", ".join(f"{i}: {ours[i]} != {want[name][i]}" for i in diff))
    for name in ("n_windows", "n_ambiguous"):
        if int(getattr(got, name)) != want[name]:
            bad.append(f"{name}: {getattr(got, name)} != {want[name]}")
    if not bad:
        raw = got.text.tobytes()
        to = got.text_offsets.tolist()
        flat = [r for grp in want["groups"] for r in grp]
        ours = [raw[to[j]:to[j + 1]] for j in range(len(to) - 1)]
        if ours != flat:
            diff = [j for j, (x, y) in enumerate(zip(ours, flat)) if x != y][:limit]
            bad.append(f"gathered bytes: {len(ours)} vs {len(flat)} reads; first differences at gathered reads {diff}")
        per = got.reads_per_amplicon()
        for g, (buf, off) in enumerate(per):
            mine = [buf.tobytes()[off[i]:off[i + 1]] for i in range(len(off) - 1)]
            if mine != want["groups"][g]:
                bad.append(f"reads_per_amplicon: group {g} differs")
    return bad


def digest(got):
    """One hash over every returned array (byte-equality of two runs)."""
    h = hashlib.sha256()
    for part in (got.which, got.strand, got.votes, got.rival, got.counts, got.group_offsets, got.order, got.text,
                 got.text_offsets, np.asarray([got.n_windows, got.n_ambiguous, got.n_tie, got.n_no_hit], np.int64)):
        h.update(np.ascontiguousarray(part).tobytes())
        h.update(b"|")
    return h.hexdigest()


def run(d, amps, reads, lead=0, **kw):
    from crispresso_amd import demux

    return demux.demultiplex(list(amps), pack(reads, lead), demultiplexer=d, **kw)


def check(d, amps, reads, lead=0, want=None, **kw):
    """Runs the GPU path and the model; returns (result, model's dict), asserting they agree."""
    want = want or dm.demultiplex(amps, reads, **kw)
    got = run(d, amps, reads, lead, **kw)
    bad = mismatches(got, want)
    assert not bad, "\n".join(bad)
    assert got.which.dtype == np.int32 and got.strand.dtype == np.uint8 and got.counts.dtype == np.int64
    assert got.n_assigned + got.n_tie + got.n_no_hit == len(reads)
    return got, want


def child(mode):
    from crispresso_amd import demux

    out = {"ok": True, "bad": [], "fallback": [], "digest": []}
    with demux.GpuDemultiplexer(0) as d:
        def one(amps, reads, **kw):
            got = run(d, amps, reads, **kw)
            bad = mismatches(got, dm.demultiplex(amps, reads, **kw))
            out["ok"] = out["ok"] and not bad
            out["bad"] += bad
            out["fallback"].append(got.fallback)
            out["digest"].append(digest(got))

        if mode == "stitched":
            one(*stitched())
            one(*stitched(), k=8, min_hits=1)
            one(*stitched(), both_strands=False)
        elif mode == "chunks":
            one(*chunk_reads())
            one(*chunk_reads(), k=8)
            one(chunk_reads()[0], [])
    print(json.dumps(out))


if __name__ == "__main__" and len(sys.argv) == 2:
    child(sys.argv[1])
