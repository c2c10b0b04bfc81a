"""Inputs of the grouped-read packer's tests (tests/test_demux_pack_model.py,
tests/test_gpu_demux_resident.py): amplicons and reads as lists of ``bytes`` with fixed seeds, all
for k = 8 and min_hits = 1 so that reads as short as 8 bases are assigned.  Every piece is taken
where tests/demux_model.py assigns it to the group and strand meant, and
tests/test_demux_pack_model.py::test_cases_are_what_they_claim holds each case to its docstring.

Run as ``python -m tests.demux_pack_cases <case>`` it is the child process of the tests whose
setting is read when the context is created (CRISPR_NWD_CHUNK, CRISPR_NWD_TALLY_SLOTS): one JSON
line with a digest of everything the packer returned.
"""
import functools
import hashlib
import json
import sys

import numpy as np

from tests import demux_cases as dc
from tests import demux_model as dm
from tests.alleles_cases import pack

K, MIN_HITS = 8, 1
KW = {"k": K, "min_hits": MIN_HITS}
BLOCK = 4096          # gathered positions per block of the packer's count kernel (256 dwords)
LEN_GROUP = 1024      # nw::kLenGroup


@functools.lru_cache(maxsize=None)
def amplicons():
    """One amplicon long enough for a 4096-base read and five short ones."""
    return tuple([dc.bases(4200, 701)] + [dc.bases(300, 702 + g) for g in range(5)])


@functools.lru_cache(maxsize=None)
def _index():
    return dm.build_index(amplicons(), K)


def piece(g, n, strand=0, hint=0):
    """n bases of amplicon g that the rule assigns to (g, strand) -- the first start at or after
    ``hint`` at which it does -- given as the read that gathers to them: reverse-complemented
    for strand 1."""
    amp = amplicons()[g]
    for s in list(range(hint, len(amp) - n + 1)) + list(range(0, hint)):
        o = amp[s:s + n]
        read = dm.revcomp(o) if strand else o
        if dm.decide(dm.votes_of(_index(), read, K), MIN_HITS)[:2] == (g, strand):
            return read
    raise AssertionError(f"no piece of {n} bases in amplicon {g}")


def with_breaks(read, strand, positions, byte=b"N"):
    """``read`` with ``byte`` at the given positions of its gathered orientation."""
    o = dm.revcomp(read) if strand else read
    for p in positions:
        o = o[:p] + byte + o[p + 1:]
    return dm.revcomp(o) if strand else o


def lengths():
    """8, 15, 16, 17, 31, 32, 33 and 4096 bases in one group, both strands: dwords hold the end
    of one read and the start of the next, and in places three reads."""
    order = [15, 8, 8, 16, 17, 31, 32, 33, 4096, 8, 8, 8, 15, 33, 8, 17, 4096, 31]
    reads = [piece(0, n, i % 2, 37 * i) for i, n in enumerate(order)]
    return list(amplicons()), reads


def phases():
    """Groups that start at gathered positions 21, 31 and 50 (1, 3, 2 mod 4; 5, 15 mod 16), an
    empty group between two others, a first and a last group of one read each; the reads given in
    another order than the groups'."""
    plan = [(5, 33, 1), (1, 21, 0), (4, 20, 1), (2, 10, 1), (4, 9, 0), (3, 19, 0), (4, 40, 1)]   # (group, bases, strand)
    amps = list(amplicons())[1:]            # (without the long amplicon: group 0 is the plan's 1)
    amps.insert(2, dc.bases(120, 777))      # amplicon 2 gets no read; the plan's groups 3.. keep their number
    reads = []
    index = dm.build_index(amps, K)
    for i, (g, n, s) in enumerate(plan):
        g2 = g - 1 if g < 3 else g
        amp = amps[g2]
        for st in range(11 * i, len(amp) - n):
            o = amp[st:st + n]
            r = dm.revcomp(o) if s else o
            if dm.decide(dm.votes_of(index, r, K), MIN_HITS)[:2] == (g2, s):
                reads.append(r)
                break
    assert len(reads) == len(plan)
    return amps, reads


def one_group():
    """Every read in one group, neither the first nor the last."""
    reads = [piece(2, 8 + (5 * i) % 60, i % 2, 7 * i) for i in range(40)]
    return list(amplicons()), reads


def strand_breaks():
    """Strand-1 reads with an N at their first base, their last base and on both sides of the
    dword boundary that falls inside them after the reversal; lower-case reads on both strands;
    a read that is all exceptions apart from the window that assigns it.  All in one group."""
    reads, at = [], 0
    for i, n in enumerate([40, 41, 43, 40, 47, 40, 45, 40]):
        s = 1 if i != 3 else 0
        r = piece(1, n, s, 13 * i)
        edge = (-at) % 16 or 16                       # a dword starts at this base of the gathered read
        where = {0: [0], 1: [n - 1], 2: [edge - 1, edge], 3: [edge], 4: [edge + 15, edge + 16], 5: [0, n - 1],
                 6: [edge - 1], 7: []}[i]
        r = with_breaks(r, s, where, b"N" if i % 2 == 0 else b"n")
        reads.append(r.lower() if i in (4, 7) else r)
        at += n
    reads += [piece(1, 30, 0, 50).lower(), piece(1, 30, 1, 90).lower(), piece(1, 25, 1, 120).swapcase()]
    core = piece(1, 8, 1, 200)
    reads += [b"N" * 20 + core + b"-" * 13, b"RYKM" + piece(1, 9, 0, 150) + b"nnnnn."]
    return list(amplicons()), reads


def exception_blocks():
    """Exceptions in every position of the two dwords before and the two after the first block
    boundary of the count kernel, and a run of them further on."""
    a = piece(0, 4090, 0, 10)
    a = with_breaks(a, 0, range(4060, 4090))
    b = with_breaks(piece(0, 80, 1, 500), 1, range(0, 40), b"-")
    c = with_breaks(piece(0, 4096, 1, 60), 1, range(4000, 4096, 3))
    d = with_breaks(piece(0, 64, 0, 900), 0, [0, 1, 2, 31, 32, 33])
    return list(amplicons()), [a, b, c, d]


def no_exceptions():
    amps, reads = lengths()
    more = [piece(g, 20 + 3 * i, i % 2, 17 * i) for i, g in enumerate([1, 2, 4, 5, 2, 1])]
    return amps, reads + more


def long_group():
    """Three reads in group 0, then LEN_GROUP + 1 in group 1: the second group's base offsets are
    every 1024th offset counted from gathered read 3."""
    reads = [piece(1, 11, 0, 3), piece(1, 9, 1, 40), piece(1, 14, 0, 80)]
    for i in range(LEN_GROUP + 1):
        reads.append(piece(2, 8 + i % 9, i % 2, (3 * i) % 250))
    rng = np.random.Generator(np.random.PCG64(5))
    where = sorted(int(x) for x in rng.choice(np.arange(3, len(reads)), 12, replace=False))
    for r in where:                                   # a few exceptions on both sides of read 3 + 1024
        reads[r] = reads[r] + b"N"
    reads[3 + LEN_GROUP - 1] += b"N"
    reads[3 + LEN_GROUP] = b"N" + reads[3 + LEN_GROUP]
    return list(amplicons()), reads


def none_assigned():
    return list(amplicons()[1:3]), [dc.bases(7, 1), b"", b"NNNNNNNNNNNN", amplicons()[1][:7]]


CASES = {"lengths": lengths, "phases": phases, "one_group": one_group, "strand_breaks": strand_breaks,
         "exception_blocks": exception_blocks, "no_exceptions": no_exceptions, "long_group": long_group,
         "none_assigned": none_assigned}


@functools.lru_cache(maxsize=None)
def case(name):
    """(amplicons, reads, the model's dict) of one case, computed once."""
    amps, reads = CASES[name]()
    want = dm.demultiplex(amps, reads, **KW)
    return amps, reads, want


def gathered(want):
    """(text, text_offsets) of the model's groups: what nwd_gather returns."""
    flat = [r for grp in want["groups"] for r in grp]
    return pack(flat)


def digest(pk, packed, exc_pos, exc_byte):
    h = hashlib.sha256()
    for part in (pk.group_offsets, pk.order, pk.text_offsets, pk.lens, pk.group_exc, packed, exc_pos, exc_byte):
        h.update(np.ascontiguousarray(part).tobytes())
        h.update(b"|")
    return h.hexdigest()


def run_pack(d, amps, reads):
    """set_amplicons, assign, pack, fetch on demultiplexer ``d``: (assign's tuple, PackedGroups,
    packed, exc_pos, exc_byte)."""
    from crispresso_amd import demux

    abuf, aoff = demux.pack_amplicons(list(amps))
    rbuf, roff = pack(reads)
    d.set_amplicons(abuf, aoff, K)
    got = d.assign(rbuf, roff, MIN_HITS, True)
    pk = d.pack(got[5])
    return (got, pk) + tuple(d.fetch_packed())


def child(names):
    from crispresso_amd import demux

    out = {"digest": [], "fallback": []}
    with demux.GpuDemultiplexer(0) as d:
        for name in names:
            amps, reads = CASES[name]()
            _, pk, packed, pos, byt = run_pack(d, amps, reads)
            out["digest"].append(digest(pk, packed, pos, byt))
            out["fallback"].append(d.last_fallback())
    print(json.dumps(out))


if __name__ == "__main__" and len(sys.argv) >= 2:
    child(sys.argv[1:])
