"""Inputs of tests/test_gpu_summary.py: the pooled panel as read pairs, the two ways through the
demultiplexer (the merged reads resident in HBM against their host copy) and one digest over
everything either way returns.

Run as ``python -m tests.pooled_summary_cases`` it is the child process of the test whose
settings are read when the context is created (CRISPR_NWD_CHUNK, CRISPR_NWD_TALLY_SLOTS): one
JSON line with the digests of both ways, case by case, and the fallback reads.
"""
import hashlib
import json

import numpy as np

from tests import demux_cases as dc
from tests import demux_model as dm
from tests.alleles_cases import pack

KW = dict(min_hits=2, both_strands=True)
K = 16


def pairs_of(reads, n1=100, qual=b"I"):
    """Each read as a pair: R1 = its first n1 bases, R2 = the reverse complement of its last n1,
    constant quality; packed (s1, q1, off1, s2, q2, off2)."""
    r1 = [r[:n1] for r in reads]
    r2 = [dm.revcomp(r[-n1:]) for r in reads]
    s1, off1 = pack(r1)
    s2, off2 = pack(r2)
    return s1, np.full(len(s1), qual[0], np.uint8), off1, s2, np.full(len(s2), qual[0], np.uint8), off2


def single_of(reads, qual=b"I"):
    s1, off1 = pack(reads)
    return s1, np.full(len(s1), qual[0], np.uint8), off1, None, None, None


def cases():
    """{name: (amplicons, packed reads)}: the panel as pairs; reads stitched from five amplicons
    (more candidates than a small tally holds), single-end."""
    amps, reads = dc.pooled_panel()
    s_amps, s_reads = dc.stitched()
    return {"panel_pairs": ([a.encode() for a in amps], pairs_of(reads)),
            "stitched_single": (list(s_amps), single_of([r for r in s_reads if r]))}


def digest(got, pk, packed, pos, byt):
    h = hashlib.sha256()
    for part in (*got[:5], np.asarray(got[5:8], np.int64), pk.group_offsets, pk.order, pk.text_offsets, pk.lens,
                 pk.group_exc, np.asarray([pk.n_exc], np.int64), packed, pos, byt):
        h.update(np.ascontiguousarray(part).tobytes())
        h.update(b"|")
    return h.hexdigest()


def both_ways(d, al, amps, packed_reads):
    """(digest from the resident reads, digest from their host copy, fallback reads of the
    resident way, number of merged reads); the result is released before the packer runs."""
    from crispresso_amd import demux, frontend

    abuf, aoff = demux.pack_amplicons([a.decode() for a in amps])
    d.set_amplicons(abuf, aoff, K)
    al.set_reference(amps[0].decode())
    rr = frontend.prepare_packed_resident(al, *packed_reads)
    with rr:
        text, off = rr.fetch_text(), rr.offsets
        got = d.assign_prepared(rr, **KW)
        fallback = d.last_fallback()
    pk = d.pack(got[5])
    mine = digest(got, pk, *d.fetch_packed())
    host = d.assign(np.ascontiguousarray(text), off, **KW)
    hp = d.pack(host[5])
    theirs = digest(host, hp, *d.fetch_packed())
    assert d.last_fallback() == fallback
    return mine, theirs, fallback, len(rr)


def child():
    from crispresso_amd import demux
    from crispresso_amd.aligner import GpuAligner

    out = {"mine": [], "theirs": [], "fallback": [], "m": []}
    with demux.GpuDemultiplexer(0) as d, GpuAligner(0) as al:
        for name, (amps, packed_reads) in sorted(cases().items()):
            mine, theirs, fallback, m = both_ways(d, al, amps, packed_reads)
            out["mine"].append(mine)
            out["theirs"].append(theirs)
            out["fallback"].append(fallback)
            out["m"].append(m)
    print(json.dumps(out))


if __name__ == "__main__":
    child()
