"""tests/exception_cases.py held to its conditions (CPU): every class of exception read is present, so
that no test of tests/test_gpu_exceptions.py passes on an empty class; the packer's exception list, the
chunk slices the host takes of it and classify's search for an exception's read, each against a short
numpy restatement on the batch's own offsets."""
import numpy as np
import pytest

from crispresso_amd.aligner import pack_2bit
from oracle import oracle_py
from tests import exception_cases as ec

SEEDS = (0, 1, 2)


@pytest.fixture(scope="module", params=SEEDS)
def b(request):
    return ec.batch(request.param)


def test_every_class_occurs(b):
    assert b.n == ec.N_READS and len(b.labels) == b.n
    assert len(b.amp) == ec.LA and len(b.hdr) == ec.LA and b.amp != b.hdr
    seen = set(b.labels)
    assert seen == set(ec.LABELS), set(ec.LABELS) ^ seen
    exc = b.has_exception()
    for lab, x in zip(b.labels, exc):
        assert x == lab.startswith("x_"), lab
    assert exc.mean() >= 0.40
    assert exc[::2].all()            # every second read
    assert exc[0] and exc[-1]


def test_classes_are_what_their_labels_say(b):
    A, H = b.amp.encode(), b.hdr.encode()
    by = {}
    for i, lab in enumerate(b.labels):
        by.setdefault(lab, []).append(i)
    r = lambda lab: [b.reads[i] for i in by[lab]]
    assert all(x[0:1] == b"N" and x[1:] == A[1:] for x in r("x_first_byte"))
    assert all(x[-1:] == b"N" and x[:-1] == A[:-1] for x in r("x_last_byte"))
    # one N at batch positions of every residue mod 16
    res = set()
    for i in by["x_res16"]:
        x = b.reads[i]
        assert x.count(b"N") == 1
        res.add(int(b.off[i] + x.index(b"N")) % 16)
    assert res == set(range(16))
    for i in by["x_nn_dword"]:   # NN across a dword boundary of the batch
        p = int(b.off[i]) + b.reads[i].index(b"NN")
        assert p % 4 == 3 and b.reads[i].count(b"N") == 2
    assert all(b"N" * 5 in x and x.count(b"N") == 5 for x in r("x_run5"))
    assert all(b"N" * 17 in x and x.count(b"N") == 17 for x in r("x_run17"))
    assert all(x == b"N" * ec.LA for x in r("x_all_n"))
    # the last byte of read i and the first byte of read i + 1 both exceptions
    assert any(b.labels[i + 1] == "x_pair_first" for i in by["x_pair_last"])
    for i in by["x_pair_last"]:
        assert b.reads[i][-1:] == b"N"
    for i in by["x_pair_first"]:
        assert b.reads[i][0:1] == b"N" and b.reads[i - 1][-1:] not in (b"A", b"C", b"G", b"T")
    for name, byte in zip(("R", "Y", "dash", "n", "star", "high"), ec.OTHER_BYTES):
        assert all(x.count(byte) == 1 for x in r("x_byte_" + name))
    assert ec.OTHER_BYTES[-1][0] >= 0x80
    # N where the amplicon has A: the 2-bit decoding of the read equals the amplicon
    dec = lambda x: bytes(c if c in b"ACGT" else ord("A") for c in x)
    assert all(dec(x) == A and A[x.index(b"N")] == ord("A") for x in r("x_amp_n_at_a"))
    assert all(ec.hamming(dec(x), A) == 1 and A[x.index(b"N")] == ord("C") for x in r("x_amp_n_at_c"))
    for x in r("x_hdr_n_at_a_block"):
        assert dec(x) == H and ec.HDR_START <= x.index(b"N") < ec.HDR_START + ec.HDR_LEN
    for x in r("x_hdr_n_at_a_outside"):
        assert dec(x) == H and not ec.HDR_START <= x.index(b"N") < ec.HDR_START + ec.HDR_LEN
    # what would take a certificate, plus one N (at a place that agrees with the amplicon)
    for k in (1, 2, 3):
        for x in r(f"x_sub{k}_n"):
            assert len(x) == ec.LA and x.count(b"N") == 1
            assert ec.hamming(x.replace(b"N", A[x.index(b"N"):x.index(b"N") + 1]), A) == k
    for x in r("x_indel1_n"):
        i = x.index(b"N")
        assert x.count(b"N") == 1 and ec.one_indel_of(x[:i] + A[i:i + 1] + x[i + 1:], A)
    assert all(x == b"N" for x in r("x_len1"))
    assert all(len(x) == 2 for x in r("x_len2")) and all(len(x) == 3 for x in r("x_len3"))
    for m in range(4):
        assert all(len(x) % 4 == m and len(x) < ec.LA for x in r(f"x_len_mod{m}"))
    assert all(len(x) > ec.LA for x in r("x_longer"))
    # plain neighbours
    assert all(x == A for x in r("p_exact")) and all(x == H for x in r("p_hdr"))
    assert all(len(x) == ec.LA and ec.hamming(x, A) == 1 for x in r("p_sub1"))
    assert all(ec.one_indel_of(x, A) for x in r("p_del") + r("p_ins"))


def test_boundaries_fall_between_exception_reads(b):
    exc = b.has_exception()
    for m in ec.BOUNDARIES:
        for q in range(m, b.n, m):
            assert exc[q - 1] and exc[q], (m, q)
    # the chunks the host plans for CRISPR_NW_CHUNK = 257 and 1024, and for the pooled test's groups under 257
    G = ec.POOLED_GROUPS
    spans = [(0, b.n, 257), (0, b.n, 1024)] + [(g0, g1, 257) for g0, g1 in zip(G[:-1], G[1:])]
    for g0, g1, chunk in spans:
        cuts = g0 + np.cumsum(ec.plan_sizes(g1 - g0, chunk))
        assert cuts[-1] == g1 and max(ec.plan_sizes(g1 - g0, chunk)) <= chunk
        for q in list(cuts[:-1]) + ([g0] if g0 else []):
            assert exc[q - 1] and exc[q]
            assert b.reads[q - 1][-1:] == b"N" and b.reads[q][0:1] == b"N"   # and the exceptions meet across it


def test_packer_lists_the_exceptions(b):
    for base in (0, 7):   # the batch at the start of its buffer and mid-buffer
        full = np.concatenate([np.frombuffer(b"ACGTACG"[:base], np.uint8), b.buf])
        pr = pack_2bit(full, b.off + base)
        is_exc = ~np.isin(b.buf, np.frombuffer(b"ACGTacgt", np.uint8))
        pos = np.flatnonzero(is_exc) + base
        assert np.array_equal(pr.exc_pos, pos) and np.array_equal(pr.exc_byte, b.buf[pos - base])
        assert set((pr.exc_pos % 16).tolist()) == set(range(16))
        assert pr.lens is not None and np.array_equal(pr.lens, np.diff(b.off))
        # the 2-bit stream: (byte >> 1) & 3 of every base, 0 at an exception
        codes = np.where(is_exc, 0, (b.buf >> 1) & 3)
        stream = np.unpackbits(pr.packed, bitorder="little").reshape(-1, 2)
        got = (stream[:, 0] | (stream[:, 1] << 1))[base:base + len(b.buf)]
        assert np.array_equal(got, codes)


def test_oracle_aligns_every_read(b):
    for ref in (b.amp, b.hdr):
        res, aln = oracle_py.align_batch(ref, b.buf, b.off, None, nthreads=8)
        assert len(res) == b.n and (res["aln_len"] >= np.maximum(np.diff(b.off), len(ref))).all()
        assert (res["aln_len"] <= np.diff(b.off) + len(ref)).all()


def test_classify_read_search_restated(b):
    """classify's search for the read of an exception at batch position p, block by block (256 reads: the
    block's offsets s_off[0 .. cnt], "the last read starting at or before p" among reads 0 .. cnt - 1),
    against numpy's searchsorted on the whole batch's offsets."""
    pos, _ = ec.exceptions_of(b.buf)
    assert (np.diff(b.off) > 0).all()   # (no zero-length reads: they own no position)
    want = np.searchsorted(b.off, pos, "right") - 1
    flagged = np.zeros(b.n, bool)
    for bl in range(0, b.n, 256):
        bh = min(b.n, bl + 256)
        s_off, cnt = b.off[bl:bh + 1], bh - bl
        x0, x1 = np.searchsorted(pos, s_off[0], "left"), np.searchsorted(pos, s_off[cnt], "left")
        for t in range(x0, x1):
            p, lo, hi = pos[t], 0, cnt - 1
            while lo < hi:
                mid = (lo + hi + 1) >> 1
                if s_off[mid] <= p:
                    lo = mid
                else:
                    hi = mid - 1
            assert bl + lo == want[t]
            flagged[bl + lo] = True
    assert np.array_equal(flagged, b.has_exception())


@pytest.mark.parametrize("chunk", [257, 1024])
def test_chunk_slices_partition_the_exception_list(b, chunk):
    """The host slices the call's exception list per chunk with lower_bound at offsets[lo] and offsets[hi]:
    the slices are disjoint, in order, cover the list, and each holds exactly its chunk's reads' exceptions."""
    for base in (0, 7):
        pos, _ = ec.exceptions_of(b.buf, base)
        off = b.off + base
        cuts = np.concatenate([[0], np.cumsum(ec.plan_sizes(b.n, chunk))])
        e_prev = 0
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            e0, e1 = np.searchsorted(pos, off[lo], "left"), np.searchsorted(pos, off[hi], "left")
            assert e0 == e_prev and e1 > e0   # (every chunk starts and ends on an exception read)
            assert ((pos[e0:e1] >= off[lo]) & (pos[e0:e1] < off[hi])).all()
            if lo > 0:
                assert pos[e0] == off[lo]        # the chunk's first byte
            if hi < b.n:
                assert pos[e1 - 1] == off[hi] - 1   # and its last
            e_prev = e1
        assert e_prev == len(pos)


def test_certifiable_counts_only_plain_reads(b):
    """The bound the GPU tests put on the certificate counters: plain reads only."""
    plain = int((~b.has_exception()).sum())
    lab = np.array(b.labels)
    amp_only = int(np.isin(lab, ["p_exact", "p_sub1", "p_del", "p_ins"]).sum())
    hdr_only = int((lab == "p_hdr").sum())
    assert ec.certifiable(b, b.amp, None) == amp_only
    assert ec.certifiable(b, b.amp, b.hdr) == amp_only + hdr_only == plain
    assert ec.certifiable(b, b.hdr, None) == hdr_only
    assert ec.certifiable(b, b.hdr, b.amp) == hdr_only + int((lab == "p_exact").sum())
