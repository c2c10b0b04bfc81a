"""Inputs and the checks of tests/test_gpu_resident_alleles.py: hand-built alignments as
(runs, read bytes, class) against one amplicon, uploaded the way tests/around_cut_cases.py uploads
them but with the keep flags and the nwq_read records on the device as well; the rows the host
path gives for them (alleles.group_reads_host + nw_expand_ops_subset); and the device calls
(nwa_table_device / nwa_table_fetch, nwa_windows_resident).

Run as ``python -m tests.resident_alleles_cases forced`` it is the child process of the
forced-collision test (CRISPR_NWA_HASH_BITS is read when the context is created).
"""
import ctypes
import json
import sys

import numpy as np

from tests.alleles_cases import pack

M, X, Y = 0, 1, 2
FILL = 0xEE


def amplicon(la, seed=81):
    rng = np.random.Generator(np.random.PCG64(seed + la))
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), la)).decode()


def read_of(amp, runs, cls=1, subs=None, seed=0, alphabet=b"ACGT"):
    """The read an alignment of `runs` against `amp` comes from: M copies the amplicon (position
    p of the amplicon replaced by subs[p]), X inserts bytes of `alphabet`, Y skips."""
    rng = np.random.Generator(np.random.PCG64(2000 + seed))
    subs = subs or {}
    out, ia = bytearray(), 0
    for t, l in runs:
        if t == M:
            out += bytes(subs.get(i, ord(amp[i])) for i in range(ia, ia + l))
            ia += l
        elif t == X:
            out += bytes(rng.choice(np.frombuffer(alphabet, np.uint8), l))
        else:
            ia += l
    assert ia == len(amp), (runs, ia)
    return {"runs": list(runs), "seq": bytes(out), "cls": cls}


def alternating(la, k):
    """k runs: M1 X1 M1 Y1 ... and a last M run with the rest of the amplicon."""
    runs, ia = [], 0
    for j in range(k - 1):
        t = (M, X, M, Y)[j % 4]
        runs.append((t, 1))
        ia += t != X
    assert ia < la
    return runs + [(M, la - ia)]


def single_run_reads(amp):
    """Alignments of len(amp) columns: the amplicon itself (three times), and one substitution
    at the first, the middle and the last base (the middle one twice)."""
    la = len(amp)
    flip = {"A": "C", "C": "G", "G": "T", "T": "A"}
    out = [read_of(amp, [(M, la)], cls=0)] * 3
    for p in sorted({0, la // 2, la - 1}):
        rd = read_of(amp, [(M, la)], subs={p: ord(flip[amp[p]])})
        out += [rd, rd] if p == la // 2 else [rd]
    return out


def shape_reads(amp):
    """The run shapes of one batch (amplicon of at least 140 bases): a single M run; a leading Y
    and a trailing X run; alternating runs numbering 64, 65 and 130 (one wavefront step, one
    more, and three steps); N, IUPAC and '-' bytes in M and X runs; a read of no byte."""
    la = len(amp)
    return [
        read_of(amp, [(M, la)], cls=0),
        read_of(amp, [(Y, 7), (M, la - 7), (X, 5)], seed=1),
        read_of(amp, alternating(la, 64), seed=2),
        read_of(amp, alternating(la, 65), seed=3),
        read_of(amp, alternating(la, 130), seed=4),
        read_of(amp, [(M, la)], cls=0),
        read_of(amp, [(M, 40), (X, 70), (M, la - 40)], seed=5, alphabet=b"ACGTNRYK-"),
        read_of(amp, [(M, la)], subs={3: ord("N"), 64: ord("R"), la - 1: ord("-"), 70: ord("S")}),
        read_of(amp, [(X, 66), (Y, la)], seed=6),                 # no M column at all
        read_of(amp, alternating(la, 130), seed=4),
        read_of(amp, [(Y, la)], cls=1),                           # a kept read of no byte with a run
        {"runs": [], "seq": b"", "cls": 0, "drop": True},           # no byte, no run: never kept here
    ]


def cycled(distinct, n):
    return [distinct[j % len(distinct)] for j in range(n)]


def results_of(reads):
    """nwq_read records that are a function of the read's bytes and runs (identical reads carry
    identical records, as the quantifier's do)."""
    n = len(reads)
    rr = np.full((max(n, 1), 4), 9, np.int32)
    for j, rd in enumerate(reads):
        rr[j] = (rd["cls"], sum(rd["seq"]) % 11, sum(l for t, l in rd["runs"] if t == X),
                 sum(l for t, l in rd["runs"] if t == Y))
    return rr


class Arrays:
    """The host arrays of a batch as they are uploaded."""

    def __init__(self, amp, reads, lead=0, bias=0, aln_len=None):
        self.amp, self.reads, self.bias, self.n = amp, reads, bias, len(reads)
        n = self.n
        self.buf, self.off = pack([rd["seq"] for rd in reads], lead, bias)
        self.ops = np.array([t << 28 | l for rd in reads for t, l in rd["runs"]] + [0xDEADBEEF], np.uint32)
        self.ops_off = np.zeros(n + 1, np.int64)
        np.cumsum([len(rd["runs"]) for rd in reads], out=self.ops_off[1:])
        self.stats = np.full((max(n, 1), 8), -7, np.int32)
        self.stats[:n, 0] = [sum(l for _, l in rd["runs"]) for rd in reads] if aln_len is None else aln_len
        self.rr = results_of(reads)


def host_table(lib, arrays, keep, awidth):
    """(first, count, cols, [(aligned-read row, reference row)], results) of the kept reads from
    the host text: alleles.group_reads_host, then nw_expand_ops_subset for the groups' first
    reads, cut to min(aln_len, awidth) columns."""
    from crispresso_amd import _lib, alleles

    a = arrays
    off = np.ascontiguousarray(a.off - a.bias)
    groups = alleles.group_reads_host(a.buf, off, keep=keep)
    idx = np.ascontiguousarray(groups.first, np.int64)
    m = len(idx)
    aln = a.stats[idx, 0].astype(np.int64) if m else np.zeros(0, np.int64)
    stride = max(16, (int(aln.max()) + 15) & ~15) if m else 16
    rows = np.zeros((max(m, 1), 3, stride), np.uint8)
    amp = a.amp.encode()
    rc = lib.nw_expand_ops_subset(amp, len(amp), _lib.ptr(a.buf), _lib.ptr(off), _lib.ptr(idx), m, _lib.ptr(a.ops),
                                  _lib.ptr(a.ops_off), _lib.ptr(rows), stride, 1)
    assert rc == 0, rc
    cols = np.minimum(aln, awidth)
    pairs = [(bytes(rows[q, 2, :c]), bytes(rows[q, 0, :c])) for q, c in enumerate(cols.tolist())]
    return idx.tolist(), groups.count.tolist(), cols.tolist(), pairs, a.rr[idx].tolist() if m else []


def device_table(lib, ctx, arrays, keep, awidth, fetch=True):
    """nwa_table_device on own device buffers (keep: uint8 values as given, or None for NULL) ->
    (rc, n_groups, row_stride, rows uint8 [groups][2][stride] fetched into a pre-filled array,
    cols, first, count, results)."""
    from crispresso_amd import _lib
    from crispresso_amd.devmem import DeviceBuffer

    a = arrays
    amp = a.amp.encode()
    ng, stride = ctypes.c_int64(-5), ctypes.c_int32(-5)
    keep_arr = np.zeros(max(a.n, 1), np.uint8)
    if keep is not None:
        keep_arr[:a.n] = keep
    with DeviceBuffer.from_array(a.buf) as d_buf, DeviceBuffer.from_array(a.off) as d_off, \
            DeviceBuffer.from_array(a.ops) as d_ops, DeviceBuffer.from_array(a.ops_off) as d_ops_off, \
            DeviceBuffer.from_array(a.stats) as d_stats, DeviceBuffer.from_array(a.rr) as d_rr, \
            DeviceBuffer.from_array(keep_arr) as d_keep:
        rc = lib.nwa_table_device(ctx, d_ops.ptr, d_ops_off.ptr, d_stats.ptr, d_buf.ptr, d_off.ptr, a.bias, a.n,
                                  awidth, amp, len(amp), d_keep.ptr if keep is not None else None, d_rr.ptr,
                                  ctypes.byref(ng), ctypes.byref(stride))
    g, w = int(ng.value), int(stride.value)
    if rc != 0 or not fetch:
        return rc, g, w, None, None, None, None, None
    rows = np.full((max(g, 1), 2, max(w, 1)), FILL, np.uint8)
    cols, res = np.full(max(g, 1), -5, np.int32), np.full((max(g, 1), 4), -5, np.int32)
    first, count = np.full(max(g, 1), -5, np.int64), np.full(max(g, 1), -5, np.int64)
    assert lib.nwa_table_fetch(ctx, _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(first), _lib.ptr(count), _lib.ptr(res)) == 0
    return rc, g, w, rows[:g], cols[:g].tolist(), first[:g].tolist(), count[:g].tolist(), res[:g].tolist()


def same_as_host(lib, ctx, arrays, keep, awidth):
    """One nwa_table_device call against host_table; returns what the device gave."""
    want_first, want_count, want_cols, want_rows, want_res = host_table(lib, arrays, keep, awidth)
    got = device_table(lib, ctx, arrays, keep, awidth)
    rc, g, w, rows, cols, first, count, res = got
    assert rc == 0, lib.nwa_last_error(ctx)
    assert g == len(want_first) and first == want_first and count == want_count and cols == want_cols and res == want_res
    if g == 0:
        assert w == 0
        return got
    assert w == max(16, (max(want_cols) + 15) & ~15)
    for q, c in enumerate(cols):
        assert (bytes(rows[q, 0, :c]), bytes(rows[q, 1, :c])) == want_rows[q], q
        assert not rows[q, :, c:].any(), q                       # zero-padded, over the 0xEE it was fetched into
    return got


def device_windows_resident(lib, ctx, batch, cuts, offset, keep=None, tag=None, want_gor=True):
    """tests.around_cut_cases.device_windows through nwa_windows_resident: the same batch with
    the keep flags (values as given) and the results on the device."""
    from crispresso_amd import _lib
    from crispresso_amd.devmem import DeviceBuffer

    reads = batch.reads
    n = len(reads)
    buf, off = pack([rd["seq"].encode() for rd in reads])
    ops = np.array([t << 28 | l for rd in reads for t, l in rd["runs"]] + [0xDEADBEEF], np.uint32)
    ops_off = np.zeros(n + 1, np.int64)
    np.cumsum([len(rd["runs"]) for rd in reads], out=ops_off[1:])
    stats = np.full((max(n, 1), 8), -7, np.int32)
    stats[:n, 0] = [sum(l for _, l in rd["runs"]) for rd in reads]
    rr = np.full((max(n, 1), 4), 9, np.int32)
    rr[:n, 0] = [rd["cls"] for rd in reads]
    keep_arr = np.zeros(max(n, 1), np.uint8)
    if keep is not None:
        keep_arr[:n] = keep
    tag = None if tag is None else np.ascontiguousarray(tag, np.int32)
    cuts = np.ascontiguousarray(cuts, np.int32)
    ng = np.full(max(len(cuts), 1), -5, np.int64)
    bad, first_bad = ctypes.c_int64(-5), ctypes.c_int64(-5)
    amp = batch.amp.encode()
    with DeviceBuffer.from_array(buf) as d_buf, DeviceBuffer.from_array(off) as d_off, \
            DeviceBuffer.from_array(ops) as d_ops, DeviceBuffer.from_array(ops_off) as d_ops_off, \
            DeviceBuffer.from_array(stats) as d_stats, DeviceBuffer.from_array(rr) as d_rr, \
            DeviceBuffer.from_array(keep_arr) as d_keep:
        rc = lib.nwa_windows_resident(ctx, d_ops.ptr, d_ops_off.ptr, d_stats.ptr, d_buf.ptr, d_off.ptr, 0, n,
                                      batch.awidth, amp, len(amp), _lib.ptr(cuts), len(cuts), offset,
                                      d_keep.ptr if keep is not None else None, _lib.ptr(tag), d_rr.ptr, int(want_gor),
                                      _lib.ptr(ng), ctypes.byref(bad), ctypes.byref(first_bad))
    out = []
    if rc == 0 and bad.value == 0:
        W = 2 * offset
        for k in range(len(cuts)):
            g = int(ng[k])
            win = np.full((max(g, 1), 2, W), 0xEE, np.uint8)
            wl, un = np.zeros(max(g, 1), np.int32), np.zeros(max(g, 1), np.uint8)
            first, count = np.zeros(max(g, 1), np.int64), np.zeros(max(g, 1), np.int64)
            gor = np.full(max(n, 1), -5, np.int32) if want_gor else None
            assert lib.nwa_windows_fetch(ctx, k, _lib.ptr(win), _lib.ptr(wl), _lib.ptr(first), _lib.ptr(count),
                                         _lib.ptr(un), _lib.ptr(gor)) == 0
            assert all(not win[i, :, wl[i]:].any() for i in range(g))
            wins = [(bytes(win[i, 0, :wl[i]]).decode(), bytes(win[i, 1, :wl[i]]).decode()) for i in range(g)]
            out.append((first[:g].tolist(), count[:g].tolist(), None if gor is None else gor[:n].tolist(),
                        un[:g].tolist(), wins))
    return rc, int(bad.value), int(first_bad.value), out, ng[: len(cuts)].tolist()


def collision_arrays():
    """1,000 reads of 120 distinct single-substitution and single-insertion alleles of one
    150-base amplicon, in random order."""
    amp = amplicon(150)
    rng = np.random.Generator(np.random.PCG64(17))
    flip = {"A": "C", "C": "G", "G": "T", "T": "A"}
    distinct = [read_of(amp, [(M, 150)], cls=0)]
    for p in range(1, 60):
        distinct.append(read_of(amp, [(M, 150)], subs={p: ord(flip[amp[p]])}))
    for p in range(60, 120):
        distinct.append(read_of(amp, [(M, p), (X, 2), (M, 150 - p)], seed=p))
    reads = [distinct[i] for i in rng.integers(0, len(distinct), 1000)]
    return Arrays(amp, reads, lead=1)


def forced_child():
    """The forced-collision run: collision_arrays() twice on one context against the host path,
    with and without keep flags; one JSON line."""
    from crispresso_amd import _lib

    lib = _lib.load()
    ctx = ctypes.c_void_p()
    rc = lib.nwa_create(0, ctypes.byref(ctx))
    if rc != 0:
        print(json.dumps({"ok": False, "why": f"nwa_create {rc}"}))
        return
    a = collision_arrays()
    out = {"ok": True, "collided": [], "why": ""}
    for keep in (None, (np.arange(a.n) % 5 != 0).astype(np.uint8) * 2, None):
        try:
            same_as_host(lib, ctx, a, keep, 5000)
        except AssertionError as exc:
            out["ok"], out["why"] = False, repr(exc)[:500]
        out["collided"].append(int(lib.nwa_table_collided(ctx)))
    lib.nwa_destroy(ctx)
    print(json.dumps(out))


if __name__ == "__main__" and sys.argv[1:] == ["forced"]:
    forced_child()
