"""Reads with exception bytes (tests/exception_cases.py: N, IUPAC codes, '-', any byte that is not ACGTacgt,
at every place the packed aligner does position arithmetic on them) through every entry point that takes
a packed batch, every read against the CPU oracle (tests/every_read.py).

The packed call (with lengths, without, mid-buffer), the resident passes, the pooled call and the dual
call, each under the chunk sizes that put a chunk boundary between two exception reads and on both
paths: the band path (classify decodes the 2-bit reads and writes the DP reads' bytes, exceptions in
place) and CRISPR_NW_KERNEL=full (the unpack kernels write every byte, the exact kernels read them).

The dual call runs its two passes on concurrent streams over one byte buffer (while a kernel
of one pass may read a byte, the other pass stores nothing but that byte's final value to it).  A test
cannot make a race deterministic; these put ~3000 exception reads per pass into every dual case, and
under CRISPR_NW_CHUNK=257 24 interleaved chunk pairs.

Counters (band path): GpuAligner.path_counts()["exact_copies"] is the number of reads that left classify
and nw_band_cert certified (exact copies, one to three substitutions, one indel, window and known copies:
the call's reads minus its DP reads).  No read with an exception byte may be among them, so it can never
exceed exception_cases.certifiable(): the reads WITHOUT an exception byte that some certificate could take.
"""
import dataclasses
import functools

import numpy as np
import pytest

from crispresso_amd import synth
from crispresso_amd.aligner import pack_2bit
from tests import exception_cases as ec
from tests.every_read import every_read, every_read_multi, every_read_records

pytestmark = pytest.mark.gpu

THREADS = 16
CHUNKS = [None, 1024, 257]
PATHS = ["band", "full"]


@pytest.fixture
def aligners(gpu_aligner_factory):
    """The session's factory, with the contexts a test made closed when it ends."""
    made = []

    def make(options=None):
        a = gpu_aligner_factory(options)
        made.append(a)
        return a

    yield make
    for a in made:
        a.close()


def _env(monkeypatch, chunk, path):
    if chunk is None:
        monkeypatch.delenv("CRISPR_NW_CHUNK", raising=False)
    else:
        monkeypatch.setenv("CRISPR_NW_CHUNK", str(chunk))
    if path == "full":
        monkeypatch.setenv("CRISPR_NW_KERNEL", "full")
    else:
        monkeypatch.delenv("CRISPR_NW_KERNEL", raising=False)


@functools.lru_cache(maxsize=None)
def _packed(seed, form="lens"):
    """(text buffer, offsets, PackedReads) of the seed's batch: with the reads' lengths, without them
    (nw_align_ops_packed: the offsets cross), or starting mid-buffer at offset 7."""
    b = ec.batch(seed)
    buf, off = b.buf, b.off
    if form == "mid7":
        buf = np.concatenate([np.frombuffer(b"ACGTACG", np.uint8), b.buf])
        off = b.off + 7
    pr = pack_2bit(buf, off)
    assert pr.lens is not None and len(pr.exc_pos) > 3000
    if form == "nolens":
        pr = dataclasses.replace(pr, lens=None)
    return buf, off, pr


# One oracle comparison per (seed, amplicon): an output that every_read found equal to the oracle on
# every read is kept, and a later output of the same reads against the same amplicon that equals it
# in every record, run offset and run equals the oracle on every read too.  Anything else goes
# through every_read again (and fails there, with the reads it found).
_verified = {}


def _assert_oracle(seed, ref, buf, off, ob, what):
    n = len(off) - 1
    total = int(ob.ops_off[n])
    key = (seed, ref)
    if key in _verified:
        st, oo, ops = _verified[key]
        if (every_read_records(ob.stats, st) == 0 and np.array_equal(ob.ops_off[:n + 1], oo)
                and np.array_equal(ob.ops[:total], ops)):
            return
    res = every_read(ref, buf, off, ob, THREADS)
    assert res["mismatches"] == 0 and res["reads"] == n, (what, res)
    _verified.setdefault(key, (ob.stats[:n].copy(), ob.ops_off[:n + 1].copy(), ob.ops[:total].copy()))


def _assert_none_certified(a, seed, ref, known, path, what):
    """path_counts()["exact_copies"] (see the module's docstring) within what the plain reads allow."""
    if path == "full":
        return
    counts = a.path_counts()
    b = ec.batch(seed)
    allowed = ec.certifiable(b, ref, known)
    assert 0 < counts["exact_copies"] <= allowed, (what, counts, allowed)
    assert b.n - counts["exact_copies"] >= int(b.has_exception().sum())   # every exception read took the DP


# ---------------------------------------------------------------- the packed call

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("form", ["lens", "nolens", "mid7"])
def test_packed_call(aligners, monkeypatch, form, chunk, path):
    _env(monkeypatch, chunk, path)
    b = ec.batch(0)
    buf, off, pr = _packed(0, form)
    a = aligners()
    a.set_reference(b.amp)
    ob = a.align_ops_packed(pr)
    _assert_none_certified(a, 0, b.amp, None, path, (form, chunk))
    _assert_oracle(0, b.amp, buf, off, ob, ("packed call", form, chunk, path))


# ---------------------------------------------------------------- resident passes

@pytest.mark.parametrize("form", ["lens", "mid7"])
def test_resident_batch_runs_and_holds_every_byte(aligners, form):
    """upload_packed + run_async, twice, against the oracle; the device's byte buffer then holds every
    read's bytes upper-cased (what tests/test_gpu_ops.py reads of its packed batch upload)."""
    from crispresso_amd.devmem import _D2H, hip

    b = ec.batch(1)
    buf, off, pr = _packed(1, form)
    a = aligners()
    a.set_reference(b.amp)
    a.upload_packed(pr)
    for run in range(2):
        a.run_async()
        a.sync()
        ob = a.download_ops(b.n)
        _assert_none_certified(a, 1, b.amp, None, "band", ("resident batch", run))
        _assert_oracle(1, b.amp, buf, off, ob, ("resident batch", form, run))
    dev = a.device_ops()
    got = np.zeros(int(off[-1] - off[0]), np.uint8)
    assert hip().hipMemcpy(got.ctypes.data, dev["reads"] + int(off[0]) - dev["reads_bias"], got.nbytes, _D2H) == 0
    want = np.frombuffer(bytes(b.buf).upper(), np.uint8)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), bad[:10].tolist(), [b.labels[int(np.searchsorted(b.off, p, "right")) - 1]
                                                          for p in bad[:10]])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("chunk", [None, 257])
def test_resident_pass_after_a_packed_call(aligners, monkeypatch, chunk, path):
    """After a packed call, the reads still on the device against the HDR amplicon (align_ops resident),
    with runs and records only."""
    _env(monkeypatch, chunk, path)
    b = ec.batch(2)
    buf, off, pr = _packed(2)
    a = aligners()
    a.set_reference(b.amp)
    ob1 = a.align_ops_packed(pr)
    _assert_oracle(2, b.amp, buf, off, ob1, ("packed call before the resident pass", chunk, path))
    a.set_reference(b.hdr)
    ob2 = a.align_ops(None, pr.offsets, resident=True)
    # (the amplicon the batch was last aligned against is the resident pass's known sequence)
    _assert_none_certified(a, 2, b.hdr, b.amp, path, ("resident pass", chunk))
    _assert_oracle(2, b.hdr, buf, off, ob2, ("resident pass, runs", chunk, path))
    ob3 = a.align_ops(None, pr.offsets, resident=True, records_only=True)
    assert not ob3.has_runs and every_read_records(ob3.stats, ob2.stats) == 0


# ---------------------------------------------------------------- the pooled call

@pytest.mark.parametrize("path", PATHS)
def test_pooled_call_groups_cut_at_exception_reads(aligners, monkeypatch, path):
    """Four amplicons, the batch split between them at exception reads (exception_cases.POOLED_GROUPS: the
    last byte of a group and the first byte of the next are both exceptions), chunks of 257 reads (not
    aligned to classify's 256-read blocks)."""
    _env(monkeypatch, 257, path)
    b = ec.batch(0)
    buf, off, pr = _packed(0)
    amps = [b.amp, b.hdr, synth.hdr_amplicon(b.amp, seed=11, start=40, length=6),
            synth.hdr_amplicon(b.hdr, seed=12, start=200, length=4)]
    G = ec.POOLED_GROUPS
    which = np.repeat(np.arange(4, dtype=np.int32), np.diff(G))
    a = aligners()
    ob = a.align_multi_ops(amps, pr, None, which)
    res = every_read_multi(amps, buf, off, which, ob, THREADS)
    assert res["mismatches"] == 0 and res["reads"] == b.n, res


# ---------------------------------------------------------------- the dual call

@pytest.mark.parametrize("order", ["band-first", "unpack-first"])
@pytest.mark.parametrize("chunk", [None, 257])
def test_dual_call_one_pass_on_each_path(aligners, monkeypatch, order, chunk):
    """One amplicon of 250 bp (band path) and one over 1024 bp (exact kernels on unpacked bytes) in one dual
    call, either as the first: the read range is unpacked once, beside a classify that stores the same
    bytes.  1024 reads of the generator (the long amplicon's exact alignments are the slow part)."""
    _env(monkeypatch, chunk, "band")
    b = ec.batch(0, 1024)
    assert b.has_exception().mean() >= 0.40
    long_amp = b.amp + synth.random_amplicon(800, 77)
    pr = pack_2bit(b.buf, b.off)
    first, second = (b.amp, long_amp) if order == "band-first" else (long_amp, b.amp)
    a = aligners()
    a.set_reference(first)
    ob1, ob2 = a.align_dual_packed(pr, second)
    for ref, ob, what in ((first, ob1, "first pass"), (second, ob2, "second pass")):
        res = every_read(ref, b.buf, b.off, ob, THREADS)
        assert res["mismatches"] == 0 and res["reads"] == b.n, (what, order, chunk, res)


@pytest.mark.parametrize("path", PATHS + ["band+known"])
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_dual_call(aligners, monkeypatch, seed, chunk, path):
    """Both passes of the dual call against the oracle on every read, equal to two separate calls in
    records, run offsets and runs, and its records-only form equal to the runs form.  "band+known": the
    context holds set_known(hdr), as align_reads sets it for the amplicon pass."""
    known = path == "band+known"
    path = "band" if known else path
    _env(monkeypatch, chunk, path)
    b = ec.batch(seed)
    buf, off, pr = _packed(seed)
    n = b.n
    a = aligners()
    a.set_reference(b.amp)
    if known:
        a.set_known(b.hdr)
    ob1, ob2 = a.align_dual_packed(pr, b.hdr)
    assert a.reference == b.amp
    # (the dual call's counters are its amplicon pass's; HDR copies are known copies there)
    _assert_none_certified(a, seed, b.amp, b.hdr, path, ("dual", seed, chunk))
    _assert_oracle(seed, b.amp, buf, off, ob1, ("dual call, amplicon pass", seed, chunk, path, known))
    _assert_oracle(seed, b.hdr, buf, off, ob2, ("dual call, HDR pass", seed, chunk, path, known))
    d1 = (ob1.stats.copy(), ob1.ops_off.copy(), ob1.ops.copy())
    d2 = (ob2.stats.copy(), ob2.ops_off.copy(), ob2.ops.copy())

    def same(ob, d, what):
        assert every_read_records(ob.stats[:n], d[0][:n]) == 0, what
        assert np.array_equal(ob.ops_off[:n + 1], d[1][:n + 1]), what
        assert np.array_equal(ob.ops[:int(d[1][n])], d[2][:int(d[1][n])]), what

    # the records-only form (the HDR pass's runs stay on the device)
    ob3, ob4 = a.align_dual_packed(pr, b.hdr, records_only2=True)
    same(ob3, d1, "records-only form, amplicon pass")
    assert not ob4.has_runs and every_read_records(ob4.stats[:n], d2[0][:n]) == 0
    assert np.array_equal(ob4.ops_off[:n + 1], d2[1][:n + 1])
    # two separate calls
    s1 = a.align_ops_packed(pr)
    _assert_none_certified(a, seed, b.amp, b.hdr if known else None, path, ("separate amplicon call", seed, chunk))
    same(s1, d1, "separate call against the amplicon")
    a.set_known(None)
    a.set_reference(b.hdr)
    s2 = a.align_ops_packed(pr)
    _assert_none_certified(a, seed, b.hdr, None, path, ("separate HDR call", seed, chunk))
    same(s2, d2, "separate call against the HDR amplicon")
