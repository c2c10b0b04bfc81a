"""Pooled amplicon mode: assign reads to their amplicons on the GPU, behind the C ABI of
``include/crispr_demux.h``.

CRISPRessoPooled's ``ONLY_AMPLICONS`` mode (CRISPResso/CRISPRessoPooledCORE.py:843-878) builds a
bowtie2 index of the amplicons, maps every read and splits the mapped reads into one
``AMPL_<name>.fastq.gz`` per amplicon.  Here the index, the assignment and the split run in HBM
(crispresso_amd/csrc/nw_demux.hip) by the exact window vote the header states; it is not bowtie2
(no MAPQ, no soft clipping, no genome), and a read the rule cannot place is reported as a tie or
as no hit, not guessed.

* :func:`demultiplex`         -- amplicons + reads -> :class:`DemuxResult`
* :func:`align_demultiplexed` -- the same, then :func:`crispresso_amd.pooled.align_pooled`
* :func:`align_demultiplexed_resident` -- assigned, grouped and 2-bit packed in HBM, each group
  adopted by the aligner where it lies; only decisions, records and runs cross PCIe
* :func:`summarize_pooled` -- raw reads (host, or merged pairs resident in HBM) to the reference's
  ``SAMPLES_QUANTIFICATION_SUMMARY.txt``: the identity filter and the counts on the device
  (``include/crispr_summary.h``, crispresso_amd/csrc/nw_summary.hip), 16 integers back per amplicon;
  with ``allow_hdr`` the rows' ``Expected_HDR`` amplicons by a second alignment per group
* :func:`read_amplicons_file` -- the reference's tab-separated amplicon table
* ``python -m crispresso_amd.demux`` -- FASTQ (``-r2``: pairs) + amplicon table -> per-amplicon
  FASTQ files, the reference's ``REPORT_READS_ALIGNED_TO_AMPLICONS.txt`` and, with ``--summary``
  (``--hdr``: the ``Expected_HDR`` column used), the summary table

Every refusal is made here, before any GPU call.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import gzip
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import NWD_NO_HIT, NWD_TIE, NativeLibraryError
from .aligner import pack_reads

MIN_K, MAX_K = 8, 31
MAX_AMPLICONS, MAX_AMPLICON_BASES, MAX_READ = 65535, 1 << 24, 4096
PHASES = ("assign", "upload_wall", "index", "gather")
REPORT_COLUMNS = ("Name", "Amplicon_Sequence", "sgRNA", "Expected_HDR", "Coding_sequence",
                  "Demultiplexed_fastq.gz_filename", "n_reads", "n_reads_aligned_%")
REASONS = {NWD_TIE: "tie", NWD_NO_HIT: "no_hit"}
_VALID_FILENAME_CHARS = set("+-_.() abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789")
_COMPLEMENT = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    _COMPLEMENT[_a] = _b


class DemuxError(RuntimeError):
    """A failed demultiplexing call."""


def check_params(k, min_hits) -> Tuple[int, int]:
    k, min_hits = int(k), int(min_hits)
    if not MIN_K <= k <= MAX_K:
        raise ValueError(f"window length {k}: {MIN_K} to {MAX_K} are supported")
    if min_hits < 1:
        raise ValueError(f"min_hits {min_hits}: at least 1")
    return k, min_hits


def check_offsets(buf: np.ndarray, offsets: np.ndarray, what: str, longest: Optional[int] = None) -> None:
    if offsets.ndim != 1 or len(offsets) < 1:
        raise ValueError(f"{what} offsets must hold n + 1 values")
    lens = np.diff(offsets)
    if len(lens) and bool((lens < 0).any()):
        raise ValueError(f"{what} offsets do not ascend")
    if int(offsets[0]) < 0 or int(offsets[-1]) > len(buf):
        raise ValueError(f"{what} offsets point outside the text")
    if longest is not None and len(lens) and int(lens.max()) > longest:
        raise ValueError(f"a {what[:-1]} of {int(lens.max())} bases: at most {longest} are supported")


def _packed(seqs) -> Tuple[np.ndarray, np.ndarray]:
    if isinstance(seqs, tuple) and len(seqs) == 2 and isinstance(seqs[0], np.ndarray):
        return np.ascontiguousarray(seqs[0], dtype=np.uint8), np.ascontiguousarray(seqs[1], dtype=np.int64)
    return pack_reads(list(seqs))


def pack_amplicons(amplicons) -> Tuple[np.ndarray, np.ndarray]:
    """The amplicons as bytes + offsets, refused outside the index's limits."""
    buf, off = _packed(amplicons)
    check_offsets(buf, off, "amplicons")
    n = len(off) - 1
    if not 1 <= n <= MAX_AMPLICONS:
        raise ValueError(f"{n} amplicons: 1 to {MAX_AMPLICONS} are supported")
    if int(off[-1] - off[0]) > MAX_AMPLICON_BASES:
        raise ValueError(f"{int(off[-1] - off[0])} amplicon bases: at most {MAX_AMPLICON_BASES} are supported")
    return buf, off


def reverse_complement(seq: bytes) -> bytes:
    """A<->T C<->G a<->t c<->g, every other byte unchanged, reversed (the gather kernel's rule)."""
    return _COMPLEMENT[np.frombuffer(seq, np.uint8)[::-1]].tobytes()


@dataclass
class DemuxResult:
    """One :func:`demultiplex` call: the per-read decisions and the gathered, oriented reads."""

    which: np.ndarray                  # int32 [n]: amplicon index, NWD_NO_HIT (-1) or NWD_TIE (-2)
    strand: np.ndarray                 # uint8 [n]: 1 = the read is the amplicon's reverse complement
    votes: np.ndarray                  # int32 [n]: best
    rival: np.ndarray                  # int32 [n]
    counts: np.ndarray                 # int64 [amplicons]
    group_offsets: np.ndarray          # int64 [amplicons + 1] into order / text_offsets
    order: np.ndarray                  # int64 [n_assigned]: input index of each gathered read
    text: np.ndarray                   # uint8: the gathered bytes, strand-1 reads reverse-complemented
    text_offsets: np.ndarray           # int64 [n_assigned + 1]
    n_windows: int
    n_ambiguous: int
    n_tie: int = 0
    n_no_hit: int = 0
    fallback: int = 0
    kernel_ms: float = 0.0
    upload_ms: float = 0.0

    @property
    def n_assigned(self) -> int:
        return int(len(self.order))

    def reads_per_amplicon(self) -> List[Tuple[np.ndarray, np.ndarray]]:
        """One packed ``(buf, offsets)`` per amplicon, already oriented: what
        :func:`crispresso_amd.pooled.align_pooled` takes."""
        out = []
        for g in range(len(self.counts)):
            lo, hi = int(self.group_offsets[g]), int(self.group_offsets[g + 1])
            t0, t1 = int(self.text_offsets[lo]), int(self.text_offsets[hi])
            out.append((self.text[t0:t1], self.text_offsets[lo:hi + 1] - t0))
        return out


@dataclass
class PackedGroups:
    """One :meth:`GpuDemultiplexer.pack`: where the grouped reads lie in the packed batch in HBM."""

    group_offsets: np.ndarray          # int64 [amplicons + 1]
    order: np.ndarray                  # int64 [n_assigned]
    text_offsets: np.ndarray           # int64 [n_assigned + 1]: gathered coordinates
    lens: np.ndarray                   # uint16 [n_assigned]
    group_exc: np.ndarray              # int64 [amplicons + 1]: group g's slots of the exception list
    n_exc: int
    kernel_ms: float


class GpuDemultiplexer:
    """One ``nwd_ctx`` (one GPU), reusable across calls and amplicon sets.  Not thread-safe."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        ctx = ctypes.c_void_p()
        rc = self._lib.nwd_create(int(device), ctypes.byref(ctx))
        if rc != 0:
            raise NativeLibraryError(f"nwd_create(device={device}) failed with code {rc} (no GPU?)")
        self._ctx = ctx
        self.device = device
        self.n_amplicons = 0
        self.n_windows = self.n_ambiguous = 0
        self._packed: Optional[PackedGroups] = None

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.nwd_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            msg = self._lib.nwd_last_error(self._ctx).decode(errors="replace")
            raise DemuxError(f"{what} failed ({rc}): {msg}")

    def phase_times(self) -> Dict[str, float]:
        ms = np.zeros(4, np.float32)
        self._lib.nwd_phase_times(self._ctx, _lib.ptr(ms))
        return dict(zip(PHASES, (float(x) for x in ms)))

    def last_fallback(self) -> int:
        return int(self._lib.nwd_last_fallback(self._ctx))

    def set_amplicons(self, buf: np.ndarray, offsets: np.ndarray, k: int) -> Tuple[int, int]:
        nw, na = ctypes.c_int64(), ctypes.c_int64()
        n = len(offsets) - 1
        self._packed = None
        self._check(self._lib.nwd_set_amplicons(self._ctx, _lib.ptr(buf), _lib.ptr(offsets), n, k, ctypes.byref(nw),
                                                ctypes.byref(na)), "nwd_set_amplicons")
        self.n_amplicons, self.n_windows, self.n_ambiguous = n, int(nw.value), int(na.value)
        return self.n_windows, self.n_ambiguous

    def assign(self, buf: np.ndarray, offsets: np.ndarray, min_hits: int, both_strands: bool):
        n = len(offsets) - 1
        which, strand = np.empty(n, np.int32), np.empty(n, np.uint8)
        votes, rival = np.empty(n, np.int32), np.empty(n, np.int32)
        counts = np.zeros(self.n_amplicons, np.int64)
        na, nt, nn = (ctypes.c_int64() for _ in range(3))
        ms = ctypes.c_float()
        self._packed = None
        self._check(self._lib.nwd_assign(self._ctx, _lib.ptr(buf), _lib.ptr(offsets), n, min_hits, int(bool(both_strands)),
                                         _lib.ptr(which), _lib.ptr(strand), _lib.ptr(votes), _lib.ptr(rival),
                                         _lib.ptr(counts), ctypes.byref(na), ctypes.byref(nt), ctypes.byref(nn),
                                         ctypes.byref(ms)), "nwd_assign")
        return which, strand, votes, rival, counts, int(na.value), int(nt.value), int(nn.value), float(ms.value)

    def assign_prepared(self, rr, min_hits: int, both_strands: bool):
        """:meth:`assign` on the merged reads a front-end call left in HBM (``rr``: a
        :class:`crispresso_amd.frontend.ResidentReads`; ``nwd_assign_prepared``): no upload, the
        same return.  ``rr`` may be closed right after."""
        n = len(rr)
        which, strand = np.empty(n, np.int32), np.empty(n, np.uint8)
        votes, rival = np.empty(n, np.int32), np.empty(n, np.int32)
        counts = np.zeros(self.n_amplicons, np.int64)
        na, nt, nn = (ctypes.c_int64() for _ in range(3))
        ms = ctypes.c_float()
        self._packed = None
        self._check(self._lib.nwd_assign_prepared(self._ctx, ctypes.byref(rr.result()), min_hits, int(bool(both_strands)),
                                                  _lib.ptr(which), _lib.ptr(strand), _lib.ptr(votes), _lib.ptr(rival),
                                                  _lib.ptr(counts), ctypes.byref(na), ctypes.byref(nt),
                                                  ctypes.byref(nn), ctypes.byref(ms)), "nwd_assign_prepared")
        return which, strand, votes, rival, counts, int(na.value), int(nt.value), int(nn.value), float(ms.value)

    def gather(self, n_assigned: int, text_cap: int):
        """(group_offsets, order, text, text_offsets) of the last :meth:`assign`; a short
        ``text_cap`` is answered with the needed size, and the call is made again."""
        goff = np.zeros(self.n_amplicons + 1, np.int64)
        order = np.empty(n_assigned, np.int64)
        toff = np.zeros(n_assigned + 1, np.int64)
        need = ctypes.c_int64()
        text = np.empty(max(text_cap, 1), np.uint8)
        rc = self._lib.nwd_gather(self._ctx, _lib.ptr(goff), _lib.ptr(order), _lib.ptr(text), _lib.ptr(toff), text_cap,
                                  ctypes.byref(need))
        if rc == _lib.NW_E_CAPACITY:
            text_cap = int(need.value)
            text = np.empty(max(text_cap, 1), np.uint8)
            rc = self._lib.nwd_gather(self._ctx, _lib.ptr(goff), _lib.ptr(order), _lib.ptr(text), _lib.ptr(toff),
                                      text_cap, ctypes.byref(need))
        self._check(rc, "nwd_gather")
        return goff, order, text[:int(need.value)], toff

    def pack(self, n_assigned: int) -> "PackedGroups":
        """The grouped reads of the last :meth:`assign` 2-bit packed in HBM (``nwd_pack``): the
        index arrays :meth:`gather` gives, the lengths and each group's slice of the exception
        list.  The gathered text is not made; nothing but these small arrays crosses PCIe."""
        goff = np.zeros(self.n_amplicons + 1, np.int64)
        order = np.empty(n_assigned, np.int64)
        toff = np.zeros(n_assigned + 1, np.int64)
        lens = np.empty(n_assigned, np.uint16)
        gexc = np.zeros(self.n_amplicons + 1, np.int64)
        ne, ms = ctypes.c_int64(), ctypes.c_float()
        self._check(self._lib.nwd_pack(self._ctx, _lib.ptr(goff), _lib.ptr(order), _lib.ptr(toff), _lib.ptr(lens),
                                       _lib.ptr(gexc), ctypes.byref(ne), ctypes.byref(ms)), "nwd_pack")
        self._packed = PackedGroups(goff, order, toff, lens, gexc, int(ne.value), float(ms.value))
        return self._packed

    def fetch_packed(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(packed, exc_pos, exc_byte) of the last :meth:`pack`, copied to the host (for tests)."""
        pk = self._packed
        if pk is None:
            raise DemuxError("fetch_packed before pack")
        nbytes = (int(pk.text_offsets[-1]) + 3) // 4
        packed = np.zeros(max(nbytes, 1), np.uint8)
        pos, byt = np.empty(pk.n_exc, np.int64), np.empty(pk.n_exc, np.uint8)
        self._check(self._lib.nwd_fetch_packed(self._ctx, _lib.ptr(packed), nbytes, _lib.ptr(pos), _lib.ptr(byt), None),
                    "nwd_fetch_packed")
        return packed[:nbytes], pos, byt

    def adopt(self, aligner, g: int) -> int:
        """Make group ``g`` of the last :meth:`pack` the resident batch of ``aligner`` (ops output,
        its reference set): ``nwd_adopt_group``.  Returns the group's number of reads."""
        self._check(self._lib.nwd_adopt_group(self._ctx, aligner._h, int(g)), "nwd_adopt_group")
        pk = self._packed
        lo, hi = int(pk.group_offsets[g]), int(pk.group_offsets[g + 1])
        aligner.adopted(None, pk.text_offsets[lo:hi + 1])
        return hi - lo


_DEFAULT: Dict[int, GpuDemultiplexer] = {}


def default_demultiplexer(device: int = 0) -> GpuDemultiplexer:
    d = _DEFAULT.get(device)
    if d is None:
        d = _DEFAULT[device] = GpuDemultiplexer(device)
    return d


def demultiplex(amplicons, reads, *, k: int = 16, min_hits: int = 2, both_strands: bool = True,
                demultiplexer: Optional[GpuDemultiplexer] = None) -> DemuxResult:
    """Assign every read to the amplicon its length-``k`` windows vote for (the rule of
    ``include/crispr_demux.h``) and gather the assigned reads per amplicon, oriented.

    ``amplicons``: a list of ``str``; ``reads``: a list of ``str`` or the packed
    ``(buf, offsets)`` pair (uint8 bytes, int64 offsets)."""
    k, min_hits = check_params(k, min_hits)
    abuf, aoff = pack_amplicons(amplicons)
    rbuf, roff = _packed(reads)
    check_offsets(rbuf, roff, "reads", MAX_READ)
    if len(roff) - 1 > 2 ** 31 - 1:
        raise ValueError("more than 2^31 - 1 reads")
    d = demultiplexer or default_demultiplexer()
    n_windows, n_ambiguous = d.set_amplicons(abuf, aoff, k)
    which, strand, votes, rival, counts, na, nt, nn, ms = d.assign(rbuf, roff, min_hits, both_strands)
    lens = np.diff(roff)
    goff, order, text, toff = d.gather(na, int(lens[which >= 0].sum()))
    times = d.phase_times()
    return DemuxResult(which, strand, votes, rival, counts, goff, order, text, toff, n_windows, n_ambiguous, nt, nn,
                       d.last_fallback(), ms, times["upload_wall"])


def align_demultiplexed(amplicons: Sequence[str], reads, aligner, *, min_reads: int = 0, **kw):
    """:func:`demultiplex`, then :func:`crispresso_amd.pooled.align_pooled` on the amplicons with
    more than ``min_reads`` reads (strictly more, as CRISPRessoPooledCORE.py:894).

    Returns ``(batches, result, skipped)``: one batch per amplicon (``None`` for a skipped one),
    the :class:`DemuxResult`, and the indices of the skipped amplicons."""
    from .pooled import align_pooled

    res = demultiplex(amplicons, reads, **kw)
    groups = res.reads_per_amplicon()
    keep = [g for g in range(len(amplicons)) if int(res.counts[g]) > min_reads]
    skipped = [g for g in range(len(amplicons)) if int(res.counts[g]) <= min_reads]
    batches: list = [None] * len(amplicons)
    if keep:
        for g, b in zip(keep, align_pooled([amplicons[g] for g in keep], [groups[g] for g in keep], aligner)):
            batches[g] = b
    return batches, res, skipped


def align_demultiplexed_resident(amplicons: Sequence[str], reads, aligner, *, min_reads: int = 0, on_group=None,
                                 with_text: bool = False, k: int = 16, min_hits: int = 2, both_strands: bool = True,
                                 demultiplexer: Optional[GpuDemultiplexer] = None):
    """:func:`align_demultiplexed` without the round trip: the reads are uploaded once, assigned,
    oriented, grouped and 2-bit packed in HBM (``nwd_pack``), and each amplicon's group is adopted
    by ``aligner`` where it lies (``nwd_adopt_group``) and aligned there.  Only the decisions,
    the records and the runs cross PCIe.

    For every amplicon with more than ``min_reads`` reads (strictly), in index order:
    ``set_reference``, adoption, one synchronised pass, ``on_group(g, aligner, n)`` while the
    group is resident (the place for ``quantify.run_device_ops`` or ``alleles.allele_table`` on
    ``aligner.device_ops()``), ``download_ops``.

    Returns ``(ops_batches, result, skipped)``: one :class:`~crispresso_amd.aligner.OpsBatch` per
    amplicon (``None`` for a skipped one; ``OpsBatch.expand(amplicons[g], text, offsets)`` on the
    group's text gives :func:`align_demultiplexed`'s rows), the :class:`DemuxResult` (``text``
    filled only with ``with_text``, by ``nwd_gather``) and the skipped indices.  ``aligner`` must
    be on the demultiplexer's device; its output mode is ops during the call and restored after."""
    k, min_hits = check_params(k, min_hits)
    abuf, aoff = pack_amplicons(amplicons)
    rbuf, roff = _packed(reads)
    check_offsets(rbuf, roff, "reads", MAX_READ)
    if len(roff) - 1 > 2 ** 31 - 1:
        raise ValueError("more than 2^31 - 1 reads")
    d = demultiplexer or default_demultiplexer(getattr(aligner, "device", 0))
    n_windows, n_ambiguous = d.set_amplicons(abuf, aoff, k)
    which, strand, votes, rival, counts, na, nt, nn, ms = d.assign(rbuf, roff, min_hits, both_strands)
    pk = d.pack(na)
    if with_text:
        _, _, text, _ = d.gather(na, int(pk.text_offsets[-1]))
    else:
        text = np.zeros(0, np.uint8)
    res = DemuxResult(which, strand, votes, rival, counts, pk.group_offsets, pk.order, text, pk.text_offsets,
                      n_windows, n_ambiguous, nt, nn, d.last_fallback(), ms, d.phase_times()["upload_wall"])
    min_reads = max(int(min_reads), 0)      # (an amplicon without a read has nothing to adopt)
    keep = [g for g in range(len(amplicons)) if int(counts[g]) > min_reads]
    skipped = [g for g in range(len(amplicons)) if int(counts[g]) <= min_reads]
    batches: list = [None] * len(amplicons)
    mode = getattr(aligner, "output_mode", "rows")
    aligner.set_output("ops")
    try:
        for g in keep:
            aligner.set_reference(amplicons[g])
            n = d.adopt(aligner, g)
            aligner.run_async()
            aligner.sync()
            if on_group is not None:
                on_group(g, aligner, n)
            batches[g] = aligner.download_ops(n)
    finally:
        aligner.set_output(mode)
    return batches, res, skipped


# ---- raw reads to the per-amplicon summary ------------------------------------------------------

SUMMARY_COLUMNS = ("Name", "Unmodified%", "NHEJ%", "HDR%", "Mixed_HDR-NHEJ%", "Reads_aligned", "Reads_total")
MAX_QUANT_AMPLICON = 32768          # nwq_params.len_amplicon must stay below it


class SummaryError(RuntimeError):
    """A failed nws_* call; ``code`` is its return, ``n_out_of_range`` what nws_flags counted."""

    def __init__(self, msg: str, code: int, n_out_of_range: int = 0):
        super().__init__(msg)
        self.code, self.n_out_of_range = code, n_out_of_range


def _first_at_least(L: int, bound, strict: bool) -> int:
    """The smallest i in [0, L] with printed_percent(i, L) > bound (strict) or >= bound; L + 1 if
    none.  The printed value does not decrease with i: a bisection."""
    from .aligner import printed_percent

    def ok(i: int) -> bool:
        v = printed_percent(i, L)
        return v > bound if strict else v >= bound

    if not ok(L):
        return L + 1
    lo, hi = 0, L                   # ok(hi); the answer lies in [lo, hi]
    while lo < hi:
        mid = (lo + hi) >> 1
        if ok(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


def identity_thresholds(min_identity_score: float, max_cols: int, start: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The tables ``nws_set_identity`` takes, int32 ``[max_cols + 1]`` indexed by the alignment
    length L (entries below ``start`` are left 0, for a caller that extends its tables):

    * ``keep_min[L]``: the smallest ``n_ident`` whose printed identity
      ``float("%.1f" % (100.0 * n_ident / L))`` is strictly greater than ``min_identity_score``
      (the reference's filter, CRISPRessoCORE.py:1997-2012), ``L + 1`` if none is;
    * ``unmod_min[L]``: the smallest ``n_ident`` that prints ``100.0`` (UNMODIFIED, CORE:2014).

    The reference compares what it printed, not the ratio: 150/250 prints 60.0 and is dropped
    at 60, and from L = 2000 on a read with one mismatch prints 100.0."""
    max_cols = int(max_cols)
    if max_cols < 0:
        raise ValueError("max_cols must not be negative")
    keep_min, unmod_min = np.zeros(max_cols + 1, np.int32), np.zeros(max_cols + 1, np.int32)
    bound = float(min_identity_score)
    for L in range(max(int(start), 0), max_cols + 1):
        keep_min[L] = _first_at_least(L, bound, True)
        unmod_min[L] = _first_at_least(L, 100.0, False)
    return keep_min, unmod_min


def printed_tables(min_identity_score: float, threshold: float = 98.0) -> Tuple[np.ndarray, int, int]:
    """The host values ``nws_set_printed`` takes, ``(tie_up, keep_tenths, hdr_tenths)``:

    * ``tie_up`` uint8 [1000]: ``tie_up[t]`` is 1 iff an identity on the rounding midpoint between
      ``t`` and ``t + 1`` tenths prints ``t + 1``.  There ``100.0 * n / L`` is the correctly rounded
      double of ``(2 t + 1) / 20`` whatever ``n`` and ``L`` are, so ``printed_percent(2 t + 1, 2000)``
      decides for all of them;
    * ``keep_tenths``: the smallest ``t`` in 0..1000 with ``t / 10.0 > min_identity_score``
      (CRISPRessoCORE.py:1849-1852), 1001 if none;
    * ``hdr_tenths``: the smallest ``t`` with ``t / 10.0 >= threshold`` (CORE:536-548), 1001 if none.

    ``float("%.1f" % x)`` is ``t / 10.0`` for the ``t`` it prints, so comparing tenths is comparing
    what the reference compares."""
    from .aligner import printed_percent

    tie_up = np.zeros(1000, np.uint8)
    for t in range(1000):
        v = printed_percent(2 * t + 1, 2000)
        if v == (t + 1) / 10.0:
            tie_up[t] = 1
        elif v != t / 10.0:
            raise AssertionError(f"the midpoint above {t} tenths prints {v!r}")
    score, bound = float(min_identity_score), float(threshold)
    keep_tenths = next((t for t in range(1001) if t / 10.0 > score), 1001)
    hdr_tenths = next((t for t in range(1001) if t / 10.0 >= bound), 1001)
    return tie_up, keep_tenths, hdr_tenths


class GpuSummarizer:
    """One ``nws_ctx`` (one GPU): the flags and the 16 counters of a resident group
    (``include/crispr_summary.h``).  Not thread-safe."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        ctx = ctypes.c_void_p()
        rc = self._lib.nws_create(int(device), ctypes.byref(ctx))
        if rc != 0:
            raise NativeLibraryError(f"nws_create(device={device}) failed with code {rc} (no GPU?)")
        self._ctx = ctx
        self.device = device
        self.min_identity_score: Optional[float] = None
        self.keep_min = self.unmod_min = np.zeros(0, np.int32)
        self.flags_ms = self.summary_ms = 0.0
        self.printed_key: Optional[Tuple[float, float]] = None     # (min_identity_score, threshold) of set_printed
        self.printed_ms = 0.0
        self.mask_ms = self.histograms_ms = 0.0

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.nws_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str, bad: int = 0) -> None:
        if rc != 0:
            msg = self._lib.nws_last_error(self._ctx).decode(errors="replace")
            raise SummaryError(f"{what} failed ({rc}): {msg}", rc, bad)

    def set_identity(self, keep_min: np.ndarray, unmod_min: np.ndarray) -> None:
        keep_min = np.ascontiguousarray(keep_min, np.int32)
        unmod_min = np.ascontiguousarray(unmod_min, np.int32)
        if keep_min.ndim != 1 or keep_min.shape != unmod_min.shape or len(keep_min) < 1:
            raise ValueError("the two tables must hold max_cols + 1 values each")
        self._check(self._lib.nws_set_identity(self._ctx, _lib.ptr(keep_min), _lib.ptr(unmod_min), len(keep_min) - 1),
                    "nws_set_identity")
        self.keep_min, self.unmod_min = keep_min, unmod_min

    def ensure_identity(self, min_identity_score: float, max_cols: int) -> None:
        """Tables for ``min_identity_score`` that reach ``max_cols``: built once, extended when a
        later group's alignments are longer."""
        score = float(min_identity_score)
        have = len(self.keep_min) - 1 if self.min_identity_score == score else -1
        if have >= max_cols:
            return
        keep_min, unmod_min = identity_thresholds(score, max_cols, have + 1)
        keep_min[:have + 1], unmod_min[:have + 1] = self.keep_min[:have + 1], self.unmod_min[:have + 1]
        self.min_identity_score = None
        self.set_identity(keep_min, unmod_min)
        self.min_identity_score = score

    def flags(self, d_stats: int, n: int, d_pre: int, d_keep: int) -> None:
        """``nws_flags``: device pointers (ints) of n nw_stat records in, pre and keep (uint8 [n])
        out.  A record outside the tables raises :class:`SummaryError` with their number."""
        bad, ms = ctypes.c_int64(), ctypes.c_float()
        rc = self._lib.nws_flags(self._ctx, d_stats, n, d_pre, d_keep, ctypes.byref(bad), ctypes.byref(ms))
        self.flags_ms = float(ms.value)
        self._check(rc, "nws_flags", int(bad.value))

    def set_printed(self, tie_up: np.ndarray, keep_tenths: int, hdr_tenths: int) -> None:
        """``nws_set_printed``: the values of :func:`printed_tables`."""
        tie_up = np.ascontiguousarray(tie_up, np.uint8)
        if tie_up.shape != (1000,):
            raise ValueError("tie_up must hold 1000 values")
        self.printed_key = None
        self._check(self._lib.nws_set_printed(self._ctx, _lib.ptr(tie_up), int(keep_tenths), int(hdr_tenths)),
                    "nws_set_printed")

    def ensure_printed(self, min_identity_score: float, threshold: float) -> None:
        """The printed-identity values for this score and threshold, built once."""
        key = (float(min_identity_score), float(threshold))
        if self.printed_key != key:
            self.set_printed(*printed_tables(*key))
            self.printed_key = key

    def printed(self, d_stats: int, n: int, d_tenths: int) -> None:
        """``nws_printed``: n nw_stat records in, their printed identities in tenths (uint16 [n])
        out.  A record out of range raises :class:`SummaryError` with their number."""
        bad, ms = ctypes.c_int64(), ctypes.c_float()
        rc = self._lib.nws_printed(self._ctx, d_stats, n, d_tenths, ctypes.byref(bad), ctypes.byref(ms))
        self.printed_ms = float(ms.value)
        self._check(rc, "nws_printed", int(bad.value))

    def flags_dual(self, d_stats_ref: int, d_tenths_rep: int, n: int, d_pre: int, d_keep: int) -> None:
        """``nws_flags_dual``: the amplicon pass's records and the Expected_HDR pass's tenths in,
        pre (UNMODIFIED, HDR, MIXED) and keep (uint8 [n]) out."""
        bad, ms = ctypes.c_int64(), ctypes.c_float()
        rc = self._lib.nws_flags_dual(self._ctx, d_stats_ref, d_tenths_rep, n, d_pre, d_keep, ctypes.byref(bad),
                                      ctypes.byref(ms))
        self.flags_ms = float(ms.value)
        self._check(rc, "nws_flags_dual", int(bad.value))

    def summary(self, d_reads: int, d_pre: int, d_keep: int, n: int) -> np.ndarray:
        """``nws_summary``: the 16 slots (int64) of n nwq_read records on the device."""
        out = np.zeros(_lib.NWS_SLOTS, np.int64)
        ms = ctypes.c_float()
        rc = self._lib.nws_summary(self._ctx, d_reads, d_pre, d_keep, n, _lib.ptr(out), ctypes.byref(ms))
        self.summary_ms = float(ms.value)
        self._check(rc, "nws_summary")
        return out

    def mask_pre(self, d_pre: int, d_keep: int, n: int, d_pre_q: int) -> None:
        """``nws_mask_pre``: ``pre`` with every dropped read's byte set to UNMODIFIED, for the
        quantifier (uint8 [n] on the device; ``d_pre_q`` may be ``d_pre``)."""
        ms = ctypes.c_float()
        rc = self._lib.nws_mask_pre(self._ctx, d_pre, d_keep, n, d_pre_q, ctypes.byref(ms))
        self.mask_ms = float(ms.value)
        self._check(rc, "nws_mask_pre")

    def histograms(self, d_reads: int, d_keep: int, n: int, bins: int):
        """``nws_histograms``: ``(ins, del, mut, indel)`` of the kept reads of n nwq_read records
        on the device, int64 ``[bins]`` each and ``[2 bins - 1]``.  A counted read with a size
        outside ``[0, bins)`` raises :class:`SummaryError` with their number."""
        bins = int(bins)
        out = np.zeros(max(5 * bins - 1, 1), np.int64)
        bad, ms = ctypes.c_int64(), ctypes.c_float()
        rc = self._lib.nws_histograms(self._ctx, d_reads, d_keep, n, bins, _lib.ptr(out), ctypes.byref(bad),
                                      ctypes.byref(ms))
        self.histograms_ms = float(ms.value)
        self._check(rc, "nws_histograms", int(bad.value))
        return out[:bins], out[bins:2 * bins], out[2 * bins:3 * bins], out[3 * bins:]


_DEFAULT_SUMMARIZER: Dict[int, GpuSummarizer] = {}


def default_summarizer(device: int = 0) -> GpuSummarizer:
    s = _DEFAULT_SUMMARIZER.get(device)
    if s is None:
        s = _DEFAULT_SUMMARIZER[device] = GpuSummarizer(device)
    return s


@dataclass
class PooledSummary:
    """One :func:`summarize_pooled` call."""

    counts: np.ndarray                 # int64 [amplicons, 16]: nws_summary's slots, zeros for a skipped amplicon
    frame: "object"                    # pandas.DataFrame: SAMPLES_QUANTIFICATION_SUMMARY.txt's rows
    result: DemuxResult
    skipped: List[int]
    kernel_ms: Dict[str, float]        # device ms of the flags, summary, quantify and printed kernels, summed over the
                                       # groups, and hdr_pass: the host's wall ms of the Expected_HDR passes


def summary_frame(names: Sequence[str], counts: np.ndarray, n_reads: Sequence[int], skipped: Sequence[int]):
    """The table of CRISPRessoPooledCORE.py:1382-1413 from the 16 slots per amplicon: the shares
    of N_TOTAL (a float, as the reference parses it) times 100, NaN throughout for an amplicon
    that was skipped or has no read aligned (the reference finds no quantification file)."""
    import pandas as pd

    rows = []
    skipped = set(int(g) for g in skipped)
    for g, name in enumerate(names):
        c = counts[g]
        N_TOTAL = float(c[1])
        if g in skipped or N_TOTAL == 0:
            rows.append([name, np.nan, np.nan, np.nan, np.nan, np.nan, int(n_reads[g])])
            continue
        N_UNMODIFIED, N_MODIFIED, N_REPAIRED, N_MIXED_HDR_NHEJ = (float(c[s]) for s in (2, 3, 4, 5))
        rows.append([name, N_UNMODIFIED / N_TOTAL * 100., N_MODIFIED / N_TOTAL * 100., N_REPAIRED / N_TOTAL * 100.,
                     N_MIXED_HDR_NHEJ / N_TOTAL * 100., N_TOTAL, int(n_reads[g])])
    return pd.DataFrame(rows, columns=list(SUMMARY_COLUMNS))


def write_summary(path: str, frame) -> None:
    """SAMPLES_QUANTIFICATION_SUMMARY.txt as the reference writes it (POOLED:1414-1416)."""
    frame.fillna("NA").to_csv(path, sep="\t", index=None)


MAX_ALIGNER_REFERENCE = 8192        # nw_set_reference's limit (include/crispr_nw.h)


def checked_expected_hdr(row: dict, amplicon: str, what: str = "amplicon") -> Optional[str]:
    """The row's ``Expected_HDR`` after the reference's checks (CRISPRessoCORE.py:1349-1364):
    stripped and upper-cased; ``None`` when empty.  Equal to the amplicon, a byte outside
    ``ATCGN`` or more bases than the aligner takes raise ``ValueError`` naming the row.  The
    reference's ``pairwise2.globalxx`` identity of the two (CORE:1366-1382) is not checked."""
    hdr = str(row.get("Expected_HDR") or "").strip().upper()
    if not hdr:
        return None
    if hdr == amplicon:
        raise ValueError(f"{what} {row['Name']}: the amplicon sequence expected after an HDR and the reference "
                         "amplicon cannot be the same")
    wrong = sorted(set(hdr) - set("ATCGN"))
    if wrong:
        raise ValueError(f"{what} {row['Name']}: the amplicon sequence expected after an HDR contains wrong "
                         "characters:%s" % " ".join(wrong))
    if len(hdr) > MAX_ALIGNER_REFERENCE:
        raise ValueError(f"{what} {row['Name']}: Expected_HDR has {len(hdr)} bases: at most {MAX_ALIGNER_REFERENCE} "
                         "are supported by the aligner")
    return hdr


def check_summary_rows(rows: Sequence[dict], allow_hdr: bool = False) -> List[str]:
    """The refusals :func:`summarize_pooled` makes on the amplicon table, before any GPU call;
    returns the amplicon sequences.  An ``Expected_HDR`` row is refused unless ``allow_hdr``, and
    with it goes through :func:`checked_expected_hdr`."""
    for row in rows:
        if row.get("Expected_HDR"):
            if not allow_hdr:
                raise ValueError(f"amplicon {row['Name']}: Expected_HDR is given, and dual alignment per amplicon is not built")
            checked_expected_hdr(row, row["Amplicon_Sequence"])
        if len(row["Amplicon_Sequence"]) >= MAX_QUANT_AMPLICON:
            raise ValueError(f"amplicon {row['Name']} has {len(row['Amplicon_Sequence'])} bases: fewer than "
                             f"{MAX_QUANT_AMPLICON} are supported")
    return [row["Amplicon_Sequence"] for row in rows]


def _summarize_groups(rows, amplicons, keep, most, prepare, aligner, q, s, out, what, min_identity_score, quant_kw,
                      on_group, hdrs=None, hdr_threshold: float = 98.0, reports=None, alleles: bool = False,
                      offset_around_cut: int = 20) -> Dict[str, float]:
    """The per-group body of :func:`summarize_pooled` and of
    :func:`crispresso_amd.regions.summarize_regions`: for every ``g`` in ``keep``, in that order,
    ``prepare(g, amplicons[g])`` (the caller's ``set_reference`` and adoption: the group's reads
    become the resident batch; returns their number, at most ``most``), one pass, ``nws_flags``,
    the quantifier on the resident ops with the device ``pre`` (globals from ``rows[g]`` and
    ``quant_kw``), ``nws_summary`` into ``out[g]``, the slot-15 check, ``on_group(g, aligner, n)``.

    A group with ``hdrs[g]`` (its checked Expected_HDR amplicon) is first prepared with that as
    the reference and aligned, and ``nws_printed`` keeps two bytes per read of that pass; then the
    body above runs with ``nws_flags_dual`` in place of ``nws_flags``.  The Expected_HDR pass goes
    first, so the ops the quantifier and ``on_group`` see are the amplicon pass's.

    With ``reports`` (a callable ``reports(g, GroupReport)``) the quantifier runs on
    ``nws_mask_pre`` of the flags, so that its totals hold the kept reads only as the reference's
    do (a dropped read's ``cls`` becomes 0, which no slot counts: the slots are the same either
    way); ``nws_summary`` still takes the flags themselves.  Then ``nws_histograms`` and the
    :class:`crispresso_amd.report.GroupReport`, handed over after ``on_group``.  The returned
    times gain ``mask`` and ``histograms``.  Without ``reports`` none of this runs.

    With ``alleles`` (needs ``reports``: :class:`ValueError` without) the report also gets the
    group's allele table and its tables around the cut sites (``offset_around_cut`` columns each
    side), made after ``nws_histograms`` from the resident ops, the keep flags and the
    ``nwq_read`` records where they lie (:func:`crispresso_amd.alleles.resident_allele_table`,
    :func:`crispresso_amd.alleles.resident_around_cut_tables`): no read's text reaches the host.
    The tables are upper case.  The returned times gain ``alleles`` and ``around_cut`` (the
    kernels' ms of ``nwa_table_device`` and ``nwa_windows_resident``; 0 for tables that took the
    host fallback) and ``alleles_wall`` / ``around_cut_wall`` (the host's wall ms, strings and
    frames included).  Without ``alleles`` no kernel more runs and no buffer more is allocated.

    Errors name the group as ``"<what> <Name>"``.  The aligner's output mode and the quantifier's
    module globals are restored.  Returns the summed kernel times (``flags``, ``summary``,
    ``quantify``, ``printed``) and ``hdr_pass``, the host's wall ms of the Expected_HDR passes."""
    import contextlib
    import time
    import types

    from . import quantify
    from .devmem import DeviceBuffer

    device = int(getattr(aligner, "device", 0))
    times = {"flags": 0.0, "summary": 0.0, "quantify": 0.0, "printed": 0.0, "hdr_pass": 0.0}
    mode = getattr(aligner, "output_mode", "rows")
    saved_globals = quantify._GLOBALS
    hdrs = hdrs or [None] * len(rows)
    if alleles and reports is None:
        raise ValueError("alleles=True fills the groups' reports: pass reports as well")
    if reports is not None:
        from .report import GroupReport, guide_cut_pairs

        times.update(mask=0.0, histograms=0.0)
    if alleles:
        from . import alleles as al_tables

        times.update(alleles=0.0, around_cut=0.0, alleles_wall=0.0, around_cut_wall=0.0)
        awidth = int(aligner.options.awidth)
        grouper = al_tables.default_grouper(device)
    most_hdr = max((2 * most for g in keep if hdrs[g]), default=0)
    aligner.set_output("ops")
    try:
        with DeviceBuffer(most, device) as d_pre, DeviceBuffer(most, device) as d_keep, \
                DeviceBuffer(16 * most, device) as d_out, DeviceBuffer(most_hdr, device) as d_rep, \
                (DeviceBuffer(most, device) if reports is not None else contextlib.nullcontext()) as d_pre_q:
            for g in keep:
                amp, row, hdr = amplicons[g], rows[g], hdrs[g]
                try:
                    if hdr:
                        t0 = time.perf_counter()
                        n = prepare(g, hdr)
                        aligner.run_async()
                        aligner.sync()
                        s.ensure_printed(min_identity_score, hdr_threshold)
                        s.printed(aligner.device_ops()["stats"], n, d_rep.ptr)
                        times["printed"] += s.printed_ms
                        times["hdr_pass"] += (time.perf_counter() - t0) * 1e3
                    n = prepare(g, amp)
                    aligner.run_async()
                    aligner.sync()
                    dev = aligner.device_ops()
                    if hdr:
                        s.flags_dual(dev["stats"], d_rep.ptr, n, d_pre.ptr, d_keep.ptr)
                    else:
                        s.ensure_identity(min_identity_score, int(dev["max_cols"]))
                        s.flags(dev["stats"], n, d_pre.ptr, d_keep.ptr)
                    if reports is not None:
                        s.mask_pre(d_pre.ptr, d_keep.ptr, n, d_pre_q.ptr)
                        times["mask"] += s.mask_ms
                except SummaryError as exc:
                    raise SummaryError(f"{what} {row['Name']}: {exc}", exc.code, exc.n_out_of_range) from None
                args = types.SimpleNamespace(
                    amplicon_seq=amp, guide_seq=row.get("sgRNA") or None, coding_seq=row.get("Coding_sequence") or None,
                    expected_hdr_amplicon_seq=hdr, hdr_perfect_alignment_threshold=hdr_threshold, **quant_kw)
                try:
                    q.set_params(quantify.globals_from_args(args), args, amplicon_has_n="N" in amp.upper())
                    totals = q.run_device_ops(amp, dev, d_pre.ptr if reports is None else d_pre_q.ptr, n, d_out.ptr)
                except quantify.QuantificationError as exc:     # (e.g. an amplicon too long for the quantifier's LDS)
                    raise quantify.QuantificationError(f"{what} {row['Name']}: {exc}") from None
                times["quantify"] += q.last_kernel_ms
                out[g] = s.summary(d_out.ptr, d_pre.ptr, d_keep.ptr, n)
                times["flags"] += s.flags_ms
                times["summary"] += s.summary_ms
                if int(out[g, 15]):
                    raise quantify.QuantificationError(
                        f"{what} {row['Name']}: {int(out[g, 15])} kept reads are not alignments of it "
                        "(LEN_AMPLICON bases)")
                if on_group is not None:
                    on_group(g, aligner, n)
                if reports is not None:
                    try:
                        hist = s.histograms(d_out.ptr, d_keep.ptr, n, int(dev["max_cols"]) + 1)
                    except SummaryError as exc:
                        raise SummaryError(f"{what} {row['Name']}: {exc}", exc.code, exc.n_out_of_range) from None
                    times["histograms"] += s.histograms_ms
                    cuts = quantify.compute_cut_points(amp, args.guide_seq, args.cleavage_offset)
                    table = around = None
                    if alleles:
                        try:
                            t0 = time.perf_counter()
                            table = al_tables.resident_allele_table(dev, n, awidth, amp, d_keep.ptr, d_out.ptr, device,
                                                                    grouper)
                            t1 = time.perf_counter()
                            times["alleles"] += sum(grouper.table_times().values())
                            pairs = guide_cut_pairs(args.guide_seq, cuts)
                            pair_cuts = [c for _, c in pairs]
                            frames = al_tables.resident_around_cut_tables(
                                dev, n, awidth, amp, pair_cuts, int(offset_around_cut), d_keep.ptr, d_out.ptr, table,
                                device, grouper)
                            around = [(sg, c, f) for (sg, c), f in zip(pairs, frames)]
                            if pairs and al_tables.windows_on_device(amp, pair_cuts, int(offset_around_cut)):
                                times["around_cut"] += sum(grouper.window_times().values())
                            times["alleles_wall"] += (t1 - t0) * 1e3
                            times["around_cut_wall"] += (time.perf_counter() - t1) * 1e3
                        except al_tables.AlleleError as exc:
                            raise al_tables.AlleleError(f"{what} {row['Name']}: {exc}") from None
                    reports(g, GroupReport(row["Name"], amp, cuts, n, out[g].copy(),
                                           q.unpack_totals(totals, int(dev["max_cols"])), *hist,
                                           has_coding_seq=bool(args.coding_seq), has_expected_hdr=bool(hdr),
                                           alleles=table, around_cut=around))
    finally:
        quantify._GLOBALS = saved_globals
        aligner.set_output(mode)
    return times


def summarize_pooled(rows: Sequence[dict], reads, aligner, *, min_reads: int = 1000, min_identity_score: float = 60.0,
                     window_around_sgrna: int = 1, cleavage_offset: int = -3, exclude_bp_from_left: int = 15,
                     exclude_bp_from_right: int = 15, ignore_substitutions: bool = False,
                     ignore_insertions: bool = False, ignore_deletions: bool = False,
                     hide_mutations_outside_window_NHEJ: bool = False, k: int = 16, min_hits: int = 2,
                     both_strands: bool = True, on_group=None, demultiplexer: Optional[GpuDemultiplexer] = None,
                     quantifier=None, summarizer: Optional[GpuSummarizer] = None, allow_hdr: bool = False,
                     hdr_perfect_alignment_threshold: float = 98.0, reports=None, alleles: bool = False,
                     offset_around_cut: int = 20) -> PooledSummary:
    """Raw reads to CRISPRessoPooled's SAMPLES_QUANTIFICATION_SUMMARY.txt (amplicon mode) with the
    reads in HBM from the first kernel to the last.

    ``rows``: what :func:`read_amplicons_file` returns.  ``reads``: the packed host pair
    ``(buf, offsets)`` (or a list of ``str``), uploaded once, or a
    :class:`crispresso_amd.frontend.ResidentReads`, the merged pairs a front-end call left in
    HBM (assigned there, ``nwd_assign_prepared``).  ``aligner`` must be on the reads' device.

    The reads are assigned, oriented, grouped and packed as by
    :func:`align_demultiplexed_resident`.  Then, for every amplicon with strictly more than
    ``min_reads`` reads, in index order: ``set_reference``, adoption, one pass; ``nws_flags`` on
    the records (the filter on the printed identity against ``min_identity_score`` and the
    UNMODIFIED flag, from :func:`identity_thresholds`); the quantifier on the resident ops with
    that device ``pre`` (its globals from the row's sgRNA and coding sequence,
    :func:`crispresso_amd.quantify.globals_from_args`); ``nws_summary``; ``on_group(g, aligner,
    n)`` while the group is resident.  Per group only 16 integers come back.

    With ``allow_hdr`` a row's ``Expected_HDR`` (checked by :func:`checked_expected_hdr`) is used
    as the reference does with ``-e`` (CRISPRessoCORE.py:1849-1856, 536-548, 2014): the group is
    adopted and aligned twice, first against the Expected_HDR amplicon, of which ``nws_printed``
    keeps the printed identity (two bytes a read), then against the amplicon; ``nws_flags_dual``
    keeps a read whose printed identity to either is above ``min_identity_score`` and marks it
    HDR (repaired above ref and >= ``hdr_perfect_alignment_threshold``) or MIXED (above ref,
    below the threshold); the quantifier runs on the alignment to the amplicon.  Rows without
    ``Expected_HDR`` go the way described above in the same call.  The demultiplexer's index
    holds the amplicons only: an HDR allele's read reaches its amplicon through the windows
    outside the edit.

    With ``reports``, a callable ``reports(g, report)``, every summarized amplicon also yields a
    :class:`crispresso_amd.report.GroupReport`: the slots, the quantifier's effect vectors,
    counters and frameshift histograms over the kept reads (``nws_mask_pre`` hands the dropped
    reads to the quantifier as UNMODIFIED, which it skips before any total, as the reference
    drops them before it quantifies) and the four size histograms (``nws_histograms``, counted
    in HBM).  :func:`crispresso_amd.report.write_report` makes the reference's
    ``CRISPResso_on_<name>`` folder of one.  ``counts`` and ``frame`` are the same with and
    without ``reports``.

    With ``alleles`` (needs ``reports``) every report also carries the amplicon's allele table
    (``report.alleles``, the reference's ``df_alleles``) and its tables around the cut sites
    (``report.around_cut``, ``offset_around_cut`` columns each side, the reference's
    ``--offset_around_cut_to_plot``): identical kept reads are grouped in HBM and the rows of one
    read per group are built there (``nwa_table_device``, ``nwa_windows_resident``), so the
    group's text never exists on the host.  These tables are upper case, as the whole resident
    path is.  :func:`crispresso_amd.report.write_report` then writes
    ``Alleles_frequency_table.txt`` and the around-cut files as well.

    Differences from the reference, deliberate: a read is aligned in the orientation the
    demultiplexer chose and is not retried reverse-complemented; an ``Expected_HDR`` row is
    refused unless ``allow_hdr``; without ``reports`` the quantifier's effect vectors and
    histograms (not returned then) are not masked by the identity filter.  A kept read that is
    not an alignment of its amplicon (slot 15) raises :class:`crispresso_amd.quantify.QuantificationError`."""
    from . import quantify
    from .frontend import ResidentReads

    k, min_hits = check_params(k, min_hits)
    if alleles and reports is None:
        raise ValueError("alleles=True fills the amplicons' reports: pass reports as well")
    amplicons = check_summary_rows(rows, allow_hdr)
    hdrs = [checked_expected_hdr(row, amp) for row, amp in zip(rows, amplicons)] if allow_hdr else None
    abuf, aoff = pack_amplicons(amplicons)
    device = int(getattr(aligner, "device", 0))
    resident = isinstance(reads, ResidentReads)
    if resident:
        if reads.closed:
            raise ValueError("the resident reads were released")
        if int(reads.device) != device:
            raise ValueError(f"the aligner is on device {device}, the resident reads on device {reads.device}")
    else:
        rbuf, roff = _packed(reads)
        check_offsets(rbuf, roff, "reads", MAX_READ)
        if len(roff) - 1 > 2 ** 31 - 1:
            raise ValueError("more than 2^31 - 1 reads")
    for what, stage in (("demultiplexer", demultiplexer), ("quantifier", quantifier), ("summarizer", summarizer)):
        if stage is not None and int(stage.device) != device:
            raise ValueError(f"the aligner is on device {device}, the {what} on device {stage.device}")
    d = demultiplexer or default_demultiplexer(device)
    q = quantifier or quantify.default_quantifier(device)
    s = summarizer or default_summarizer(device)

    n_windows, n_ambiguous = d.set_amplicons(abuf, aoff, k)
    if resident:
        which, strand, votes, rival, counts, na, nt, nn, ms = d.assign_prepared(reads, min_hits, both_strands)
    else:
        which, strand, votes, rival, counts, na, nt, nn, ms = d.assign(rbuf, roff, min_hits, both_strands)
    pk = d.pack(na)
    res = DemuxResult(which, strand, votes, rival, counts, pk.group_offsets, pk.order, np.zeros(0, np.uint8),
                      pk.text_offsets, n_windows, n_ambiguous, nt, nn, d.last_fallback(), ms,
                      d.phase_times()["upload_wall"])
    min_reads = max(int(min_reads), 0)      # (an amplicon without a read has nothing to adopt)
    keep = [g for g in range(len(amplicons)) if int(counts[g]) > min_reads]
    skipped = [g for g in range(len(amplicons)) if int(counts[g]) <= min_reads]
    out = np.zeros((len(amplicons), _lib.NWS_SLOTS), np.int64)
    most = max((int(counts[g]) for g in keep), default=0)
    def prepare(g: int, reference: str) -> int:
        aligner.set_reference(reference)
        return d.adopt(aligner, g)

    times = _summarize_groups(rows, amplicons, keep, most, prepare, aligner, q, s, out, "amplicon", min_identity_score,
                              dict(window_around_sgrna=window_around_sgrna, cleavage_offset=cleavage_offset,
                                   exclude_bp_from_left=exclude_bp_from_left, exclude_bp_from_right=exclude_bp_from_right,
                                   ignore_substitutions=ignore_substitutions, ignore_insertions=ignore_insertions,
                                   ignore_deletions=ignore_deletions,
                                   hide_mutations_outside_window_NHEJ=hide_mutations_outside_window_NHEJ), on_group,
                              hdrs, float(hdr_perfect_alignment_threshold), reports, bool(alleles),
                              int(offset_around_cut))
    frame = summary_frame([row["Name"] for row in rows], out, counts.tolist(), skipped)
    return PooledSummary(out, frame, res, skipped, times)


# ---- the command line's files ------------------------------------------------------------------

def clean_filename(name: str) -> str:
    """The reference's ``clean_filename``: the characters a file name may hold, the rest dropped."""
    return "".join(c for c in name.encode("ascii", "ignore").decode("ascii") if c in _VALID_FILENAME_CHARS)


def read_amplicons_file(path: str) -> List[dict]:
    """The reference's amplicon table (CRISPRessoPooledCORE.py:739-787): tab-separated name,
    sequence, then sgRNA, expected HDR and coding sequence, which are carried to the report and
    otherwise ignored.  ``#`` starts a comment; lines without a name or a sequence are dropped;
    sequences are upper-cased; blanks in a name become ``_``; names and sequences must be
    distinct and hold only ``ACGTN``."""
    rows = []
    with open(path, "r") as f:
        for line in f:
            line = line.split("#", 1)[0].rstrip("\r\n")
            if not line.strip():
                continue
            cells = [c.strip() for c in line.split("\t")] + [""] * 5
            name, seq = cells[0], cells[1].upper()
            if not name or not seq:
                continue
            rows.append({"Name": name.replace(" ", "_"), "Amplicon_Sequence": seq, "sgRNA": cells[2].upper(),
                         "Expected_HDR": cells[3].upper(), "Coding_sequence": cells[4].upper()})
    if len({r["Amplicon_Sequence"] for r in rows}) != len(rows):
        raise ValueError("The amplicons should be all distinct!")
    if len({r["Name"] for r in rows}) != len(rows):
        raise ValueError("The amplicon names should be all distinct!")
    for r in rows:
        wrong = sorted(set(r["Amplicon_Sequence"]) - set("ATCGN"))
        if wrong:
            raise ValueError("The amplicon sequence %s contains wrong characters:%s" % (r["Name"], " ".join(wrong)))
    if not rows:
        raise ValueError(f"{path} holds no amplicon")
    return rows


def fastq_record(name: bytes, seq: bytes, qual: bytes, strand: int = 0) -> bytes:
    """``@name\\nseq\\n+\\nqual\\n`` as the reference's awk prints SAM fields 1, 10 and 11
    (CRISPRessoPooledCORE.py:874-875): a strand-1 read reverse-complemented, its qualities
    reversed."""
    if strand:
        seq, qual = reverse_complement(seq), qual[::-1]
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def write_fastq_gz(path: str, names, seqs, quals, strands=None) -> int:
    with gzip.open(path, "wb") as f:
        for i, (nm, s, q) in enumerate(zip(names, seqs, quals)):
            f.write(fastq_record(nm, s, q, int(strands[i]) if strands is not None else 0))
    return len(names)


def report_lines(rows: Sequence[dict], files: Sequence[str], n_reads: Sequence[int]) -> List[str]:
    """REPORT_READS_ALIGNED_TO_AMPLICONS.txt (CRISPRessoPooledCORE.py:915-921): the table's
    columns, the file, ``n_reads`` and ``n_reads_aligned_%`` = n_reads over all assigned reads;
    an empty cell is ``NA``."""
    total = float(sum(int(x) for x in n_reads))
    out = ["\t".join(REPORT_COLUMNS)]
    for row, fname, nr in zip(rows, files, n_reads):
        pct = int(nr) / total * 100.0 if total else float("nan")
        cells = [row["Name"], row["Amplicon_Sequence"], row["sgRNA"] or "NA", row["Expected_HDR"] or "NA",
                 row["Coding_sequence"] or "NA", fname, str(int(nr)), "NA" if pct != pct else repr(pct)]
        out.append("\t".join(cells))
    return out


def unassigned_report_lines(n_reads: int, n_tie: int, n_no_hit: int) -> List[str]:
    """REPORT_READS_UNASSIGNED.txt: one line per reason (the reference has no counterpart)."""
    out = ["reason\tn_reads\tn_reads_%"]
    for reason, k in (("tie", n_tie), ("no_hit", n_no_hit)):
        out.append("%s\t%d\t%s" % (reason, k, repr(k / float(n_reads) * 100.0) if n_reads else "NA"))
    return out


def _resident_fastq(rows, fastq, fastq_r2, device, k, min_hits, both_strands, min_reads, front, summary):
    """The front end's way through the files: parsed, filtered, trimmed and merged on the GPU
    (``frontend.prepare_fastq_resident``), assigned where the merged reads lie, and with
    ``summary`` (the options of :func:`summarize_pooled`) quantified there.  Returns (header
    lines, sequences, qualities, DemuxResult, PooledSummary or None)."""
    from .aligner import GpuAligner
    from .frontend import prepare_fastq_resident

    amplicons = (check_summary_rows(rows, bool(summary.get("allow_hdr"))) if summary is not None
                 else [r["Amplicon_Sequence"] for r in rows])
    with GpuAligner(device) as al:
        al.set_reference(amplicons[0])          # the front end wants one; any amplicon will do
        rr, _ = prepare_fastq_resident(al, fastq, fastq_r2, with_quals=True, **front)
        with rr:
            text, qual, off = rr.fetch_text(), rr.fetch_quals(), rr.offsets.tolist()
            seqs = [text[off[j]:off[j + 1]].tobytes() for j in range(len(rr))]
            quals = [qual[off[j]:off[j + 1]].tobytes() for j in range(len(rr))]
            if summary is not None:
                ps = summarize_pooled(rows, rr, al, min_reads=min_reads, k=k, min_hits=min_hits,
                                      both_strands=both_strands, **summary)
                return rr.headers, seqs, quals, ps.result, ps
            k, min_hits = check_params(k, min_hits)
            d = default_demultiplexer(device)
            n_windows, n_ambiguous = d.set_amplicons(*pack_amplicons(amplicons), k)
            which, strand, votes, rival, counts, na, nt, nn, ms = d.assign_prepared(rr, min_hits, both_strands)
            pk = d.pack(na)
            res = DemuxResult(which, strand, votes, rival, counts, pk.group_offsets, pk.order, np.zeros(0, np.uint8),
                              pk.text_offsets, n_windows, n_ambiguous, nt, nn, d.last_fallback(), ms,
                              d.phase_times()["upload_wall"])
            return rr.headers, seqs, quals, res, None


def _folder_writer(out_dir: str, folders: Dict[int, str], refused: List[int]):
    """A ``reports`` callback that writes every group's folder under ``out_dir`` and notes a group
    without a kept read in ``refused``."""
    from . import report

    def write(g: int, rep) -> None:
        folder = os.path.join(out_dir, report.folder_name(rep.name))
        try:
            report.write_report(folder, rep)
        except report.ReportError:
            refused.append(g)
        else:
            folders[g] = folder

    return write


def demultiplex_fastq(amplicons_file: str, fastq: str, out_dir: str, *, k: int = 16, min_hits: int = 2,
                      both_strands: bool = True, min_reads_to_use_region: int = 1000, device: int = 0,
                      fastq_r2: Optional[str] = None, front: Optional[dict] = None,
                      summary: Optional[dict] = None, reports: bool = False, alleles: bool = False,
                      offset_around_cut: int = 20) -> dict:
    """The command line's work; returns what it wrote.

    With ``fastq_r2``, ``front`` (keyword arguments of ``frontend.prepare_fastq_resident``: the
    quality filter, the trim program, the FLASH options) or ``summary`` (keyword arguments of
    :func:`summarize_pooled`, ``{}`` for its defaults) the files go through the GPU front end:
    the per-amplicon FASTQ files then hold the merged (filtered, trimmed) reads under R1's
    headers with FLASH's ``/1`` cut, and with ``summary`` SAMPLES_QUANTIFICATION_SUMMARY.txt is
    written as well.  With ``reports`` (needs ``summary``) every summarized amplicon with a kept
    read gets its ``CRISPResso_on_<name>`` folder (:func:`crispresso_amd.report.write_report`)
    under ``out_dir``: ``report_folders`` maps its index to the folder, ``reports_refused`` lists
    the indices without a kept read.  With ``alleles`` (needs ``reports``) the folders also get
    ``Alleles_frequency_table.txt`` and the tables around the cut sites, ``offset_around_cut``
    columns each side (:func:`summarize_pooled`'s ``alleles``)."""
    from . import ingest

    rows = read_amplicons_file(amplicons_file)
    ps = None
    if alleles and not reports:
        raise ValueError("the allele tables go into the result folders: pass reports as well")
    folders: Dict[int, str] = {}
    refused: List[int] = []
    if reports:
        if summary is None:
            raise ValueError("reports are written from the summary: pass summary as well")
        summary = dict(summary, reports=_folder_writer(out_dir, folders, refused))
        if alleles:
            summary.update(alleles=True, offset_around_cut=int(offset_around_cut))
    if fastq_r2 is not None or front or summary is not None:
        names, seqs, quals, res, ps = _resident_fastq(rows, fastq, fastq_r2, device, k, min_hits, both_strands,
                                                      min_reads_to_use_region, front or {}, summary)
    else:
        names, seqs, quals = ingest.read_fastq(fastq, device)
        res = demultiplex([r["Amplicon_Sequence"] for r in rows], [bytes(s) for s in seqs], k=k, min_hits=min_hits,
                          both_strands=both_strands)
    os.makedirs(out_dir, exist_ok=True)
    files = []
    for g, row in enumerate(rows):
        path = os.path.join(out_dir, "%s.fastq.gz" % clean_filename("AMPL_" + row["Name"]))
        sel = res.order[int(res.group_offsets[g]):int(res.group_offsets[g + 1])].tolist()
        write_fastq_gz(path, [names[r] for r in sel], [seqs[r] for r in sel], [quals[r] for r in sel],
                       [res.strand[r] for r in sel])
        files.append(path)
    left = np.flatnonzero(res.which < 0).tolist()
    unassigned = os.path.join(out_dir, "UNASSIGNED.fastq.gz")
    write_fastq_gz(unassigned, [names[r] + b" " + REASONS[int(res.which[r])].encode() for r in left],
                   [seqs[r] for r in left], [quals[r] for r in left])
    report = os.path.join(out_dir, "REPORT_READS_ALIGNED_TO_AMPLICONS.txt")
    with open(report, "w") as f:
        f.write("\n".join(report_lines(rows, files, res.counts.tolist())) + "\n")
    unassigned_report = os.path.join(out_dir, "REPORT_READS_UNASSIGNED.txt")
    with open(unassigned_report, "w") as f:
        f.write("\n".join(unassigned_report_lines(len(seqs), res.n_tie, res.n_no_hit)) + "\n")
    used = [g for g in range(len(rows)) if int(res.counts[g]) > min_reads_to_use_region]
    out = {"result": res, "rows": rows, "files": files, "unassigned": unassigned, "report": report,
           "unassigned_report": unassigned_report, "regions_to_use": used, "n_reads": len(seqs)}
    if ps is not None:
        out["summary"] = ps
        out["summary_file"] = os.path.join(out_dir, "SAMPLES_QUANTIFICATION_SUMMARY.txt")
        write_summary(out["summary_file"], ps.frame)
    if reports:
        out["report_folders"], out["reports_refused"] = folders, refused
    return out


def build_parser():
    import argparse

    p = argparse.ArgumentParser(prog="python -m crispresso_amd.demux",
                                description="CRISPRessoPooled's amplicon demultiplexing (ONLY_AMPLICONS mode)",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("-f", "--amplicons_file", required=True,
                   help="tab-separated amplicon table: name, sequence, further columns")
    p.add_argument("-r1", "--fastq_r1", required=True, help="reads, FASTQ (plain or gzip)")
    p.add_argument("-o", "--output_folder", required=True)
    p.add_argument("--k", type=int, default=16, help="window length (8 to 31)")
    p.add_argument("--min_hits", type=int, default=2, help="votes a read needs to be assigned")
    p.add_argument("--forward_only", action="store_true", help="do not try the reads' reverse complement")
    p.add_argument("--min_reads_to_use_region", type=float, default=1000,
                   help="an amplicon is worth a CRISPResso run with more reads than this")
    g = p.add_argument_group("the GPU front end (any of these sends the files through it)")
    g.add_argument("-r2", "--fastq_r2", default=None, help="second mates: the pairs are merged as by FLASH")
    g.add_argument("--trim_sequences", action="store_true", help="trim by --trimmomatic_options_string")
    g.add_argument("--trimmomatic_options_string", default="",
                   help="Trimmomatic steps, e.g. 'ILLUMINACLIP:adapters.fa:0:90:10:0:true MINLEN:40'")
    g.add_argument("--min_paired_end_reads_overlap", type=int, default=4)
    g.add_argument("--max_paired_end_reads_overlap", type=int, default=100)
    g.add_argument("-q", "--min_average_read_quality", type=int, default=0)
    g.add_argument("-s", "--min_single_bp_quality", type=int, default=0)
    g = p.add_argument_group("the per-amplicon summary")
    g.add_argument("--summary", action="store_true",
                   help="align and quantify every amplicon's reads and write SAMPLES_QUANTIFICATION_SUMMARY.txt")
    g.add_argument("--reports", action="store_true",
                   help="with --summary: write a CRISPResso_on_<name> folder per summarized amplicon (editing "
                        "frequencies, effect vectors, size histograms), as CRISPRessoCompare reads them")
    g.add_argument("--alleles", action="store_true",
                   help="with --reports: also write Alleles_frequency_table.txt and, per sgRNA, "
                        "Alleles_frequency_table_around_cut_site_for_<sgRNA>.txt into every folder (upper case)")
    g.add_argument("--offset_around_cut_to_plot", type=int, default=None,
                   help="with --alleles: the columns each side of the cut site in the around-cut tables (default 20)")
    g.add_argument("--min_identity_score", type=float, default=60.0)
    g.add_argument("--window_around_sgrna", type=int, default=1)
    g.add_argument("--cleavage_offset", type=int, default=-3)
    g.add_argument("--hdr", action="store_true",
                   help="use the table's Expected_HDR column: align every read to it as well and report HDR%% and "
                        "Mixed_HDR-NHEJ%% (without this option a table with the column filled is refused)")
    g.add_argument("--hdr_perfect_alignment_threshold", type=float, default=None,
                   help="with --hdr: the printed identity to the Expected_HDR amplicon from which a read is HDR and "
                        "not mixed (default 98.0)")
    return p


def options_from_args(p, args) -> dict:
    """The keyword arguments of :func:`demultiplex_fastq` an argument set stands for.  Without any
    of the front end's or the summary's options: exactly the arguments of the demultiplexing
    alone (no ``fastq_r2``, ``front`` or ``summary``)."""
    kw = dict(k=args.k, min_hits=args.min_hits, both_strands=not args.forward_only,
              min_reads_to_use_region=args.min_reads_to_use_region)
    front: dict = {}
    if args.trim_sequences:
        if not args.trimmomatic_options_string.strip():
            p.error("--trim_sequences needs --trimmomatic_options_string (no adapter file is bundled)")
        front["trim"] = args.trimmomatic_options_string
    elif args.trimmomatic_options_string.strip():
        p.error("--trimmomatic_options_string is used only with --trim_sequences")
    if args.min_average_read_quality > 0:
        front["min_bp_quality"] = args.min_average_read_quality
    if args.min_single_bp_quality > 0:
        front["min_single_bp_quality"] = args.min_single_bp_quality
    overlap = (args.min_paired_end_reads_overlap, args.max_paired_end_reads_overlap)
    if overlap != (4, 100):
        if args.fastq_r2 is None:
            p.error("the paired-end overlap options need -r2")
        from .flash import FlashOptions

        front["flash"] = FlashOptions(min_overlap=overlap[0], max_overlap=overlap[1])
    if args.fastq_r2 is not None:
        kw["fastq_r2"] = args.fastq_r2
    if front:
        kw["front"] = front
    if args.summary:
        kw["summary"] = dict(min_identity_score=args.min_identity_score, window_around_sgrna=args.window_around_sgrna,
                             cleavage_offset=args.cleavage_offset)
    elif (args.min_identity_score, args.window_around_sgrna, args.cleavage_offset) != (60.0, 1, -3):
        p.error("--min_identity_score, --window_around_sgrna and --cleavage_offset are used only with --summary")
    if args.hdr:
        if not args.summary:
            p.error("--hdr is used only with --summary")
        kw["summary"]["allow_hdr"] = True
        kw["summary"]["hdr_perfect_alignment_threshold"] = (
            98.0 if args.hdr_perfect_alignment_threshold is None else args.hdr_perfect_alignment_threshold)
    elif args.hdr_perfect_alignment_threshold is not None:
        p.error("--hdr_perfect_alignment_threshold is used only with --hdr")
    if args.reports:
        if not args.summary:
            p.error("--reports is used only with --summary")
        kw["reports"] = True
    if args.alleles:
        if not args.reports:
            p.error("--alleles is used only with --reports")
        kw["alleles"] = True
        kw["offset_around_cut"] = 20 if args.offset_around_cut_to_plot is None else args.offset_around_cut_to_plot
    elif args.offset_around_cut_to_plot is not None:
        p.error("--offset_around_cut_to_plot is used only with --alleles")
    return kw


def main(argv=None) -> int:
    p = build_parser()
    args = p.parse_args(argv)
    files = [args.amplicons_file, args.fastq_r1] + ([args.fastq_r2] if args.fastq_r2 is not None else [])
    for f in files:
        if not os.path.exists(f):
            p.error(f"cannot open {f}")
    kw = options_from_args(p, args)
    if "summary" in kw:
        try:
            check_summary_rows(read_amplicons_file(args.amplicons_file), bool(kw["summary"].get("allow_hdr")))
        except ValueError as exc:
            p.error(str(exc))
    out = demultiplex_fastq(args.amplicons_file, args.fastq_r1, args.output_folder, **kw)
    res = out["result"]
    print(f"{out['n_reads']} reads: {res.n_assigned} assigned to {len(out['rows'])} amplicons, {res.n_tie} ties, "
          f"{res.n_no_hit} without a hit; {len(out['regions_to_use'])} amplicons with more than "
          f"{args.min_reads_to_use_region:g} reads: {out['report']}")
    if "summary_file" in out:
        print(f"summary of {len(out['rows']) - len(out['summary'].skipped)} amplicons: {out['summary_file']}")
    if "report_folders" in out:
        print(f"{len(out['report_folders'])} result folders under {args.output_folder}")
        for g in out["reports_refused"]:
            print(f"amplicon {out['rows'][g]['Name']}: no read passed the identity filter, no folder is written")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
