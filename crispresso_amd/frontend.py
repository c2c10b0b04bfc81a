"""The read front end on the GPU: raw reads (pairs) to a resident aligner batch.

CRISPResso filters the reads by quality (``CRISPResso/CRISPRessoCORE.py:162-308``), trims them
with Trimmomatic (``CORE:1585-1640``), merges pairs with FLASH (``CORE:1655-1677``) and hands the
merged file to the alignment.  :func:`prepare_packed` is those steps in one call on one upload
(C ABI ``nwp_prepare``, ``include/crispr_front.h``, kernels ``crispresso_amd/csrc/front_pack.hip``
with the clip, steps and merge kernels of :mod:`crispresso_amd.trim` and
:mod:`crispresso_amd.flash`): the merged reads stay in HBM, laid out as
``aligner.upload_packed(pack_2bit(text))`` would have left them, and the aligner's
``run_async`` / ``sync`` / ``download_ops`` / ``device_ops`` then run with nothing uploaded in
between.  The host receives each input read's status, the batch's text, offsets, lengths and
source indices.  :func:`prepare_fastq` is that call on FASTQ files read by the interpreter;
:func:`prepare_fastq_device` parses the files on the GPU (:mod:`crispresso_amd.ingest`) and hands
the records to the same kernels where they lie (``nwp_prepare_records``).
:func:`prepare_packed_resident` / :func:`prepare_fastq_resident` are the same calls with the merged
reads kept in HBM (:class:`ResidentReads`) for a stage that reads them there
(``demux.GpuDemultiplexer.assign_prepared``, ``demux.summarize_pooled``).  There is no CPU
fallback: without the library or a GPU every call raises
:class:`crispresso_amd._lib.NativeLibraryError`.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple, Union

import numpy as np

from . import _lib
from .aligner import GpuAligner, PackedReads
from .fastq import fasta_name
from .flash import FlashOptions, _pack, read_fastq
from .ingest import read_fastq_records
from .trim import MAX_STEPS, TrimError, TrimProgram, UnsupportedTrimStep, _check_packed, _clip_arguments

FILTERED, TRIMMED, NOT_COMBINED, COMBINED, COMBINED_OUTIE = (
    _lib.NWP_FILTERED, _lib.NWP_TRIMMED, _lib.NWP_NOT_COMBINED, _lib.NWP_COMBINED, _lib.NWP_COMBINED_OUTIE)


class FrontError(RuntimeError):
    """A failed nwp_prepare / nwp_fetch (the message is the library's); ``code`` is its return."""

    def __init__(self, msg: str, code: int):
        super().__init__(f"{msg} (code {code})")
        self.code = code


@dataclass
class PreparedBatch:
    """What :func:`prepare_packed` left in the aligner's context, as the host sees it."""
    status: np.ndarray    # uint8 [n]: FILTERED, TRIMMED, NOT_COMBINED, COMBINED, COMBINED_OUTIE per input read
    src: np.ndarray       # int64 [m]: the input index of each batch read
    buf: np.ndarray       # uint8: the batch's text, dense
    offsets: np.ndarray   # int64 [m + 1], from 0
    lens: np.ndarray      # uint16 [m]
    quals: Optional[np.ndarray] = None   # uint8, dense, ASCII (with_quals)
    packed: Optional[PackedReads] = None   # the 2-bit stream and its exceptions (with_packed)
    stats: Dict[str, Union[int, float]] = field(default_factory=dict)

    def __len__(self) -> int:
        return len(self.lens)

    def read(self, j: int) -> bytes:
        return self.buf[self.offsets[j]:self.offsets[j + 1]].tobytes()


def prepare_packed(aligner: GpuAligner, s1: np.ndarray, q1: np.ndarray, off1: np.ndarray,
                   s2: Optional[np.ndarray], q2: Optional[np.ndarray], off2: Optional[np.ndarray], *,
                   min_bp_quality: int = 0, min_single_bp_quality: int = 0,
                   trim: Union[None, str, List[str], TrimProgram] = None, flash: Optional[FlashOptions] = None,
                   with_quals: bool = False, with_packed: bool = False,
                   force_ops_output: bool = True) -> PreparedBatch:
    """Filter, trim, merge and pack read pairs on the GPU and leave the merged reads in
    ``aligner``'s context as its resident batch.

    Inputs are packed: uint8 sequence / quality buffers and int64 offsets (n + 1, from 0) per
    mate; ``s2=None``: single-end reads (filter, trim, pack; no merge).  ``trim`` is a
    :class:`TrimProgram` or a ``--trimmomatic_options_string`` (:meth:`TrimProgram.from_steps`,
    with its refusals); ``flash`` defaults to CRISPResso's FLASH options.  With the filter on, an
    empty read raises ``ValueError`` (as ``fastq.get_ids_reads_to_remove``).  The aligner must have
    a reference; its output mode is set to "ops" unless ``force_ops_output`` is False (then a
    context in rows mode is refused, as by ``upload_packed``'s C entry).  When no read survives the
    context keeps its previous batch."""
    lib, res, n = _call_packed("prepare_packed", aligner, s1, q1, off1, s2, q2, off2, min_bp_quality,
                               min_single_bp_quality, trim, flash, with_quals, force_ops_output)
    return _collect(aligner, lib, res, n, with_quals, with_packed)


def _call_packed(who: str, aligner: GpuAligner, s1, q1, off1, s2, q2, off2, min_bp_quality, min_single_bp_quality, trim,
                 flash, with_quals: bool, force_ops_output: bool):
    """nwp_prepare on packed host reads: ``(lib, the live nwp_result, n)``."""
    paired = s2 is not None
    prog = _program(who, trim)
    s1, q1, off1, s2, q2, off2 = _check_packed(who, s1, q1, off1, s2, q2, off2)
    n = len(off1) - 1
    filt = min_bp_quality > 0 or min_single_bp_quality > 0
    if filt and n and (np.any(np.diff(off1) == 0) or (paired and np.any(np.diff(off2) == 0))):
        raise ValueError(f"{who}: a record has no qualities")   # numpy: min() of an empty array
    p, _alive = _params(prog, min_bp_quality, min_single_bp_quality, flash, with_quals)
    lib = _lib.load()
    if force_ops_output:
        aligner.set_output("ops")
    res = _lib.NwpResult()
    rc = lib.nwp_prepare(aligner._h, ctypes.byref(p), _lib.ptr(s1), _lib.ptr(q1), _lib.ptr(off1),
                         _lib.ptr(s2) if paired else None, _lib.ptr(q2) if paired else None,
                         _lib.ptr(off2) if paired else None, n, ctypes.byref(res))
    if rc != 0:
        raise FrontError(lib.nwp_last_error().decode(errors="replace"), rc)
    return lib, res, n


def _program(who: str, trim) -> TrimProgram:
    prog = trim if isinstance(trim, TrimProgram) else (TrimProgram.from_steps(trim) if trim else TrimProgram())
    if prog.clip is not None and prog.clip.minlen != 0:
        raise TrimError(f"{who}: the clip options' minlen must be 0 (MINLEN is a step)")
    if len(prog.steps) > MAX_STEPS:
        raise UnsupportedTrimStep(f"more than {MAX_STEPS} steps after ILLUMINACLIP")
    return prog


def _params(prog: TrimProgram, min_bp_quality: int, min_single_bp_quality: int, flash: Optional[FlashOptions],
            with_quals: bool):
    """nwp_params and the arrays its pointers point into (to be kept until the call returns)."""
    o = flash or FlashOptions()
    p = _lib.NwpParams()
    p.min_avg_quality, p.min_single_quality = int(min_bp_quality), int(min_single_bp_quality)
    alive = []
    if prog.clip is not None:
        _args, arrays = _clip_arguments(prog.clip, 0)
        clip, ad, ad_off, roles, pre, pre_off = arrays
        alive.append(arrays)
        p.clip = ctypes.pointer(clip)
        p.adapters, p.adapter_off, p.adapter_role = _lib.ptr(ad), _lib.ptr(ad_off), _lib.ptr(roles)
        p.prefixes, p.prefix_off = _lib.ptr(pre), _lib.ptr(pre_off)
        p.n_adapters, p.n_prefix_pairs = len(prog.clip.adapters), len(prog.clip.prefix_pairs)
    steps = prog.native_steps()
    alive.append(steps)
    p.steps, p.n_steps = ctypes.cast(steps, ctypes.POINTER(_lib.NwtStep)), len(prog.steps)
    p.flash = _lib.NwfParams(o.min_overlap, o.max_overlap, o.max_mismatch_density, int(o.allow_outies),
                             o.phred_offset, int(o.cap_mismatch_quals))
    p.want_quals = int(with_quals)
    return p, alive


def _stats(res, n: int) -> Dict[str, Union[int, float]]:
    """The counters and kernel times of an nwp_result as PreparedBatch.stats names them."""
    total, n_exc = int(res.total), int(res.n_exc)
    c = [int(x) for x in res.counts]
    t = [int(x) for x in res.trim]
    stats: Dict[str, Union[int, float]] = {
        "pairs": n, "filtered": c[FILTERED], "trimmed": c[TRIMMED], "not_combined": c[NOT_COMBINED],
        "combined": c[COMBINED] + c[COMBINED_OUTIE], "innies": c[COMBINED], "outies": c[COMBINED_OUTIE],
        # Trimmomatic's summary line, over the reads the filter kept
        "trim_pairs": n - c[FILTERED], "both": t[0], "fwd_only": t[1], "rev_only": t[2], "dropped": t[3],
        "bases": total, "exceptions": n_exc,
    }
    for k, name in enumerate(_lib.NWP_MS):
        stats[name + "_ms"] = float(res.kernel_ms[k])
    return stats


def _collect(aligner: GpuAligner, lib, res, n: int, with_quals: bool, with_packed: bool) -> PreparedBatch:
    """The host's copies of a successful nwp_prepare / nwp_prepare_records; releases ``res``."""
    try:
        m, total, n_exc = int(res.m), int(res.total), int(res.n_exc)
        pool = _lib.pinned_pool()
        status = np.zeros(n, np.uint8)
        # the largest first: the pool hands a request the smallest free block that fits, and a
        # small array must not take the text's block while it is the only free one
        buf = pool.array(total, np.uint8)
        quals = pool.array(total, np.uint8) if with_quals else None
        offsets = pool.array(m + 1, np.int64)
        src = pool.array(m, np.int64)
        lens = pool.array(m, np.uint16)
        packed = np.zeros(max((total + 3) // 4, 1), np.uint8) if with_packed else None
        exc_pos = np.zeros(n_exc, np.int64) if with_packed else None
        exc_byte = np.zeros(n_exc, np.uint8) if with_packed else None
        rc = lib.nwp_fetch(ctypes.byref(res), _lib.ptr(status), _lib.ptr(offsets), _lib.ptr(lens), _lib.ptr(src),
                           _lib.ptr(buf), _lib.ptr(quals), _lib.ptr(packed), _lib.ptr(exc_pos), _lib.ptr(exc_byte))
        if rc != 0:
            raise FrontError(lib.nwp_last_error().decode(errors="replace"), rc)
    finally:
        lib.nwp_release(ctypes.byref(res))
    stats = _stats(res, n)
    pb = PreparedBatch(status, src, buf, offsets, lens, quals,
                       PackedReads(packed, offsets, exc_pos, exc_byte, lens) if with_packed else None, stats)
    if m:
        aligner.adopted(buf, offsets)
    return pb


def prepare_fastq(aligner: GpuAligner, r1: str, r2: Optional[str] = None, **kw) -> Tuple[PreparedBatch, List[str]]:
    """:func:`prepare_packed` on FASTQ(.gz) files (read as ``flash.run_flash`` reads them;
    ``r2=None``: single-end).  Returns the batch and its reads' names: R1's header lines at
    ``src`` (FLASH's own ``/1`` cut first) through :func:`crispresso_amd.fastq.fasta_name`: the names
    the aligner's ingest gives the records of FLASH's merged file."""
    n1, s1, q1 = read_fastq(r1)
    n = len(s1)
    if r2 is not None:
        _, s2, q2 = read_fastq(r2)
        n = min(n, len(s2))
    for s, q in zip(s1[:n], q1[:n]):
        if len(s) != len(q):
            raise FrontError("prepare_fastq: a sequence and its quality line differ in length", -1)
    b1, off1 = _pack(s1[:n])
    bq1, _ = _pack(q1[:n])
    if r2 is not None:
        for s, q in zip(s2[:n], q2[:n]):
            if len(s) != len(q):
                raise FrontError("prepare_fastq: a sequence and its quality line differ in length", -1)
        b2, off2 = _pack(s2[:n])
        bq2, _ = _pack(q2[:n])
    else:
        b2 = bq2 = off2 = None
    pb = prepare_packed(aligner, b1, bq1, off1, b2, bq2, off2, **kw)
    names = []
    for i in pb.src:
        h = n1[int(i)]
        if r2 is not None and h.endswith(b"/1"):
            h = h[:-2]
        names.append(fasta_name(b"@" + h))
    return pb, names


def prepare_fastq_device(aligner: GpuAligner, r1: str, r2: Optional[str] = None, *, min_bp_quality: int = 0,
                         min_single_bp_quality: int = 0, trim: Union[None, str, List[str], TrimProgram] = None,
                         flash: Optional[FlashOptions] = None, with_quals: bool = False, with_packed: bool = False,
                         force_ops_output: bool = True) -> Tuple[PreparedBatch, List[str]]:
    """:func:`prepare_fastq` with the files parsed on the GPU (:mod:`crispresso_amd.ingest`,
    ``nwi_parse_file``) and handed to the front end where they lie (``nwp_prepare_records``): the
    same arguments, the same ``(PreparedBatch, names)``; only the text of each file is uploaded,
    and only R1's names come back.  A malformed record among the first ``min(n1, n2)`` (header,
    '+' line, line lengths, quality range) refuses the call with :class:`FrontError` (code -1),
    a sequence longer than 4096 bases anywhere in either file with code -3."""
    return _fastq_device("prepare_fastq_device", lambda lib, res, n: _collect(aligner, lib, res, n, with_quals, with_packed),
                         aligner, r1, r2, min_bp_quality, min_single_bp_quality, trim, flash, with_quals,
                         force_ops_output)


def _fastq_device(who: str, collect, aligner: GpuAligner, r1: str, r2: Optional[str], min_bp_quality: int,
                  min_single_bp_quality: int, trim, flash, with_quals: bool, force_ops_output: bool):
    """The files parsed on the GPU, nwp_prepare_records on the records, ``collect(lib, res, n)``
    on the live result (a :class:`PreparedBatch` or a :class:`ResidentReads`), and the names."""
    prog = _program(who, trim)
    lib = _lib.load()
    a = read_fastq_records(r1, aligner.device, strict=False, fetch=False)
    b = None
    try:
        if r2 is not None:
            b = read_fastq_records(r2, aligner.device, strict=False, fetch=False)
        n = len(a) if b is None else min(len(a), len(b))
        filt = min_bp_quality > 0 or min_single_bp_quality > 0
        if filt and n:   # as prepare_packed: the filter's mean of an empty read (a flagged record: refused below)
            for rec in (a, b):
                if rec is not None and not 0 <= rec.info["first_bad"] < n and np.any(np.diff(rec.fetch_offsets()[:n + 1]) == 0):
                    raise ValueError(f"{who}: a record has no qualities")
        p, _alive = _params(prog, min_bp_quality, min_single_bp_quality, flash, with_quals)
        if force_ops_output:
            aligner.set_output("ops")
        res = _lib.NwpResult()
        rc = lib.nwp_prepare_records(aligner._h, ctypes.byref(p), a._h, b._h if b is not None else None,
                                     ctypes.byref(res))
        if rc != 0:
            raise FrontError(lib.nwp_last_error().decode(errors="replace"), rc)
        pb = collect(lib, res, n)
        raw, name_off = a.fetch_names()
        raw, name_off = raw.tobytes(), name_off.tolist()
    finally:
        a.close()
        if b is not None:
            b.close()
    names, heads = [], []
    for i in pb.src.tolist():
        h = raw[name_off[i]:name_off[i + 1]]
        if r2 is not None and h.endswith(b"/1"):
            h = h[:-2]
        heads.append(h)
        names.append(fasta_name(b"@" + h))
    if isinstance(pb, ResidentReads):
        pb.headers = heads
    return pb, names


class ResidentReads:
    """The merged reads of one front-end call, still in HBM: a live ``nwp_result`` that another
    stage reads where it lies (``demux.GpuDemultiplexer.assign_prepared``).  The host holds what
    it needs to name and place the reads (``status``, ``src``, ``offsets``, ``lens``, ``stats``);
    the text and the qualities are fetched only when asked for.  A context manager: ``close()``
    releases the device arrays (``nwp_release``); the aligner keeps its batch."""

    def __init__(self, aligner: GpuAligner, lib, res, n: int, with_quals: bool):
        self._lib, self._res = lib, res
        self.device = aligner.device
        self.with_quals = bool(with_quals)
        self.headers: Optional[List[bytes]] = None   # R1's header lines (FLASH's /1 cut), from prepare_fastq_resident
        m = int(res.m)
        try:
            self.status = np.zeros(n, np.uint8)
            self.offsets = np.zeros(m + 1, np.int64)
            self.lens = np.zeros(m, np.uint16)
            self.src = np.zeros(m, np.int64)
            self._check(lib.nwp_fetch(ctypes.byref(res), _lib.ptr(self.status), _lib.ptr(self.offsets),
                                      _lib.ptr(self.lens), _lib.ptr(self.src), None, None, None, None, None))
        except Exception:
            self.close()
            raise
        self.stats = _stats(res, n)
        if m:
            aligner.adopted(None, self.offsets)

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise FrontError(self._lib.nwp_last_error().decode(errors="replace"), rc)

    def __len__(self) -> int:
        return len(self.lens)

    @property
    def closed(self) -> bool:
        return not self._res.handle

    @property
    def total(self) -> int:
        return int(self.offsets[-1])

    def result(self):
        """The ``nwp_result`` (a :class:`crispresso_amd._lib.NwpResult`) for a C entry that takes it."""
        return self._res

    def _fetch(self, quals: bool) -> np.ndarray:
        if self.closed:
            raise FrontError("the reads were released", -1)
        out = _lib.pinned_pool().array(self.total, np.uint8)
        self._check(self._lib.nwp_fetch(ctypes.byref(self._res), None, None, None, None, None if quals else _lib.ptr(out),
                                        _lib.ptr(out) if quals else None, None, None, None))
        return out

    def fetch_text(self) -> np.ndarray:
        """The batch's text, dense (uint8, read j at ``offsets[j]:offsets[j + 1]``), copied to the host."""
        return self._fetch(False)

    def fetch_quals(self) -> np.ndarray:
        """The batch's qualities, dense, ASCII (a call made with ``with_quals``)."""
        if not self.with_quals:
            raise FrontError("the call did not keep the qualities (with_quals)", -1)
        return self._fetch(True)

    def close(self) -> None:
        if getattr(self, "_res", None) is not None and self._res.handle:
            self._lib.nwp_release(ctypes.byref(self._res))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def prepare_packed_resident(aligner: GpuAligner, s1: np.ndarray, q1: np.ndarray, off1: np.ndarray,
                            s2: Optional[np.ndarray], q2: Optional[np.ndarray], off2: Optional[np.ndarray], *,
                            min_bp_quality: int = 0, min_single_bp_quality: int = 0,
                            trim: Union[None, str, List[str], TrimProgram] = None, flash: Optional[FlashOptions] = None,
                            with_quals: bool = False, force_ops_output: bool = True) -> ResidentReads:
    """:func:`prepare_packed` that leaves the merged reads in HBM: the same arguments (but
    ``with_packed``), a :class:`ResidentReads` instead of the host's copies.  The aligner still
    adopts the whole batch (for a pooled run any amplicon serves as its reference; the adoption is
    a device-to-device copy that the first group's adoption overwrites)."""
    lib, res, n = _call_packed("prepare_packed_resident", aligner, s1, q1, off1, s2, q2, off2, min_bp_quality,
                               min_single_bp_quality, trim, flash, with_quals, force_ops_output)
    return ResidentReads(aligner, lib, res, n, with_quals)


def prepare_fastq_resident(aligner: GpuAligner, r1: str, r2: Optional[str] = None, *, min_bp_quality: int = 0,
                           min_single_bp_quality: int = 0, trim: Union[None, str, List[str], TrimProgram] = None,
                           flash: Optional[FlashOptions] = None, with_quals: bool = False,
                           force_ops_output: bool = True) -> Tuple[ResidentReads, List[str]]:
    """:func:`prepare_fastq_device` that leaves the merged reads in HBM: ``(ResidentReads, names)``."""
    return _fastq_device("prepare_fastq_resident", lambda lib, res, n: ResidentReads(aligner, lib, res, n, with_quals),
                         aligner, r1, r2, min_bp_quality, min_single_bp_quality, trim, flash, with_quals,
                         force_ops_output)
