"""The allele table (``Alleles_frequency_table.txt``, CRISPResso/CRISPRessoCORE.py:2923-2946)
without the per-read DataFrame, behind the C ABI of ``include/crispr_alleles.h``.

An alignment is a function of the read's bytes, and ``align_seq`` without its ``-`` is the
read, so within one batch against one amplicon the reference's groups are the groups of
byte-identical reads.  :class:`GpuAlleleGrouper` finds them in HBM on the batch the aligner
left there (``GpuAligner.device_ops()``: crispresso_amd/csrc/nw_alleles.hip);
:func:`allele_table` builds the strings of one representative per group and finishes with
the reference's own last steps on that small frame.

* :func:`group_reads_host`   -- the same groups from the host text (no GPU; case-sensitive)
* :func:`group_reads`        -- the device when an aligner holds the batch and no read has a
  lowercase byte (the device bytes are upper case, ``align_seq`` keeps the text), else the host
* :func:`allele_table`       -- groups + ops + ``nwq_read`` results -> ``df_alleles``
* :func:`merge_allele_tables` -- tables of several batches (forward + RC retry, shards) -> one
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np
import pandas as pd

from . import _lib
from ._lib import NativeLibraryError

KEYS = ["Aligned_Sequence", "Reference_Sequence", "NHEJ", "UNMODIFIED", "HDR", "n_deleted", "n_inserted", "n_mutated"]


class AlleleError(RuntimeError):
    """A failed grouping call, or results that do not belong to the batch."""


@dataclass
class ReadGroups:
    """Groups of identical kept reads in order of first appearance."""

    first: np.ndarray                      # int64 [groups]: the group's smallest read index, increasing
    count: np.ndarray                      # int64 [groups]
    group_of_read: Optional[np.ndarray]    # int32 [n] (-1: not kept), when asked for
    collided: int = 0                      # reads the device pass left to the host (equal hashes, different bytes)

    def __len__(self) -> int:
        return len(self.first)


def _host_arrays(n: int, keep, tag):
    if keep is not None:
        keep = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        if len(keep) != n:
            raise AlleleError(f"{len(keep)} keep flags for {n} reads")
    if tag is not None:
        tag = np.ascontiguousarray(tag, dtype=np.int32)
        if len(tag) != n:
            raise AlleleError(f"{len(tag)} tags for {n} reads")
    return keep, tag


def _grouped(call, n: int, keep, want_group_of_read: bool):
    """Run ``call(first, count, cap, group_of_read, n_groups)`` with room for one group per
    kept read (16 bytes each: never NW_E_CAPACITY, never a second pass)."""
    gor = np.empty(n, np.int32) if want_group_of_read else None
    cap = n if keep is None else int(np.count_nonzero(keep))
    first = np.empty(max(cap, 1), np.int64)
    count = np.empty(max(cap, 1), np.int64)
    ng = ctypes.c_int64()
    rc = call(first, count, cap, gor, ng)
    if rc != 0:
        return rc, None, None, None
    return rc, first[: ng.value].copy(), count[: ng.value].copy(), gor


class GpuAlleleGrouper:
    """One ``nwa_ctx`` (one GPU).  Not thread-safe, like the aligner context."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        ctx = ctypes.c_void_p()
        rc = self._lib.nwa_create(int(device), ctypes.byref(ctx))
        if rc != 0:
            raise NativeLibraryError(f"nwa_create(device={device}) failed with code {rc} (no GPU?)")
        self._ctx = ctx
        self.device = device
        self.last_kernel_ms = 0.0

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.nwa_destroy(self._ctx)
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

    @property
    def reads_per_step(self) -> int:
        return int(self._lib.nwa_reads_per_step(self._ctx))

    def phase_times(self) -> Dict[str, float]:
        """Device ms of the last :meth:`group` by phase."""
        ms = np.zeros(4, np.float32)
        self._lib.nwa_phase_times(self._ctx, _lib.ptr(ms))
        return dict(zip(("hash", "insert", "verify", "compaction"), (float(x) for x in ms)))

    def group(self, dev: dict, n: int, keep=None, tag=None, want_group_of_read: bool = False) -> ReadGroups:
        """Groups of the n reads of a device-resident batch: ``dev`` is
        ``GpuAligner.device_ops()`` (its ``reads``, ``offsets`` and ``reads_bias``)."""
        n = int(n)
        keep, tag = _host_arrays(n, keep, tag)
        ms = ctypes.c_float()

        def call(first, count, cap, gor, ng):
            return self._lib.nwa_group_device(self._ctx, dev["reads"], dev["offsets"], int(dev["reads_bias"]), n,
                                              _lib.ptr(keep), _lib.ptr(tag), _lib.ptr(first), _lib.ptr(count), cap,
                                              _lib.ptr(gor), ctypes.byref(ng), ctypes.byref(ms))

        rc, first, count, gor = _grouped(call, n, keep, want_group_of_read)
        if rc != 0:
            msg = self._lib.nwa_last_error(self._ctx).decode(errors="replace")
            raise AlleleError(f"nwa_group_device failed ({rc}): {msg}")
        self.last_kernel_ms = ms.value
        return ReadGroups(first, count, gor, int(self._lib.nwa_last_collided(self._ctx)))


_DEFAULT: Dict[int, GpuAlleleGrouper] = {}


def default_grouper(device: int = 0) -> GpuAlleleGrouper:
    g = _DEFAULT.get(device)
    if g is None:
        g = _DEFAULT[device] = GpuAlleleGrouper(device)
    return g


def group_reads_host(buf: np.ndarray, offsets: np.ndarray, keep=None, tag=None, want_group_of_read: bool = False,
                     nthreads: int = 0) -> ReadGroups:
    """The groups from the host text (nwa_group_host): case-sensitive, no GPU."""
    lib = _lib.load()
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    keep, tag = _host_arrays(n, keep, tag)

    def call(first, count, cap, gor, ng):
        return lib.nwa_group_host(_lib.ptr(buf), _lib.ptr(offsets), n, _lib.ptr(keep), _lib.ptr(tag), _lib.ptr(first),
                                  _lib.ptr(count), cap, _lib.ptr(gor), ctypes.byref(ng), int(nthreads))

    rc, first, count, gor = _grouped(call, n, keep, want_group_of_read)
    if rc != 0:
        raise AlleleError(f"nwa_group_host failed ({rc})")
    return ReadGroups(first, count, gor, 0)


def reads_have_lower(buf: np.ndarray, offsets: np.ndarray, nthreads: int = 0) -> bool:
    """Whether any read holds a byte ``a``-``z`` (nwa_reads_have_lower)."""
    lib = _lib.load()
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    rc = lib.nwa_reads_have_lower(_lib.ptr(buf), _lib.ptr(offsets), len(offsets) - 1, int(nthreads))
    if rc < 0:
        raise AlleleError(f"nwa_reads_have_lower failed ({rc})")
    return bool(rc)


def group_reads(aligner, buf: np.ndarray, offsets: np.ndarray, keep=None, tag=None,
                want_group_of_read: bool = False) -> ReadGroups:
    """The groups of a batch: on the device when ``aligner`` (a GpuAligner) holds it resident
    (its last upload / run in ops mode) and no read has a lowercase byte -- the device bytes are
    upper case, so ``acgt`` and ``ACGT`` would merge there while ``align_seq`` keeps the text --
    otherwise from the host text."""
    n = len(offsets) - 1
    dev = None
    if aligner is not None and n > 0 and hasattr(aligner, "device_ops") and not reads_have_lower(buf, offsets):
        from .aligner import NeedleError

        try:
            dev = aligner.device_ops()
        except NeedleError:      # no resident ops-mode batch (a call-level or pooled pass leaves none)
            dev = None
    if dev is None:
        return group_reads_host(buf, offsets, keep, tag, want_group_of_read)
    return default_grouper(aligner.device).group(dev, n, keep, tag, want_group_of_read)


def _finish(frame: pd.DataFrame) -> pd.DataFrame:
    """The reference's last steps (CORE:2923-2946) on a frame of distinct rows with their
    counts in ``#Reads``: group by the eight keys, %Reads, sort by #Reads descending."""
    alleles = frame.groupby(KEYS)["#Reads"].sum().reset_index()
    alleles["%Reads"] = alleles["#Reads"] / alleles["#Reads"].sum() * 100.0
    return alleles.sort_values(by="#Reads", ascending=False)


def allele_table(amplicon: str, buf: np.ndarray, offsets: np.ndarray, ops_batch, read_results,
                 groups: ReadGroups, nthreads: int = 0) -> pd.DataFrame:
    """``run_summary(df)["df_alleles"]`` without the per-read DataFrame.

    ``ops_batch``: the batch's :class:`~crispresso_amd.aligner.OpsBatch`; ``read_results``: the
    ``[n][4]`` int32 array of ``nwq_read`` (cls, n_mutated, n_inserted, n_deleted) the
    quantification produced (or its structured form); ``groups``: the groups of the kept reads
    (:func:`group_reads`).  The three rows are built for each group's first read only
    (nw_expand_ops_subset), cut to ``awidth`` columns as the DataFrame's are; NHEJ / UNMODIFIED /
    HDR come from ``cls`` as ``quantify._result_tuple`` maps them.  The final group-by over
    these distinct rows restores the reference's groups where byte groups are finer (an RC-retry
    input that still carries ``-`` gives one ``align_seq`` from two inputs), and makes the frame
    that is sorted the one ``run_summary`` sorts: equal under ``assert_frame_equal``, ties
    included.  ``ref_positions`` (CORE:2948-2953) is not added, as in ``run_summary``."""
    lib = _lib.load()
    rr = np.asarray(read_results)
    if rr.dtype.names:
        rr = np.ascontiguousarray(rr).view(np.int32).reshape(-1, 4)
    idx = np.ascontiguousarray(groups.first, dtype=np.int64)
    m = len(idx)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    n = len(offsets) - 1
    if len(rr) != n or len(ops_batch) != n or (m and (idx.min() < 0 or idx.max() >= n)):
        raise AlleleError("groups, results and alignments are not of one batch")
    res = rr[idx]
    cls = res[:, 0]
    if (cls < 0).any():
        raise AlleleError(f"reads are not aligned to the amplicon (LEN_AMPLICON bases): {idx[cls < 0][:5].tolist()}")
    ref = amplicon.encode("ascii")
    aln_len = ops_batch.stats["aln_len"][idx].astype(np.int64)
    cols = np.minimum(aln_len, ops_batch.awidth)
    stride = max(16, (int(aln_len.max()) + 15) & ~15) if m else 16
    rows = np.zeros((m, 3, stride), np.uint8)
    ops = np.ascontiguousarray(ops_batch.ops, dtype=np.uint32)
    rc = lib.nw_expand_ops_subset(ref, len(ref), _lib.ptr(buf), _lib.ptr(offsets), _lib.ptr(idx), m,
                                  _lib.ptr(ops) if len(ops) else None, _lib.ptr(ops_batch.ops_off), _lib.ptr(rows),
                                  stride, int(nthreads))
    if rc != _lib.NW_OK:
        raise AlleleError(f"nw_expand_ops_subset: runs do not match the reads (code {rc})")
    ref_rows = rows[:, 0, :].tobytes()
    seq_rows = rows[:, 2, :].tobytes()
    frame = pd.DataFrame({
        "Aligned_Sequence": [seq_rows[q * stride:q * stride + c].decode("ascii") for q, c in enumerate(cols.tolist())],
        "Reference_Sequence": [ref_rows[q * stride:q * stride + c].decode("ascii") for q, c in enumerate(cols.tolist())],
        "NHEJ": cls == 1, "UNMODIFIED": cls == 0, "HDR": cls == 2,
        "n_deleted": res[:, 3].astype(np.int64), "n_inserted": res[:, 2].astype(np.int64),
        "n_mutated": res[:, 1].astype(np.int64),
        "#Reads": np.asarray(groups.count, dtype=np.int64),
    }, columns=KEYS + ["#Reads"])
    return _finish(frame)


def merge_allele_tables(tables: Sequence[pd.DataFrame]) -> pd.DataFrame:
    """One table from the tables of several batches (the forward batch + the RC-retry batch,
    the shards of ``distributed.py``): ``#Reads`` summed by the eight keys, ``%Reads``
    recomputed, sorted again."""
    tables = [t for t in tables if t is not None and len(t)]
    if not tables:
        return _finish(pd.DataFrame({k: [] for k in KEYS + ["#Reads"]}).astype({"#Reads": np.int64}))
    return _finish(pd.concat([t[KEYS + ["#Reads"]] for t in tables], ignore_index=True))
