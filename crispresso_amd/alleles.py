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

The table around a cut site (``Alleles_frequency_table_around_cut_site_for_<sgRNA>.txt``,
CORE:801-836, 3642-3657) regroups the alleles by a ``2 * offset``-column window.  That window is
a function of a read's runs, its bytes and the amplicon, so it is cut and grouped per read in
HBM (crispresso_amd/csrc/nw_windows.hip) and strings are built for the window groups only.

* :func:`around_cut_from_alleles` -- ``get_dataframe_around_cut`` on a ``df_alleles`` (no GPU)
* :func:`around_cut_tables`       -- one frame per cut point: from the resident batch when the
  device path takes the arguments, else ``allele_table`` + ``around_cut_from_alleles``
* :func:`merge_around_cut_tables` -- around-cut tables of several batches -> one

A resident summary (``summarize_pooled`` / ``summarize_regions``) has no text on the host and its
keep flags and ``nwq_read`` records stay in HBM; there the rows of one read per group are built
on the device too (crispresso_amd/csrc/nw_allele_rows.hip).  These tables are upper case.

* :func:`resident_allele_table`      -- device groups + device rows -> ``df_alleles``
* :func:`resident_around_cut_tables` -- the windows with device keep flags and results, or
  :func:`around_cut_from_alleles` on the resident allele table
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

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


@dataclass
class WindowGroups:
    """Groups of the kept reads' windows around one cut point, in order of first appearance."""

    win: np.ndarray                        # uint8 [groups][2][2 * offset]: aligned-read row, reference row, zero-padded
    win_len: np.ndarray                    # int32 [groups]
    first: np.ndarray                      # int64 [groups]
    count: np.ndarray                      # int64 [groups]
    unedited: np.ndarray                   # uint8 [groups]: a read of the group is UNMODIFIED
    group_of_read: Optional[np.ndarray]    # int32 [n] (-1: not kept), when asked for
    collided: int = 0                      # records of the call the device pass left to the host

    def __len__(self) -> int:
        return len(self.first)


@dataclass
class AlleleRows:
    """One representative per group of identical kept reads of a resident batch, in order of
    first appearance (nwa_table_device)."""

    rows: np.ndarray                       # uint8 [groups][2][row_stride]: aligned-read row, reference row, zero-padded
    cols: np.ndarray                       # int32 [groups]: min(aln_len, awidth) of the group's first read
    first: np.ndarray                      # int64 [groups]
    count: np.ndarray                      # int64 [groups]
    results: np.ndarray                    # int32 [groups][4]: the first read's nwq_read
    collided: int = 0                      # reads the device pass left to the host

    def __len__(self) -> int:
        return len(self.first)


def _results_array(read_results, n: int) -> np.ndarray:
    """The ``[n][4]`` int32 array of ``nwq_read`` from it or from its structured form."""
    rr = np.asarray(read_results)
    if rr.dtype.names:
        rr = np.ascontiguousarray(rr).view(np.int32)
    rr = np.ascontiguousarray(rr, dtype=np.int32).reshape(-1, 4)
    if len(rr) != n:
        raise AlleleError(f"{len(rr)} read results for {n} reads")
    return rr


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

    def window_times(self) -> Dict[str, float]:
        """Device ms of the last :meth:`windows` by phase (summed over its cut points)."""
        ms = np.zeros(3, np.float32)
        self._lib.nwa_windows_times(self._ctx, _lib.ptr(ms))
        return dict(zip(("extract", "group", "finish"), (float(x) for x in ms)))

    def windows(self, dev: dict, n: int, awidth: int, amplicon: str, cut_points: Sequence[int], offset: int,
                read_results, keep=None, tag=None, want_group_of_read: bool = False) -> List[WindowGroups]:
        """The window groups of a device-resident batch, one :class:`WindowGroups` per cut point
        (nwa_windows_device): ``dev`` is ``GpuAligner.device_ops()``.  Raises :class:`AlleleError`
        when a kept read's columns do not hold a cut point (the reference's ``ValueError``) or the
        arguments are outside what the device path takes (:func:`windows_on_device`)."""
        n = int(n)
        keep, tag = _host_arrays(n, keep, tag)
        rr = _results_array(read_results, n)
        return self._windows("nwa_windows_device", dev, n, awidth, amplicon, cut_points, offset, _lib.ptr(keep), tag,
                             _lib.ptr(rr), want_group_of_read)

    def windows_resident(self, dev: dict, n: int, awidth: int, amplicon: str, cut_points: Sequence[int], offset: int,
                         d_keep: int, d_results: int, tag=None, want_group_of_read: bool = False) -> List[WindowGroups]:
        """:meth:`windows` with the keep flags and the ``nwq_read`` records in HBM
        (nwa_windows_resident): ``d_keep`` (uint8 ``[n]``, non-zero = kept, or 0 for all) and
        ``d_results`` are device pointers, as a resident summary leaves them."""
        n = int(n)
        _, tag = _host_arrays(n, None, tag)
        return self._windows("nwa_windows_resident", dev, n, awidth, amplicon, cut_points, offset, int(d_keep or 0), tag,
                             int(d_results or 0), want_group_of_read)

    def _windows(self, entry: str, dev: dict, n: int, awidth: int, amplicon: str, cut_points, offset: int, keep: int,
                 tag, results: int, want_group_of_read: bool) -> List[WindowGroups]:
        cuts = np.ascontiguousarray(cut_points, dtype=np.int32)
        ng = np.zeros(max(len(cuts), 1), np.int64)
        bad, first_bad = ctypes.c_int64(), ctypes.c_int64()
        amp = amplicon.encode("ascii")
        rc = getattr(self._lib, entry)(self._ctx, dev["ops"], dev["ops_off"], dev["stats"], dev["reads"],
                                       dev["offsets"], int(dev["reads_bias"]), n, int(awidth), amp, len(amp),
                                       _lib.ptr(cuts), len(cuts), int(offset), keep, _lib.ptr(tag),
                                       results, int(want_group_of_read), _lib.ptr(ng), ctypes.byref(bad),
                                       ctypes.byref(first_bad))
        if rc != 0:
            msg = self._lib.nwa_last_error(self._ctx).decode(errors="replace")
            raise AlleleError(f"{entry} failed ({rc}): {msg}")
        if bad.value:
            raise AlleleError(f"{bad.value} kept reads have no column for the cut point in their first "
                              f"min(aln_len, awidth) columns; the first is read {first_bad.value}")
        collided = int(self._lib.nwa_windows_collided(self._ctx))
        out = []
        for k in range(len(cuts)):
            g = int(ng[k])
            w = WindowGroups(np.zeros((g, 2, 2 * int(offset)), np.uint8), np.zeros(g, np.int32), np.zeros(g, np.int64),
                             np.zeros(g, np.int64), np.zeros(g, np.uint8),
                             np.empty(n, np.int32) if want_group_of_read else None, collided)
            rc = self._lib.nwa_windows_fetch(self._ctx, k, _lib.ptr(w.win), _lib.ptr(w.win_len), _lib.ptr(w.first),
                                             _lib.ptr(w.count), _lib.ptr(w.unedited), _lib.ptr(w.group_of_read))
            if rc != 0:
                raise AlleleError(f"nwa_windows_fetch({k}) failed ({rc})")
            out.append(w)
        return out

    def table_times(self) -> Dict[str, float]:
        """Device ms of the last :meth:`table` by phase."""
        ms = np.zeros(2, np.float32)
        self._lib.nwa_table_times(self._ctx, _lib.ptr(ms))
        return dict(zip(("group", "rows"), (float(x) for x in ms)))

    def table(self, dev: dict, n: int, awidth: int, amplicon: str, d_keep: int, d_results: int) -> AlleleRows:
        """The representative rows of a device-resident batch whose keep flags and ``nwq_read``
        records are in HBM as well (nwa_table_device): ``dev`` is ``GpuAligner.device_ops()``,
        ``d_keep`` (uint8 ``[n]``, non-zero = kept, or 0 for all) and ``d_results`` are device
        pointers.  The kept reads are grouped by their bytes and one wavefront per group builds
        the two rows of its first read in HBM; only the groups' rows come back.  The bytes are
        upper case, as the whole resident path is.  Raises :class:`AlleleError` when a
        representative's runs do not match its bytes or the amplicon."""
        n = int(n)
        amp = amplicon.encode("ascii")
        ng, stride = ctypes.c_int64(), ctypes.c_int32()
        rc = self._lib.nwa_table_device(self._ctx, dev["ops"], dev["ops_off"], dev["stats"], dev["reads"], dev["offsets"],
                                        int(dev["reads_bias"]), n, int(awidth), amp, len(amp), int(d_keep or 0),
                                        int(d_results or 0), ctypes.byref(ng), ctypes.byref(stride))
        if rc != 0:
            msg = self._lib.nwa_last_error(self._ctx).decode(errors="replace")
            raise AlleleError(f"nwa_table_device failed ({rc}): {msg}")
        g, w = int(ng.value), max(int(stride.value), 16)
        t = AlleleRows(np.zeros((g, 2, w), np.uint8), np.zeros(g, np.int32), np.zeros(g, np.int64), np.zeros(g, np.int64),
                       np.zeros((g, 4), np.int32), int(self._lib.nwa_table_collided(self._ctx)))
        rc = self._lib.nwa_table_fetch(self._ctx, _lib.ptr(t.rows), _lib.ptr(t.cols), _lib.ptr(t.first), _lib.ptr(t.count),
                                       _lib.ptr(t.results))
        if rc != 0:
            raise AlleleError(f"nwa_table_fetch failed ({rc})")
        return t


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


# ------------------------------------------------------------------ the table around a cut site

AROUND_COLUMNS = ["Reference_Sequence", "Unedited", "%Reads", "#Reads"]
WINDOW_MAX_OFFSET = 64          # nwa_windows_device's limits (include/crispr_alleles.h)
WINDOW_MAX_AMPLICON = 16384
_COUNTED = frozenset("ATCGN")


def ref_positions(ref_seq: str) -> List[int]:
    """CORE:2055-2067: a column whose reference byte is one of ``A T C G N`` gets the number of
    such columns before it; every other column (``-``, IUPAC, lower case) gets minus that
    number, or -1 while it is 0."""
    out, idx = [], 0
    for c in ref_seq:
        if c in _COUNTED:
            out.append(idx)
            idx += 1
        else:
            out.append(-idx if idx else -1)
    return out


def _finish_around(aligned, reference, unedited, reads) -> pd.DataFrame:
    """Windows with their counts -> the frame of ``get_dataframe_around_cut`` (CORE:812-836):
    grouped by the two windows, ``#Reads`` summed, ``Unedited`` ORed, ``%Reads`` = ``#Reads`` /
    total * 100, sorted by ``#Reads`` descending, then the two windows ascending (the reference
    sorts by ``%Reads`` with an unstable sort: its order of ties is undefined)."""
    frame = pd.DataFrame({"Aligned_Sequence": np.asarray(aligned, dtype=object),
                          "Reference_Sequence": np.asarray(reference, dtype=object),
                          "Unedited": np.asarray(unedited, dtype=bool),
                          "#Reads": np.asarray(reads, dtype=np.int64)})
    g = frame.groupby(["Aligned_Sequence", "Reference_Sequence"], sort=True).agg({"Unedited": "any", "#Reads": "sum"})
    g = g.reset_index()
    g["Unedited"] = g["Unedited"].astype(bool)
    g["#Reads"] = g["#Reads"].astype(np.int64)
    total = int(g["#Reads"].sum())
    g["%Reads"] = g["#Reads"] / total * 100.0 if total else g["#Reads"].astype(np.float64)
    g = g.sort_values(by=["#Reads", "Aligned_Sequence", "Reference_Sequence"], ascending=[False, True, True],
                      kind="stable")
    return g.set_index("Aligned_Sequence")[AROUND_COLUMNS]


def around_cut_from_alleles(df_alleles: pd.DataFrame, cut_point: int, offset: int) -> pd.DataFrame:
    """``get_dataframe_around_cut(df_alleles, cut_point, offset)`` (CORE:801-836) on a
    ``df_alleles`` as :func:`allele_table` returns it; no GPU.  ``ref_positions`` comes from
    ``Reference_Sequence`` (:func:`ref_positions`); the cut column is the first whose value is
    ``cut_point``, and the window is ``s[cut_idx - offset + 1 : cut_idx + offset + 1]`` under
    Python's slice rules, as the reference writes it.  An allele without such a column (its
    reference row was cut before it) is the reference's ``ValueError``: :class:`AlleleError`."""
    cut_point, offset = int(cut_point), int(offset)
    aligned = df_alleles["Aligned_Sequence"].tolist()
    reference = df_alleles["Reference_Sequence"].tolist()
    cut_of: Dict[str, int] = {}
    wa, wr = [], []
    for q, (a, r) in enumerate(zip(aligned, reference)):
        cut_idx = cut_of.get(r)
        if cut_idx is None:
            try:
                cut_idx = ref_positions(r).index(cut_point)
            except ValueError:
                raise AlleleError(f"allele {q} ({a[:40]!r}...) has no column for cut point {cut_point} in its "
                                  f"{len(r)} reference columns") from None
            cut_of[r] = cut_idx
        lo, hi = cut_idx - offset + 1, cut_idx + offset + 1
        wa.append(a[lo:hi])
        wr.append(r[lo:hi])
    return _finish_around(wa, wr, df_alleles["UNMODIFIED"].to_numpy(dtype=bool), df_alleles["#Reads"].to_numpy())


def merge_around_cut_tables(tables: Sequence[pd.DataFrame]) -> pd.DataFrame:
    """One around-cut table from the tables of several batches for the same cut point and
    offset (forward + RC retry, shards, pooled parts): ``#Reads`` summed, ``Unedited`` ORed,
    ``%Reads`` recomputed, sorted again."""
    tables = [t.reset_index() for t in tables if t is not None and len(t)]
    if not tables:
        return _finish_around([], [], [], [])
    t = pd.concat(tables, ignore_index=True)
    return _finish_around(t["Aligned_Sequence"], t["Reference_Sequence"], t["Unedited"], t["#Reads"])


def windows_on_device(amplicon: str, cut_points: Sequence[int], offset: int) -> bool:
    """Whether nwa_windows_device takes these: 1 <= offset <= 64, every cut point inside the
    amplicon, an amplicon of upper-case ``A C G T N`` only that fits the kernel's LDS."""
    return (1 <= int(offset) <= WINDOW_MAX_OFFSET and 0 < len(amplicon) <= WINDOW_MAX_AMPLICON and
            set(amplicon) <= set("ACGTN") and all(0 <= int(c) < len(amplicon) for c in cut_points))


def around_cut_tables(aligner, amplicon: str, buf: np.ndarray, offsets: np.ndarray, read_results,
                      cut_points: Sequence[int], offset: int = 20, keep=None, tag=None, *, ops_batch=None,
                      dev: Optional[dict] = None, nthreads: int = 0) -> List[pd.DataFrame]:
    """``Alleles_frequency_table_around_cut_site_for_<sgRNA>`` (CORE:3642-3657) for every cut
    point: one frame per cut point in the form of :func:`around_cut_from_alleles`.

    From the device (crispresso_amd/csrc/nw_windows.hip), with strings for the window groups
    only, when ``aligner`` holds the batch resident (``device_ops()``; or ``dev`` gives the
    device arrays of a pass that left none, e.g. a pooled one), no read has a lowercase byte
    and :func:`windows_on_device` holds.  Otherwise :func:`allele_table` +
    :func:`around_cut_from_alleles` on ``ops_batch`` (default: ``aligner.download_ops``).
    ``read_results``: the ``[n][4]`` ``nwq_read`` array; ``keep`` / ``tag`` as
    :func:`group_reads` takes them."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    n = len(offsets) - 1
    keep, tag = _host_arrays(n, keep, tag)
    rr = _results_array(read_results, n)
    cuts = [int(c) for c in cut_points]
    kept = np.ones(n, bool) if keep is None else keep != 0
    if not kept.any():
        return [_finish_around([], [], [], []) for _ in cuts]
    if (rr[kept, 0] < 0).any():
        bad = np.flatnonzero(kept & (rr[:, 0] < 0))[:5].tolist()
        raise AlleleError(f"reads are not aligned to the amplicon (LEN_AMPLICON bases): {bad}")
    device = getattr(aligner, "device", 0) if aligner is not None else 0
    awidth = ops_batch.awidth if ops_batch is not None else getattr(getattr(aligner, "options", None), "awidth", None)
    if awidth is not None and windows_on_device(amplicon, cuts, offset) and not reads_have_lower(buf, offsets):
        if dev is None and aligner is not None and hasattr(aligner, "device_ops"):
            from .aligner import NeedleError

            try:
                dev = aligner.device_ops()
            except NeedleError:      # no resident ops-mode batch
                dev = None
        if dev is not None:
            from .needle import _rows_to_str

            out = []
            for w in default_grouper(device).windows(dev, n, awidth, amplicon, cuts, offset, rr, keep, tag):
                lens = w.win_len.astype(np.int64)
                out.append(_finish_around(_rows_to_str(w.win[:, 0, :], lens), _rows_to_str(w.win[:, 1, :], lens),
                                          w.unedited, w.count))
            return out
    if ops_batch is None:
        if aligner is None or not hasattr(aligner, "download_ops"):
            raise AlleleError("the host path needs the batch's OpsBatch (ops_batch) or an aligner that holds it")
        ops_batch = aligner.download_ops(n)
    groups = group_reads_host(buf, offsets, keep, tag) if dev is not None else group_reads(aligner, buf, offsets, keep, tag)
    table = allele_table(amplicon, buf, offsets, ops_batch, rr, groups, nthreads)
    return [around_cut_from_alleles(table, c, offset) for c in cuts]


# ------------------------------------------------------------------ from a resident summary: no text on the host

def resident_allele_table(dev: dict, n: int, awidth: int, amplicon: str, d_keep: int, d_results: int,
                          device: int = 0, grouper: Optional[GpuAlleleGrouper] = None) -> pd.DataFrame:
    """:func:`allele_table` of a resident batch whose reads, keep flags and ``nwq_read`` records
    never left HBM (a group of :func:`crispresso_amd.demux.summarize_pooled` or
    :func:`crispresso_amd.regions.summarize_regions` after its quantifier pass): ``dev`` is
    ``GpuAligner.device_ops()``, ``d_keep`` / ``d_results`` are device pointers.

    :meth:`GpuAlleleGrouper.table` groups the kept reads by their bytes and builds the two rows of
    one read per group in HBM; the strings are made of those rows here, NHEJ / UNMODIFIED / HDR
    come from ``cls`` as :func:`allele_table` maps them, and the reference's own last steps
    finish the frame.  Byte-identical reads against one amplicon (or amplicon + Expected_HDR pair)
    have identical runs, flags and ``nwq_read``, and the resident paths never retry a read
    reverse-complemented, so the byte groups are the reference's groups.  The resident bytes are
    upper case, as the whole resident path is: a lower-case input base shows upper case here."""
    t = (grouper or default_grouper(device)).table(dev, n, awidth, amplicon, d_keep, d_results)
    if not len(t):
        return merge_allele_tables([])
    res = t.results
    cls = res[:, 0]
    if (cls < 0).any():
        raise AlleleError(f"reads are not aligned to the amplicon (LEN_AMPLICON bases): {t.first[cls < 0][:5].tolist()}")
    stride = t.rows.shape[2]
    cols = t.cols.tolist()
    seq_rows = t.rows[:, 0, :].tobytes()
    ref_rows = t.rows[:, 1, :].tobytes()
    frame = pd.DataFrame({
        "Aligned_Sequence": [seq_rows[q * stride:q * stride + c].decode("ascii") for q, c in enumerate(cols)],
        "Reference_Sequence": [ref_rows[q * stride:q * stride + c].decode("ascii") for q, c in enumerate(cols)],
        "NHEJ": cls == 1, "UNMODIFIED": cls == 0, "HDR": cls == 2,
        "n_deleted": res[:, 3].astype(np.int64), "n_inserted": res[:, 2].astype(np.int64),
        "n_mutated": res[:, 1].astype(np.int64),
        "#Reads": t.count.astype(np.int64),
    }, columns=KEYS + ["#Reads"])
    return _finish(frame)


def resident_around_cut_tables(dev: dict, n: int, awidth: int, amplicon: str, cut_points: Sequence[int], offset: int,
                               d_keep: int, d_results: int, table: Optional[pd.DataFrame] = None, device: int = 0,
                               grouper: Optional[GpuAlleleGrouper] = None) -> List[pd.DataFrame]:
    """:func:`around_cut_tables` of a resident batch whose keep flags and ``nwq_read`` records
    are in HBM: one frame per cut point in the form of :func:`around_cut_from_alleles`.  Through
    nwa_windows_resident when :func:`windows_on_device` holds; otherwise
    :func:`around_cut_from_alleles` on ``table``, the batch's :func:`resident_allele_table`
    (made here when not given).  Neither way needs a read's text.  Upper case, as
    :func:`resident_allele_table` explains."""
    cuts = [int(c) for c in cut_points]
    if not cuts:
        return []
    if windows_on_device(amplicon, cuts, offset):
        out = []
        g = grouper or default_grouper(device)
        for w in g.windows_resident(dev, n, awidth, amplicon, cuts, offset, d_keep, d_results):
            lens = w.win_len.tolist()
            width = w.win.shape[2]
            a_rows, r_rows = w.win[:, 0, :].tobytes(), w.win[:, 1, :].tobytes()
            out.append(_finish_around([a_rows[q * width:q * width + c].decode("ascii") for q, c in enumerate(lens)],
                                      [r_rows[q * width:q * width + c].decode("ascii") for q, c in enumerate(lens)],
                                      w.unedited, w.count))
        return out
    if table is None:
        table = resident_allele_table(dev, n, awidth, amplicon, d_keep, d_results, device, grouper)
    return [around_cut_from_alleles(table, c, offset) for c in cuts]
