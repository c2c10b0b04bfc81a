"""sgRNA counting (``CRISPRessoCount``, CRISPResso/CRISPRessoCountCORE.py:219-227, 305-350) on
the GPU, behind the C ABI of ``include/crispr_count.h``.

Per read the reference runs ``str.find`` of the tracrRNA, slices the ``guide_length`` bytes
before it (Python's slice rule: a tracrRNA closer to the read's start than ``guide_length``
usually gives the empty guide) and increments a dict.  Here the find, the slice and the tally
run in HBM (crispresso_amd/csrc/nw_count.hip); the host finishes with the reference's own three
expressions on the small table of distinct guides.

* :func:`count_guides`     -- reads as packed bytes + offsets -> :class:`GuideCounts`
* :func:`count_fastq`      -- the same from a FASTQ through the native ingest
* :func:`read_guides_file` -- the lines of ``--sgRNA_file``
* ``python -m crispresso_amd.count`` -- the reference's command line and output file

The reads are compared as given (case-sensitive, nothing upper-cased), like the reference.
``sort_values`` in the reference is not stable, so its order of equal counts is not a fact of
the reference; here it is the stable sort over the order of first appearance (no whitelist) or
the file order (whitelist).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import NativeLibraryError

DEFAULT_TRACR = "GTTTTAGAGCTAGAAATAGC"
MAX_PATTERN, MAX_GUIDE = 128, 64
PHASES = ("find", "insert", "publish", "verify_or_lookup", "compact", "upload_wall")


class CountError(RuntimeError):
    """A failed counting call."""


def check_tracr(tracr) -> bytes:
    """The tracrRNA as the reference takes it (stripped, upper-cased; ``find_wrong_nt``)."""
    if isinstance(tracr, bytes):
        tracr = tracr.decode("latin-1")
    t = str(tracr).strip().upper()
    if not t:
        raise ValueError("the tracrRNA is empty")
    wrong = sorted(set(t) - set("ATCGN"))
    if wrong:
        raise ValueError("The tracrRNA sequence contains wrong characters:%s" % " ".join(wrong))
    if len(t) > MAX_PATTERN:
        raise ValueError(f"a tracrRNA of {len(t)} bases: 1 to {MAX_PATTERN} are supported")
    return t.encode("ascii")


def check_guide_length(L) -> int:
    L = int(L)
    if not 0 <= L <= MAX_GUIDE:
        raise ValueError(f"guide length {L}: 0 to {MAX_GUIDE} are supported")
    return L


def _distinct(keys: Sequence[bytes]) -> List[bytes]:
    return list(dict.fromkeys(bytes(k) for k in keys))


def read_guides_file(path: str) -> List[bytes]:
    """The keys of ``--sgRNA_file`` (CountCORE:305-310): every line stripped, duplicates on their
    first position, an empty line the key ``b""``."""
    with open(path, "rb") as f:
        return _distinct(line.strip() for line in f)


@dataclass
class GuideCounts:
    """The tally of one call: the dict of the reference's loop, in its insertion order."""

    guides: List[bytes]
    counts: np.ndarray                     # int64 [groups]
    first: np.ndarray                      # int64 [groups]: smallest read index; -1 for whitelist keys
    n_reads: int
    n_found: int                           # reads that hold the tracrRNA
    n_counted: int                         # reads counted in a group
    pos: Optional[np.ndarray] = None       # int32 [n]: the tracrRNA's position, -1 = absent
    group_of_read: Optional[np.ndarray] = None   # int32 [n]: index into guides, -1 = not counted
    collided: int = 0
    kernel_ms: float = 0.0

    def __len__(self) -> int:
        return len(self.guides)

    def to_frame(self):
        """The reference's table (CountCORE:344-350), its three expressions on the host; equal
        counts keep the order of ``guides`` (a stable sort)."""
        import pandas as pd

        index = pd.Index([g.decode("latin-1") for g in self.guides], dtype=object)
        df = pd.Series(np.asarray(self.counts, dtype=np.int64), index=index, name="Read_Counts").to_frame()
        df.index.name = "Guide_Sequence"
        N_READS = self.n_reads
        with np.errstate(divide="ignore", invalid="ignore"):
            df["Read_%"] = df["Read_Counts"] / N_READS * 100
            df["RPM"] = df["Read_Counts"] / N_READS * 1000000
        return df.sort_values(by="Read_Counts", ascending=False, kind="stable")


class GpuGuideCounter:
    """One ``nwc_ctx`` (one GPU).  Not thread-safe, like the aligner context."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        ctx = ctypes.c_void_p()
        rc = self._lib.nwc_create(int(device), ctypes.byref(ctx))
        if rc != 0:
            raise NativeLibraryError(f"nwc_create(device={device}) failed with code {rc} (no GPU?)")
        self._ctx = ctx
        self.device = device

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.nwc_destroy(self._ctx)
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

    def phase_times(self) -> Dict[str, float]:
        """ms of the last :meth:`count` by phase (device time; ``upload_wall`` on the host)."""
        ms = np.zeros(6, np.float32)
        self._lib.nwc_phase_times(self._ctx, _lib.ptr(ms))
        return dict(zip(PHASES, (float(x) for x in ms)))

    def last_collided(self) -> int:
        return int(self._lib.nwc_last_collided(self._ctx))

    def count(self, text: np.ndarray, offsets: np.ndarray, tracr: bytes, L: int, keys: Optional[List[bytes]],
              want_pos: bool, want_group_of_read: bool) -> GuideCounts:
        lib = self._lib
        n = len(offsets) - 1
        pos = np.empty(n, np.int32) if want_pos else None
        gor = np.empty(n, np.int32) if want_group_of_read else None
        if keys is None:
            wl_bytes = wl_off = None
            n_wl = -1
            cap = min(n, 1 << 16)
        else:
            wl_bytes = np.frombuffer(b"".join(keys) + b"\0", np.uint8)
            wl_off = np.zeros(len(keys) + 1, np.int64)
            np.cumsum([len(k) for k in keys], out=wl_off[1:])
            n_wl = len(keys)
            cap = n_wl
        key_cap = int(wl_off[-1]) if keys is not None else cap * L
        ng, nkb, nf, nc = (ctypes.c_int64() for _ in range(4))
        ms = ctypes.c_float()

        def arrays(cap, key_cap):
            return (np.empty(max(cap, 1), np.int64), np.empty(max(cap, 1), np.int64),
                    np.zeros(max(cap, 1) + 1, np.int64), np.empty(max(key_cap, 1), np.uint8))

        first, count, koff, kbytes = arrays(cap, key_cap)
        rc = lib.nwc_count(self._ctx, _lib.ptr(text), _lib.ptr(offsets), n, tracr, len(tracr), L,
                           _lib.ptr(wl_bytes), _lib.ptr(wl_off), n_wl, _lib.ptr(first), _lib.ptr(count),
                           _lib.ptr(koff), _lib.ptr(kbytes), cap, key_cap, _lib.ptr(pos), _lib.ptr(gor),
                           ctypes.byref(ng), ctypes.byref(nkb), ctypes.byref(nf), ctypes.byref(nc), ctypes.byref(ms))
        if rc == _lib.NW_E_CAPACITY:        # more distinct guides than the first guess: they are kept, fetch them
            cap, key_cap = ng.value, nkb.value
            first, count, koff, kbytes = arrays(cap, key_cap)
            rc = lib.nwc_fetch_groups(self._ctx, _lib.ptr(first), _lib.ptr(count), _lib.ptr(koff), _lib.ptr(kbytes),
                                      cap, key_cap)
        if rc != 0:
            msg = lib.nwc_last_error(self._ctx).decode(errors="replace")
            raise CountError(f"nwc_count failed ({rc}): {msg}")
        g = ng.value
        raw = kbytes.tobytes()
        ko = koff[: g + 1].tolist()
        guides = [raw[ko[i]:ko[i + 1]] for i in range(g)]
        return GuideCounts(guides, count[:g].copy(), first[:g].copy(), n, int(nf.value), int(nc.value), pos, gor,
                           self.last_collided(), float(ms.value))


_DEFAULT: Dict[int, GpuGuideCounter] = {}


def default_counter(device: int = 0) -> GpuGuideCounter:
    c = _DEFAULT.get(device)
    if c is None:
        c = _DEFAULT[device] = GpuGuideCounter(device)
    return c


def count_guides(text, offsets, tracrRNA=DEFAULT_TRACR, guide_length: int = 20, guides=None,
                 counter: Optional[GpuGuideCounter] = None, want_pos: bool = False,
                 want_group_of_read: bool = False) -> GuideCounts:
    """Count the guides of the reads ``text[offsets[r]:offsets[r + 1]]`` (uint8 bytes, int64
    offsets).  ``guides``: the whitelist (``read_guides_file``; raw lines are stripped here too),
    or None to count every guide.  Every refusal is made here, before any GPU call."""
    tracr = check_tracr(tracrRNA)
    L = check_guide_length(guide_length)
    text = np.ascontiguousarray(text, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if offsets.ndim != 1 or len(offsets) < 1:
        raise ValueError("offsets must hold n + 1 values")
    if len(offsets) - 1 > 2 ** 31 - 1:
        raise ValueError("more than 2^31 - 1 reads")
    if len(offsets) > 1 and bool((np.diff(offsets) < 0).any()):
        raise ValueError("offsets do not ascend")
    if int(offsets[0]) < 0 or int(offsets[-1]) > len(text):
        raise ValueError("offsets point outside the text")
    keys = None if guides is None else _distinct(bytes(k).strip() for k in guides)
    return (counter or default_counter()).count(text, offsets, tracr, L, keys, want_pos, want_group_of_read)


def count_fastq(path: str, tracrRNA=DEFAULT_TRACR, guide_length: int = 20, guides=None,
                min_average_read_quality: int = 0, min_single_bp_quality: int = 0,
                counter: Optional[GpuGuideCounter] = None, want_pos: bool = False,
                want_group_of_read: bool = False) -> GuideCounts:
    """:func:`count_guides` over a FASTQ (plain or gzip) through the native ingest
    (``nw_fastq_read_filtered``), with the reference's quality filter when a threshold is set.

    One known difference: the ingest keeps the letters and ``*.~?#+-`` of a sequence line, the
    reference the ``.strip()``ped line; they are equal for every FASTQ whose sequence lines
    hold only those bytes."""
    from . import fastq

    check_tracr(tracrRNA)
    check_guide_length(guide_length)
    _names, text, offsets = fastq.read_fastq_as_fasta(path, int(min_average_read_quality), int(min_single_bp_quality))
    return count_guides(text, offsets, tracrRNA, guide_length, guides, counter, want_pos, want_group_of_read)


def output_paths(fastq_path: str, name: str = "", output_folder: str = "", with_guides: bool = False):
    """(directory, table file) as the reference names them (CountCORE:234-253, 350-359); the
    reference pastes ``args.fastq`` into the file name, which only works for a bare file name,
    so the basename is used here (identical in that case)."""
    base = os.path.basename(fastq_path)
    database_id = name if name else base.replace(".fastq", "").replace(".gz", "")
    out_dir = "CRISPRessoCount_on_%s" % database_id
    if output_folder:
        out_dir = os.path.join(os.path.abspath(output_folder), out_dir)
    fname = "CRISPRessoCount_%s_on_%s.txt" % ("only_ref_guides" if with_guides else "no_ref_guides", base)
    return out_dir, os.path.join(out_dir, fname)


def main(argv=None) -> int:
    import argparse
    import re

    p = argparse.ArgumentParser(prog="python -m crispresso_amd.count", description="CRISPRessoCount parameters",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("-r", "--fastq", type=str, help="fastq file", required=True)
    p.add_argument("-q", "--min_average_read_quality", type=int, default=0,
                   help="Minimum average quality score (phred33) to keep a read")
    p.add_argument("-s", "--min_single_bp_quality", type=int, default=0,
                   help="Minimum single bp score (phred33) to keep a read")
    p.add_argument("-t", "--tracrRNA", default=DEFAULT_TRACR, help="tracr RNA sequence in each read")
    p.add_argument("-f", "--sgRNA_file", type=str, help="sgRNA description file, one sgRNA per line")
    p.add_argument("-n", "--name", help="Output name", default="")
    p.add_argument("-o", "--output_folder", help="", default="")
    p.add_argument("-l", "--guide_length", type=int, default=20,
                   help="Length in bp to extract the sgRNA upstream of the tracrRNA sequence")
    p.add_argument("--keep_intermediate", action="store_true",
                   help="accepted for the reference's command line; no intermediate file is written here")
    args = p.parse_args(argv)
    for f in (args.fastq, args.sgRNA_file):
        if f and not os.path.exists(f):
            p.error(f"cannot open {f}")
    # the reference's clean-up of --name: other characters become "_", runs of "-" / blanks one "-"
    name = args.name.encode("ascii", "ignore").decode("ascii") if args.name else ""
    name = re.sub(r"[-\s]+", "-", re.sub(r"[^\w\s-]", "_", name).strip())
    guides = read_guides_file(args.sgRNA_file) if args.sgRNA_file else None
    res = count_fastq(args.fastq, args.tracrRNA or DEFAULT_TRACR, args.guide_length, guides,
                      args.min_average_read_quality, args.min_single_bp_quality)
    if res.n_reads == 0:
        raise SystemExit("No reads in input or no reads survived the average or single bp quality filtering.")
    out_dir, table = output_paths(args.fastq, name, args.output_folder, guides is not None)
    os.makedirs(out_dir, exist_ok=True)
    res.to_frame().to_csv(table, sep="\t")
    print(f"{res.n_reads} reads, {res.n_found} with the tracrRNA, {res.n_counted} counted in {len(res)} guides: {table}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
