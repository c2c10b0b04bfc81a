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
* :func:`read_amplicons_file` -- the reference's tab-separated amplicon table
* ``python -m crispresso_amd.demux`` -- FASTQ + amplicon table -> per-amplicon FASTQ files and
  the reference's ``REPORT_READS_ALIGNED_TO_AMPLICONS.txt``

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


def demultiplex_fastq(amplicons_file: str, fastq: str, out_dir: str, *, k: int = 16, min_hits: int = 2,
                      both_strands: bool = True, min_reads_to_use_region: int = 1000, device: int = 0) -> dict:
    """The command line's work; returns what it wrote."""
    from . import ingest

    rows = read_amplicons_file(amplicons_file)
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
    return {"result": res, "rows": rows, "files": files, "unassigned": unassigned, "report": report,
            "unassigned_report": unassigned_report, "regions_to_use": used, "n_reads": len(seqs)}


def main(argv=None) -> int:
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
    args = p.parse_args(argv)
    for f in (args.amplicons_file, args.fastq_r1):
        if not os.path.exists(f):
            p.error(f"cannot open {f}")
    out = demultiplex_fastq(args.amplicons_file, args.fastq_r1, args.output_folder, k=args.k, min_hits=args.min_hits,
                            both_strands=not args.forward_only, min_reads_to_use_region=args.min_reads_to_use_region)
    res = out["result"]
    print(f"{out['n_reads']} reads: {res.n_assigned} assigned to {len(out['rows'])} amplicons, {res.n_tie} ties, "
          f"{res.n_no_hit} without a hit; {len(out['regions_to_use'])} amplicons with more than "
          f"{args.min_reads_to_use_region:g} reads: {out['report']}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
