"""Adapter trimming on the GPU with Trimmomatic 0.33 ILLUMINACLIP + MINLEN semantics.

CRISPResso runs the external Trimmomatic program on paired-end input before the
merge when ``--trim_sequences`` is given (``CRISPResso/CRISPRessoCORE.py:1620-1640``)::

    java -jar trimmomatic-0.33.jar PE -phred33 R1 R2 fp fu rp ru <--trimmomatic_options_string>

with the default options ``ILLUMINACLIP:<data>/NexteraPE-PE.fa:0:90:10:0:true MINLEN:40``
(``CORE:4113-4117``).  This module is that step in-process: :func:`trim_pairs` clips
packed read pairs through the C ABI ``nwt_trim_batch`` (``include/crispr_trim.h``, kernel
``crispresso_amd/csrc/trim_clip.hip``); :func:`run_trimmomatic_pe` reads the two FASTQ
files and writes Trimmomatic's four output files.  Steps other than ILLUMINACLIP and
MINLEN are refused (:class:`UnsupportedTrimStep`), not ignored.  There is no CPU
fallback: without the library or a GPU every call raises
:class:`crispresso_amd._lib.NativeLibraryError`.
"""
from __future__ import annotations

import ctypes
import gzip
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from .flash import _pack, read_fastq

ROLE_COMMON, ROLE_READ1, ROLE_READ2 = 0, 1, 2


class TrimError(RuntimeError):
    """A failed trim (the message is the library's)."""


class UnsupportedTrimStep(ValueError):
    """A Trimmomatic step this module does not implement (the message names it)."""


def read_adapter_fasta(path: str) -> List[Tuple[str, bytes]]:
    """(name up to the first blank, upper-cased sequence) of each FASTA record."""
    recs: List[Tuple[str, bytes]] = []
    name, seq = None, []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                if name is not None:
                    recs.append((name, "".join(seq).encode()))
                name, seq = (line[1:].split()[0] if len(line) > 1 else ""), []
            elif line:
                seq.append(line.upper())
    if name is not None:
        recs.append((name, "".join(seq).encode()))
    return recs


@dataclass
class TrimOptions:
    """ILLUMINACLIP's fields and adapters, and MINLEN.  ``adapters`` are the simple-mode
    sequences with their roles (0 both reads, 1 read 1 only, 2 read 2 only);
    ``prefix_pairs`` the palindrome prefixes, each pair cut to the shorter one's length
    from the 3' ends.  Without an ILLUMINACLIP step both lists are empty and only MINLEN
    applies."""
    seed_mismatches: int = 0
    palindrome_threshold: int = 0
    simple_threshold: int = 0
    min_prefix: int = 8
    keep_both: bool = False
    minlen: int = 0
    adapters: List[Tuple[bytes, int]] = field(default_factory=list)
    prefix_pairs: List[Tuple[bytes, bytes]] = field(default_factory=list)

    @property
    def common_adapters(self) -> List[bytes]:
        return [s for s, r in self.adapters if r == ROLE_COMMON]

    def set_adapters(self, records: Sequence[Tuple[str, bytes]]) -> None:
        """Sort FASTA records into roles as Trimmomatic does: names ending ``/1`` clip read 1,
        ``/2`` read 2, others both; a ``Prefix*/1`` + ``Prefix*/2`` pair is a palindrome prefix
        pair; within a role a sequence is used once."""
        fwd: Dict[str, bytes] = {}
        rev: Dict[str, bytes] = {}
        com: Dict[str, bytes] = {}
        fpre, rpre = set(), set()
        for name, seq in records:
            seq = seq.upper()
            if name.endswith("/1"):
                fwd[name] = seq
                if name.startswith("Prefix"):
                    fpre.add(name[:-2])
            elif name.endswith("/2"):
                rev[name] = seq
                if name.startswith("Prefix"):
                    rpre.add(name[:-2])
            else:
                com[name] = seq
        self.prefix_pairs = []
        for p in sorted(fpre & rpre):
            p1, p2 = fwd.pop(p + "/1"), rev.pop(p + "/2")
            m = min(len(p1), len(p2))
            self.prefix_pairs.append((p1[len(p1) - m:], p2[len(p2) - m:]))
        self.adapters = []
        for d, role in ((fwd, ROLE_READ1), (rev, ROLE_READ2), (com, ROLE_COMMON)):
            seen = set()
            for s in d.values():
                if s not in seen:
                    seen.add(s)
                    self.adapters.append((s, role))

    @staticmethod
    def from_steps(steps: Union[str, Sequence[str]]) -> "TrimOptions":
        """The reference's ``--trimmomatic_options_string`` (a string of blank-separated
        steps, or a list of steps): ``ILLUMINACLIP:<fasta>:s:p:t[:minprefix[:keepboth]]`` and
        ``MINLEN:n``.  Any other step raises :class:`UnsupportedTrimStep`."""
        if isinstance(steps, (str, bytes)):
            steps = (steps.decode() if isinstance(steps, bytes) else steps).split()
        o = TrimOptions()
        for st in steps:
            if st.startswith("ILLUMINACLIP:"):
                a = st[len("ILLUMINACLIP:"):].split(":")
                if len(a) < 4:
                    raise UnsupportedTrimStep(f"trim step {st!r}: ILLUMINACLIP needs <fasta>:<seed mismatches>:"
                                              "<palindrome threshold>:<simple threshold>")
                o.seed_mismatches, o.palindrome_threshold, o.simple_threshold = int(a[1]), int(a[2]), int(a[3])
                o.min_prefix = int(a[4]) if len(a) > 4 else 8
                o.keep_both = (a[5].lower() == "true") if len(a) > 5 else False
                o.set_adapters(read_adapter_fasta(a[0]))
            elif st.startswith("MINLEN:"):
                o.minlen = int(st.split(":")[1])
            else:
                raise UnsupportedTrimStep(f"trim step {st!r} is not supported (only ILLUMINACLIP and MINLEN are)")
        return o


@dataclass
class TrimResult:
    keep1: np.ndarray             # int32 [n]: bases of read 1 that survive, 0 = dropped
    keep2: Optional[np.ndarray]   # the same for read 2 (None: single-end)
    kernel_ms: float


def _pack32(items: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(items) + 1, dtype=np.int32)
    np.cumsum([len(x) for x in items], out=off[1:])
    buf = np.frombuffer(b"".join(items), dtype=np.uint8) if items else np.zeros(0, np.uint8)
    return np.ascontiguousarray(buf), off


def trim_pairs(seq1: List[bytes], qual1: List[bytes], seq2: Optional[List[bytes]], qual2: Optional[List[bytes]],
               options: TrimOptions, device: int = 0) -> TrimResult:
    """Clip read pairs (FASTQ sequence and quality lines, as bytes) on the GPU.
    ``seq2=None``: single-end reads (simple mode only)."""
    if seq2 is not None and qual2 is None:
        raise TrimError("trim_pairs: read 2 needs its qualities")
    lists = [seq1, qual1] if seq2 is None else [seq1, qual1, seq2, qual2]
    if len({len(x) for x in lists}) != 1:
        raise TrimError("trim_pairs: the lists must have the same length")
    for seqs, quals in zip(lists[0::2], lists[1::2]):
        for s, q in zip(seqs, quals):
            if len(s) != len(q):
                raise TrimError("trim_pairs: a sequence and its quality line differ in length")
    s1, off1 = _pack(seq1)
    q1, _ = _pack(qual1)
    if seq2 is None:
        return trim_packed(s1, q1, off1, None, None, None, options, device)
    s2, off2 = _pack(seq2)
    q2, _ = _pack(qual2)
    return trim_packed(s1, q1, off1, s2, q2, off2, options, device)


def trim_packed(s1: np.ndarray, q1: np.ndarray, off1: np.ndarray, s2: Optional[np.ndarray],
                q2: Optional[np.ndarray], off2: Optional[np.ndarray], options: TrimOptions,
                device: int = 0) -> TrimResult:
    """trim_pairs on packed inputs: uint8 sequence / quality buffers and int64 offsets
    (n + 1, from 0) per mate; ``s2=None`` for single-end reads."""
    o = options
    paired = s2 is not None
    s1, q1 = (np.ascontiguousarray(x, dtype=np.uint8) for x in (s1, q1))
    off1 = np.ascontiguousarray(off1, dtype=np.int64)
    if len(off1) < 1 or off1[-1] > len(s1) or len(q1) < off1[-1]:
        raise TrimError("trim_packed: offsets do not match the buffers")
    n = len(off1) - 1
    if paired:
        if q2 is None or off2 is None:
            raise TrimError("trim_packed: read 2 needs its qualities and offsets")
        s2, q2 = (np.ascontiguousarray(x, dtype=np.uint8) for x in (s2, q2))
        off2 = np.ascontiguousarray(off2, dtype=np.int64)
        if len(off2) != len(off1) or off2[-1] > len(s2) or len(q2) < off2[-1]:
            raise TrimError("trim_packed: offsets do not match the buffers")
    ad, ad_off = _pack32([s for s, _ in o.adapters])
    roles = np.ascontiguousarray([r for _, r in o.adapters], dtype=np.int32)
    pre, pre_off = _pack32([p for pair in o.prefix_pairs for p in pair])
    keep1 = np.zeros(n, dtype=np.int32)
    keep2 = np.zeros(n, dtype=np.int32) if paired else None
    params = _lib.NwtParams(o.seed_mismatches, o.palindrome_threshold, o.simple_threshold, o.min_prefix,
                            int(o.keep_both), o.minlen)
    ms = ctypes.c_float(0.0)
    lib = _lib.load()
    rc = lib.nwt_trim_batch(device, ctypes.byref(params), _lib.ptr(ad), _lib.ptr(ad_off), _lib.ptr(roles),
                            len(o.adapters), _lib.ptr(pre), _lib.ptr(pre_off), len(o.prefix_pairs),
                            _lib.ptr(s1), _lib.ptr(q1), _lib.ptr(off1),
                            _lib.ptr(s2) if paired else None, _lib.ptr(q2) if paired else None,
                            _lib.ptr(off2) if paired else None, n, _lib.ptr(keep1),
                            _lib.ptr(keep2) if paired else None, ctypes.byref(ms))
    if rc != 0:
        raise TrimError(lib.nwt_last_error().decode())
    return TrimResult(keep1, keep2, float(ms.value))


def _open_out(path: str):
    return gzip.open(path, "wb", compresslevel=1) if path.endswith(".gz") else open(path, "wb")


def run_trimmomatic_pe(r1: str, r2: str, outs: Sequence[str], steps: Union[str, Sequence[str], TrimOptions],
                       device: int = 0) -> Dict[str, int]:
    """Trimmomatic PE's outputs for two FASTQ files: ``outs`` = forward paired, forward
    unpaired, reverse paired, reverse unpaired (gzip-compressed when named ``*.gz``).
    Returns Trimmomatic's summary counts: pairs / both / fwd_only / rev_only / dropped."""
    o = steps if isinstance(steps, TrimOptions) else TrimOptions.from_steps(steps)
    if len(outs) != 4:
        raise TrimError("run_trimmomatic_pe: four output files are needed (fp, fu, rp, ru)")
    n1, s1, q1 = read_fastq(r1)
    n2, s2, q2 = read_fastq(r2)
    n = min(len(s1), len(s2))
    res = trim_pairs(s1[:n], q1[:n], s2[:n], q2[:n], o, device)
    fp, fu, rp, ru = (_open_out(p) for p in outs)
    st = {"pairs": n, "both": 0, "fwd_only": 0, "rev_only": 0, "dropped": 0}
    for i in range(n):
        k1, k2 = int(res.keep1[i]), int(res.keep2[i])
        # an empty read is never clipped away; only MINLEN drops it
        a = k1 > 0 or (len(s1[i]) == 0 and o.minlen <= 0)
        b = k2 > 0 or (len(s2[i]) == 0 and o.minlen <= 0)
        if a and b:
            fp.write(b"@%s\n%s\n+\n%s\n" % (n1[i], s1[i][:k1], q1[i][:k1]))
            rp.write(b"@%s\n%s\n+\n%s\n" % (n2[i], s2[i][:k2], q2[i][:k2]))
            st["both"] += 1
        elif a:
            fu.write(b"@%s\n%s\n+\n%s\n" % (n1[i], s1[i][:k1], q1[i][:k1]))
            st["fwd_only"] += 1
        elif b:
            ru.write(b"@%s\n%s\n+\n%s\n" % (n2[i], s2[i][:k2], q2[i][:k2]))
            st["rev_only"] += 1
        else:
            st["dropped"] += 1
    for f in (fp, fu, rp, ru):
        f.close()
    return st
