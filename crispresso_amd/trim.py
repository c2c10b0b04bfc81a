"""Read trimming on the GPU with Trimmomatic 0.33 semantics: ILLUMINACLIP, MINLEN, and the
quality and crop steps (LEADING, TRAILING, SLIDINGWINDOW, CROP, HEADCROP, AVGQUAL).

CRISPResso runs the external Trimmomatic program on paired-end input before the
merge when ``--trim_sequences`` is given (``CRISPResso/CRISPRessoCORE.py:1620-1640``)::

    java -jar trimmomatic-0.33.jar PE -phred33 R1 R2 fp fu rp ru <--trimmomatic_options_string>

with the default options ``ILLUMINACLIP:<data>/NexteraPE-PE.fa:0:90:10:0:true MINLEN:40``
(``CORE:4113-4117``).  This module is that step in-process: :func:`trim_pairs` clips
packed read pairs through the C ABI ``nwt_trim_batch`` (``include/crispr_trim.h``, kernel
``crispresso_amd/csrc/trim_clip.hip``); :func:`run_trimmomatic_pe` reads the two FASTQ
files and writes Trimmomatic's four output files, :func:`run_trimmomatic_se` the one
file of SE mode (``CORE:1585-1611``).  A step list with anything but ILLUMINACLIP and MINLEN
in it is a :class:`TrimProgram`: ``nwt_trim_program`` runs the clip kernel and then the steps
kernel (``crispresso_amd/csrc/trim_steps.hip``) on the same device buffers and returns one
window (start, length) per read.  MAXINFO, TOPHRED33/64 and an ILLUMINACLIP after another step
are refused (:class:`UnsupportedTrimStep`), not ignored.  There is no CPU
fallback: without the library or a GPU every call raises
:class:`crispresso_amd._lib.NativeLibraryError`.
"""
from __future__ import annotations

import ctypes
import gzip
import re
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


def _pack_lists(who: str, seq1, qual1, seq2, qual2):
    """FASTQ sequence and quality lines (bytes) -> the packed arguments of the *_packed calls."""
    if seq2 is not None and qual2 is None:
        raise TrimError(f"{who}: read 2 needs its qualities")
    lists = [seq1, qual1] if seq2 is None else [seq1, qual1, seq2, qual2]
    if len({len(x) for x in lists}) != 1:
        raise TrimError(f"{who}: the lists must have the same length")
    for seqs, quals in zip(lists[0::2], lists[1::2]):
        for s, q in zip(seqs, quals):
            if len(s) != len(q):
                raise TrimError(f"{who}: a sequence and its quality line differ in length")
    s1, off1 = _pack(seq1)
    q1, _ = _pack(qual1)
    if seq2 is None:
        return s1, q1, off1, None, None, None
    s2, off2 = _pack(seq2)
    q2, _ = _pack(qual2)
    return s1, q1, off1, s2, q2, off2


def _check_packed(who: str, s1, q1, off1, s2, q2, off2):
    """Packed inputs as contiguous uint8 / int64 arrays, checked against each other."""
    s1, q1 = (np.ascontiguousarray(x, dtype=np.uint8) for x in (s1, q1))
    off1 = np.ascontiguousarray(off1, dtype=np.int64)
    if len(off1) < 1 or off1[-1] > len(s1) or len(q1) < off1[-1]:
        raise TrimError(f"{who}: offsets do not match the buffers")
    if s2 is not None:
        if q2 is None or off2 is None:
            raise TrimError(f"{who}: read 2 needs its qualities and offsets")
        s2, q2 = (np.ascontiguousarray(x, dtype=np.uint8) for x in (s2, q2))
        off2 = np.ascontiguousarray(off2, dtype=np.int64)
        if len(off2) != len(off1) or off2[-1] > len(s2) or len(q2) < off2[-1]:
            raise TrimError(f"{who}: offsets do not match the buffers")
    return s1, q1, off1, s2, q2, off2


def _clip_arguments(o: TrimOptions, minlen: int):
    """The nwt_params / adapter / prefix arguments both entries take, and the arrays they point into."""
    ad, ad_off = _pack32([s for s, _ in o.adapters])
    roles = np.ascontiguousarray([r for _, r in o.adapters], dtype=np.int32)
    pre, pre_off = _pack32([p for pair in o.prefix_pairs for p in pair])
    params = _lib.NwtParams(o.seed_mismatches, o.palindrome_threshold, o.simple_threshold, o.min_prefix,
                            int(o.keep_both), minlen)
    args = (ctypes.byref(params), _lib.ptr(ad), _lib.ptr(ad_off), _lib.ptr(roles), len(o.adapters),
            _lib.ptr(pre), _lib.ptr(pre_off), len(o.prefix_pairs))
    return args, (params, ad, ad_off, roles, pre, pre_off)


def trim_pairs(seq1: List[bytes], qual1: List[bytes], seq2: Optional[List[bytes]], qual2: Optional[List[bytes]],
               options: TrimOptions, device: int = 0) -> TrimResult:
    """Clip read pairs (FASTQ sequence and quality lines, as bytes) on the GPU.
    ``seq2=None``: single-end reads (simple mode only)."""
    return trim_packed(*_pack_lists("trim_pairs", seq1, qual1, seq2, qual2), options, device)


def trim_packed(s1: np.ndarray, q1: np.ndarray, off1: np.ndarray, s2: Optional[np.ndarray],
                q2: Optional[np.ndarray], off2: Optional[np.ndarray], options: TrimOptions,
                device: int = 0) -> TrimResult:
    """trim_pairs on packed inputs: uint8 sequence / quality buffers and int64 offsets
    (n + 1, from 0) per mate; ``s2=None`` for single-end reads."""
    paired = s2 is not None
    s1, q1, off1, s2, q2, off2 = _check_packed("trim_packed", s1, q1, off1, s2, q2, off2)
    n = len(off1) - 1
    keep1 = np.zeros(n, dtype=np.int32)
    keep2 = np.zeros(n, dtype=np.int32) if paired else None
    clip_args, _alive = _clip_arguments(options, options.minlen)
    ms = ctypes.c_float(0.0)
    lib = _lib.load()
    rc = lib.nwt_trim_batch(device, *clip_args, _lib.ptr(s1), _lib.ptr(q1), _lib.ptr(off1),
                            _lib.ptr(s2) if paired else None, _lib.ptr(q2) if paired else None,
                            _lib.ptr(off2) if paired else None, n, _lib.ptr(keep1),
                            _lib.ptr(keep2) if paired else None, ctypes.byref(ms))
    if rc != 0:
        raise TrimError(lib.nwt_last_error().decode())
    return TrimResult(keep1, keep2, float(ms.value))


def _open_out(path: str):
    return gzip.open(path, "wb", compresslevel=1) if path.endswith(".gz") else open(path, "wb")


STEP_OPS = {"LEADING": 1, "TRAILING": 2, "SLIDINGWINDOW": 3, "CROP": 4, "HEADCROP": 5, "AVGQUAL": 6, "MINLEN": 7}
MAX_STEPS = 16          # NWT_MAX_STEPS
MAX_STEP_ARG = 1 << 20  # NWT_MAX_STEP_ARG
MAX_STEP_QUAL = 1000    # NWT_MAX_STEP_QUAL
_QUALITY_STEPS = ("LEADING", "TRAILING", "AVGQUAL")
_INT = re.compile(r"[0-9]+\Z")
_DEC = re.compile(r"([0-9]+\.?[0-9]*|\.[0-9]+)\Z")


@dataclass(frozen=True)
class TrimStep:
    """One step after the clip: ``arg`` is the threshold, the length, or SLIDINGWINDOW's window;
    ``r`` SLIDINGWINDOW's required quality (a float32 in the kernel, as ``Float.parseFloat``)."""
    name: str
    arg: int
    r: float = 0.0


def _split_steps(steps: Union[str, bytes, Sequence[str]]) -> List[str]:
    if isinstance(steps, (str, bytes)):
        return (steps.decode() if isinstance(steps, bytes) else steps).split()
    return list(steps)


@dataclass
class TrimProgram:
    """A ``--trimmomatic_options_string``: an optional leading ILLUMINACLIP (``clip``, its
    ``minlen`` 0) and up to 16 ordered steps."""
    clip: Optional[TrimOptions] = None
    steps: List[TrimStep] = field(default_factory=list)

    @staticmethod
    def from_steps(steps: Union[str, Sequence[str]]) -> "TrimProgram":
        """Parse a string of blank-separated steps or a list of steps.  MAXINFO, TOPHRED33,
        TOPHRED64, unknown names, an ILLUMINACLIP that is not the first step, more than 16 steps
        after it and malformed or out-of-range arguments raise :class:`UnsupportedTrimStep`."""
        prog = TrimProgram()
        for k, st in enumerate(_split_steps(steps)):
            name, _, rest = st.partition(":")
            args = rest.split(":") if rest else []
            if name == "ILLUMINACLIP":
                if k != 0:
                    raise UnsupportedTrimStep(f"trim step {st!r}: ILLUMINACLIP is supported only as the first step, "
                                              "once")
                prog.clip = TrimOptions.from_steps([st])
                continue
            if name not in STEP_OPS:
                raise UnsupportedTrimStep(f"trim step {st!r} is not supported (ILLUMINACLIP, "
                                          + ", ".join(STEP_OPS) + " are)")
            want = 2 if name == "SLIDINGWINDOW" else 1
            if len(args) != want or not _INT.match(args[0]) or len(args[0]) > 8 or int(args[0]) > MAX_STEP_ARG:
                raise UnsupportedTrimStep(f"trim step {st!r}: {name} takes {'<window>:<quality>' if want == 2 else 'one'}"
                                          f" plain decimal integer up to {MAX_STEP_ARG}")
            arg, r = int(args[0]), 0.0
            if name in _QUALITY_STEPS and arg > MAX_STEP_QUAL:
                raise UnsupportedTrimStep(f"trim step {st!r}: a quality threshold above {MAX_STEP_QUAL}")
            if name == "SLIDINGWINDOW":
                if arg == 0:
                    raise UnsupportedTrimStep(f"trim step {st!r}: a window of 0 bases")
                if not _DEC.match(args[1]) or float(args[1]) > MAX_STEP_QUAL:
                    raise UnsupportedTrimStep(f"trim step {st!r}: the required quality must be a plain decimal "
                                              f"number from 0 to {MAX_STEP_QUAL}")
                r = float(np.float32(float(args[1])))
            if len(prog.steps) == MAX_STEPS:
                raise UnsupportedTrimStep(f"trim step {st!r}: more than {MAX_STEPS} steps after ILLUMINACLIP")
            prog.steps.append(TrimStep(name, arg, r))
        return prog

    def native_steps(self):
        arr = (_lib.NwtStep * max(1, len(self.steps)))()
        for k, st in enumerate(self.steps):
            r = np.float32(st.r)
            arr[k] = _lib.NwtStep(STEP_OPS[st.name], st.arg, float(r), float(np.float32(r * np.float32(st.arg))))
        return arr


@dataclass
class TrimWindows:
    """Read i survives as ``seq[start[i] : start[i] + keep[i]]``; ``keep[i] == -1``: dropped."""
    start1: np.ndarray
    keep1: np.ndarray
    start2: Optional[np.ndarray]   # None: single-end
    keep2: Optional[np.ndarray]
    kernel_ms_clip: float
    kernel_ms_steps: float


def trim_program_pairs(seq1: List[bytes], qual1: List[bytes], seq2: Optional[List[bytes]],
                       qual2: Optional[List[bytes]], program: TrimProgram, device: int = 0) -> TrimWindows:
    """:func:`trim_pairs` for a :class:`TrimProgram`: one window per read."""
    return trim_program_packed(*_pack_lists("trim_program_pairs", seq1, qual1, seq2, qual2), program, device)


def trim_program_packed(s1: np.ndarray, q1: np.ndarray, off1: np.ndarray, s2: Optional[np.ndarray],
                        q2: Optional[np.ndarray], off2: Optional[np.ndarray], program: TrimProgram,
                        device: int = 0) -> TrimWindows:
    """:func:`trim_packed` for a :class:`TrimProgram`: one upload, the clip kernel (when the program
    has an ILLUMINACLIP), the steps kernel on the same device buffers."""
    o = program.clip
    if o is not None and o.minlen != 0:
        raise TrimError("trim_program_packed: the clip options' minlen must be 0 (MINLEN is a step)")
    if len(program.steps) > MAX_STEPS:
        raise UnsupportedTrimStep(f"more than {MAX_STEPS} steps after ILLUMINACLIP")
    paired = s2 is not None
    s1, q1, off1, s2, q2, off2 = _check_packed("trim_program_packed", s1, q1, off1, s2, q2, off2)
    n = len(off1) - 1
    out = [np.zeros(n, dtype=np.int32) for _ in range(4 if paired else 2)]
    ms = (ctypes.c_float * 2)(0.0, 0.0)
    lib = _lib.load()
    clip_args, _alive = _clip_arguments(o, 0) if o is not None else ((None, None, None, None, 0, None, None, 0), None)
    rc = lib.nwt_trim_program(device, *clip_args, program.native_steps(), len(program.steps),
                              _lib.ptr(s1), _lib.ptr(q1), _lib.ptr(off1),
                              _lib.ptr(s2) if paired else None, _lib.ptr(q2) if paired else None,
                              _lib.ptr(off2) if paired else None, n, _lib.ptr(out[0]), _lib.ptr(out[1]),
                              _lib.ptr(out[2]) if paired else None, _lib.ptr(out[3]) if paired else None, ms)
    if rc != 0:
        raise TrimError(lib.nwt_last_error().decode())
    return TrimWindows(out[0], out[1], out[2] if paired else None, out[3] if paired else None,
                       float(ms[0]), float(ms[1]))


def _only_clip_and_minlen(steps: Sequence[str]) -> bool:
    return all(st.startswith("ILLUMINACLIP:") or st.startswith("MINLEN:") for st in steps)


def run_trimmomatic_pe(r1: str, r2: str, outs: Sequence[str],
                       steps: Union[str, Sequence[str], TrimOptions, TrimProgram], device: int = 0) -> Dict[str, int]:
    """Trimmomatic PE's outputs for two FASTQ files: ``outs`` = forward paired, forward
    unpaired, reverse paired, reverse unpaired (gzip-compressed when named ``*.gz``).
    Returns Trimmomatic's summary counts: pairs / both / fwd_only / rev_only / dropped.
    A step list of ILLUMINACLIP and MINLEN only (or a :class:`TrimOptions`) is one
    ``nwt_trim_batch`` call; any other is a :class:`TrimProgram`."""
    if len(outs) != 4:
        raise TrimError("run_trimmomatic_pe: four output files are needed (fp, fu, rp, ru)")
    if not isinstance(steps, (TrimOptions, TrimProgram)):
        steps = _split_steps(steps)
        steps = TrimOptions.from_steps(steps) if _only_clip_and_minlen(steps) else TrimProgram.from_steps(steps)
    n1, s1, q1 = read_fastq(r1)
    n2, s2, q2 = read_fastq(r2)
    n = min(len(s1), len(s2))
    st = {"pairs": n, "both": 0, "fwd_only": 0, "rev_only": 0, "dropped": 0}
    if isinstance(steps, TrimProgram):
        w = trim_program_pairs(s1[:n], q1[:n], s2[:n], q2[:n], steps, device)
        fp, fu, rp, ru = (_open_out(p) for p in outs)
        for i in range(n):
            a0, k1, b0, k2 = int(w.start1[i]), int(w.keep1[i]), int(w.start2[i]), int(w.keep2[i])
            if k1 >= 0 and k2 >= 0:
                fp.write(b"@%s\n%s\n+\n%s\n" % (n1[i], s1[i][a0:a0 + k1], q1[i][a0:a0 + k1]))
                rp.write(b"@%s\n%s\n+\n%s\n" % (n2[i], s2[i][b0:b0 + k2], q2[i][b0:b0 + k2]))
                st["both"] += 1
            elif k1 >= 0:
                fu.write(b"@%s\n%s\n+\n%s\n" % (n1[i], s1[i][a0:a0 + k1], q1[i][a0:a0 + k1]))
                st["fwd_only"] += 1
            elif k2 >= 0:
                ru.write(b"@%s\n%s\n+\n%s\n" % (n2[i], s2[i][b0:b0 + k2], q2[i][b0:b0 + k2]))
                st["rev_only"] += 1
            else:
                st["dropped"] += 1
        for f in (fp, fu, rp, ru):
            f.close()
        return st
    o = steps
    res = trim_pairs(s1[:n], q1[:n], s2[:n], q2[:n], o, device)
    fp, fu, rp, ru = (_open_out(p) for p in outs)
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


def run_trimmomatic_se(r1: str, out: str, steps: Union[str, Sequence[str], TrimProgram],
                       device: int = 0) -> Dict[str, int]:
    """Trimmomatic SE (``CORE:1585-1611``): the surviving reads of one FASTQ file to ``out``
    (gzip-compressed when named ``*.gz``).  Returns reads / surviving / dropped.  The caller
    names the single-end adapter file in the ILLUMINACLIP step (the reference substitutes
    ``TruSeq3-SE.fa`` for ``NexteraPE-PE.fa``, ``CORE:1595``)."""
    prog = steps if isinstance(steps, TrimProgram) else TrimProgram.from_steps(steps)
    names, seqs, quals = read_fastq(r1)
    w = trim_program_pairs(seqs, quals, None, None, prog, device)
    st = {"reads": len(seqs), "surviving": 0, "dropped": 0}
    with _open_out(out) as f:
        for i in range(len(seqs)):
            a0, k = int(w.start1[i]), int(w.keep1[i])
            if k >= 0:
                f.write(b"@%s\n%s\n+\n%s\n" % (names[i], seqs[i][a0:a0 + k], quals[i][a0:a0 + k]))
                st["surviving"] += 1
            else:
                st["dropped"] += 1
    return st
