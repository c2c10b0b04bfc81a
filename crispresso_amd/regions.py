"""BAM records to the reads of every target on the GPU, behind the C ABI of
``include/crispr_regions.h``.

Three loops of the reference end here:

* ``CRISPRessoWGS`` (CRISPResso/CRISPRessoWGSCORE.py:166-221, called at :653-703): per region
  ``samtools view | cut`` into Python, per read a list with one entry per base
  (``get_reference_positions``), ``in`` / ``index`` on it and a slice of sequence and qualities;
* ``CRISPRessoPooled``, amplicon mode (CRISPRessoPooledCORE.py:870-878): ``samtools view -F 4 |
  awk`` appends every mapped record to the FASTQ of its reference;
* ``CRISPRessoPooled``, genome mode (CRISPRessoPooledCORE.py:1045-1082): ``samtools view -F 4 | awk |
  sort | awk`` writes one FASTQ per distinct clip-extended span of the mapped records.

Here the BAM is inflated and validated on the host (crispresso_amd/csrc/nw_bam.cpp), the CIGAR
walk, the region lookup and the slices run in HBM (crispresso_amd/csrc/nw_regions.hip), and a
region's reads come back as the packed ``(buf, offsets)`` pair :func:`pooled.align_pooled` takes.

* :func:`read_bam`           -- a BAM file or its bytes (BGZF or uncompressed) -> :class:`BamRecords`
* :func:`records_from_sam`   -- SAM text (what ``samtools view [-h]`` prints) -> :class:`BamRecords`
* :func:`extract_regions`    -- the reads of every ``(chr_id, bpstart, bpend)`` -> :class:`RegionReads`
* :func:`demux_by_reference` -- every mapped record to its reference's set -> :class:`RegionReads`
* :func:`discover_regions`   -- CRISPRessoPooled's genome mode (CRISPRessoPooledCORE.py:1045-1082):
  every distinct clip-extended span of the mapped records and its reads -> :class:`RegionReads`
* :func:`region_sequences`   -- the genome's bases of such regions from a FASTA (host side)
* :func:`extract_regions_resident`, :func:`demux_by_reference_resident`, :func:`discover_regions_resident`
  -- the same calls with the reads left in HBM as the aligner's 2-bit batch (``NWR_PACKED``: packed
  from the BAM's 4-bit codes, no text and no qualities anywhere) -> :class:`ResidentRegionReads`
* :func:`align_regions_resident` -- every target's resident reads adopted by the aligner and aligned
* :func:`summarize_regions`  -- CRISPRessoWGS / genome mode to SAMPLES_QUANTIFICATION_SUMMARY.txt in HBM;
  its rows from :func:`read_wgs_region_file` + :func:`wgs_rows` or from :func:`discovered_rows`
* ``python -m crispresso_amd.regions`` -- one ``.fastq.gz`` per target, or with ``--summary`` that table

The reference's quirk is kept: ``=``, ``X``, ``H`` and ``P`` advance nothing in its walk
(``eqx_as_match=True`` treats ``=`` and ``X`` as ``M``).  The one deliberate difference: a hit of
a record without sequence or qualities (``*`` in SAM text, which the reference slices) is dropped
and counted in ``n_no_seq``.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import gzip
import re
import struct
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import NativeLibraryError

MAX_REGIONS = _lib.NWR_MAX_REGIONS
CIGAR_OPS = "MIDNSHP=X"
SEQ_CODES = "=ACMGRSVTWYHKDBN"


class RegionsError(RuntimeError):
    """A failed read or extraction; ``code`` is the library's return where there is one."""

    def __init__(self, msg: str, code: int = 0):
        super().__init__(msg)
        self.code = code


class _BamOwner:
    """Owns one ``nwr_bam``; freed when the :class:`BamRecords` and every array viewing it are gone."""

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle

    def free(self):
        if getattr(self, "_h", None):
            self._lib.nwr_bam_free(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - runs at garbage collection
        try:
            self.free()
        except Exception:
            pass


class _BamView:
    def __init__(self, owner: _BamOwner, p: int, nbytes: int):
        self._owner = owner
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "version": 3, "data": (p, True)}


class BamRecords:
    """A BAM in host memory: header, references and the validated records (one ``nwr_bam``).
    ``data`` is the uncompressed stream; record ``i`` is ``data[offsets[i]:offsets[i + 1]]``,
    from its ``block_size`` field on."""

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle
        self._owner = _BamOwner(lib, handle)
        self.n = int(lib.nwr_bam_count(handle))
        nb = ctypes.c_int64()
        p = lib.nwr_bam_data(handle, ctypes.byref(nb))
        self.data = self._view(p, nb.value, np.uint8)
        self.offsets = self._view(lib.nwr_bam_offsets(handle), self.n + 1, np.int64)
        n_ref = int(lib.nwr_bam_n_ref(handle))
        p = lib.nwr_bam_ref_names(handle, ctypes.byref(nb))
        names = ctypes.string_at(p, nb.value) if nb.value else b""
        self.ref_names: List[str] = [s.decode("latin-1") for s in names.split(b"\0")[:n_ref]]
        self.ref_lens = self._view(lib.nwr_bam_ref_lens(handle), n_ref, np.int32).copy()
        p = lib.nwr_bam_text(handle, ctypes.byref(nb))
        self.text = ctypes.string_at(p, nb.value) if nb.value else b""

    def _view(self, p, count, dtype) -> np.ndarray:
        if not p or count <= 0:
            return np.zeros(0, dtype)
        # (read-only views whose base keeps the nwr_bam alive: an array outlives this object safely)
        return np.asarray(_BamView(self._owner, p, count * np.dtype(dtype).itemsize)).view(dtype)

    def __len__(self) -> int:
        return self.n

    def close(self) -> None:
        """Frees the records at once: the caller's promise that no view is used after."""
        if getattr(self, "_h", None):
            self.data = self.offsets = None
            self._owner.free()
            self._h = None

    def ref_id(self, name: str) -> int:
        """The index of a reference name, -1 when the BAM has none of that name."""
        if not hasattr(self, "_ref_index"):
            self._ref_index = {}
            for i, s in enumerate(self.ref_names):
                self._ref_index.setdefault(s, i)
        return self._ref_index.get(name, -1)

    def name(self, i: int) -> bytes:
        """The read name of record ``i`` (the bytes before the NUL)."""
        o = int(self.offsets[i])
        l_name = int(self.data[o + 12])
        return self.data[o + 36:o + 36 + l_name].tobytes().split(b"\0")[0]


def read_bam(path_or_bytes) -> BamRecords:
    """Read a BAM from a path or from its bytes: BGZF or an uncompressed BAM stream.  Malformed
    input of any kind raises :class:`RegionsError` with the reader's message."""
    lib = _lib.load()
    h = ctypes.c_void_p()
    err = ctypes.create_string_buffer(512)
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview, np.ndarray)):
        mem = np.frombuffer(bytes(path_or_bytes), np.uint8) if not isinstance(path_or_bytes, np.ndarray) \
            else np.ascontiguousarray(path_or_bytes, dtype=np.uint8)
        rc = lib.nwr_read_bam(None, _lib.ptr(mem) if len(mem) else None, len(mem), ctypes.byref(h), err, len(err))
    else:
        import os

        rc = lib.nwr_read_bam(os.fsencode(path_or_bytes), None, 0, ctypes.byref(h), err, len(err))
    if rc != 0:
        raise RegionsError(f"nwr_read_bam failed ({rc}): {err.value.decode(errors='replace')}")
    return BamRecords(lib, h)


def _reg2bin(beg: int, end: int) -> int:
    """The UCSC bin of [beg, end), 0-based (SAM specification, section 5.3)."""
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


_CIGAR_RE = re.compile(r"(\d+)([MIDNSHP=X])")
_NIBBLE = {c: i for i, c in enumerate(SEQ_CODES)}


def encode_record(qname: bytes, flag: int, ref_id: int, pos: int, mapq: int, cigar: str, seq: str, qual: str,
                  next_ref_id: int = -1, next_pos: int = 0, tlen: int = 0) -> bytes:
    """One BAM record (with its ``block_size``) from SAM fields; ``pos`` 1-based as in SAM text,
    ``seq`` / ``qual`` may be ``*``; no tags."""
    ops = [] if cigar == "*" else _CIGAR_RE.findall(cigar)
    if cigar != "*" and "".join(a + b for a, b in ops) != cigar:
        raise ValueError(f"cannot parse the CIGAR {cigar!r}")
    if len(ops) > 0xFFFF:
        raise ValueError("more than 65535 CIGAR operations")
    s = "" if seq == "*" else seq
    l_seq = len(s)
    codes = [_NIBBLE.get(c.upper(), 15) for c in s] + [0]
    packed = bytes((codes[2 * k] << 4) | codes[2 * k + 1] for k in range((l_seq + 1) // 2))
    if qual == "*":
        q = b"\xff" * l_seq
    else:
        if len(qual) != l_seq:
            raise ValueError("sequence and qualities differ in length")
        q = bytes(ord(c) - 33 for c in qual)
    ref_span = sum(int(a) for a, b in ops if b in "MDN=X")
    name = qname + b"\0"
    if len(name) > 255:
        raise ValueError("a read name longer than 254 bytes")
    body = struct.pack("<iiBBHHHiiii", ref_id, pos - 1, len(name), mapq, _reg2bin(pos - 1, pos - 1 + max(ref_span, 1)),
                       len(ops), flag, l_seq, next_ref_id, next_pos - 1, tlen)
    body += name + b"".join(struct.pack("<I", (int(a) << 4) | CIGAR_OPS.index(b)) for a, b in ops) + packed + q
    return struct.pack("<i", len(body)) + body


def bam_stream(references: Sequence[Tuple[str, int]], records: Iterable[bytes], text: bytes = b"") -> bytes:
    """An uncompressed BAM stream: magic, header text, references, the encoded records."""
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(references))]
    for name, length in references:
        nm = name.encode("latin-1") + b"\0"
        out += [struct.pack("<i", len(nm)), nm, struct.pack("<i", int(length))]
    out.extend(records)
    return b"".join(out)


def records_from_sam(lines, references: Optional[Sequence[Tuple[str, int]]] = None) -> BamRecords:
    """SAM text (an iterable of lines or one string, ``str`` or ``bytes``) as :class:`BamRecords`,
    in the layout a BAM of the same fields has.  The references come from ``references`` (name,
    length), else from the text's ``@SQ`` lines, else from the ``RNAME`` column in order of first
    appearance (length 0).  Optional fields (tags) are not carried over."""
    if isinstance(lines, (bytes, str)):
        lines = lines.splitlines()
    refs: List[Tuple[str, int]] = list(references) if references is not None else []
    index: Dict[str, int] = {}
    for i, (nm, _l) in enumerate(refs):
        index.setdefault(nm, i)
    fixed = references is not None
    header, recs = [], []
    for line in lines:
        if isinstance(line, bytes):
            line = line.decode("latin-1")
        line = line.rstrip("\r\n")
        if not line:
            continue
        if line.startswith("@"):
            header.append(line)
            if line.startswith("@SQ") and references is None:
                f = dict(x.split(":", 1) for x in line.split("\t")[1:] if ":" in x)
                if "SN" in f and f["SN"] not in index:
                    index[f["SN"]] = len(refs)
                    refs.append((f["SN"], int(f.get("LN", 0))))
                fixed = True
            continue
        f = line.split("\t")
        if len(f) < 11:
            raise ValueError(f"a SAM line of {len(f)} fields")

        def rid(nm, same=-1):
            if nm == "*":
                return -1
            if nm == "=":
                return same
            if nm not in index:
                if fixed:
                    raise ValueError(f"reference {nm!r} is not in the header")
                index[nm] = len(refs)
                refs.append((nm, 0))
            return index[nm]

        ref_id = rid(f[2])
        recs.append(encode_record(f[0].encode("latin-1"), int(f[1]), ref_id, int(f[3]), int(f[4]), f[5], f[9], f[10],
                                  rid(f[6], ref_id), int(f[7]), int(f[8])))
    text = ("\n".join(header) + "\n").encode("latin-1") if header else b""
    return read_bam(bam_stream(refs, recs, text))


Region = Tuple  # (chr_id, bpstart, bpend[, name])


def read_region_file(path: str) -> List[Tuple[str, int, int, str]]:
    """The reference's region file (WGSCORE:553-583): tab-separated ``chr_id bpstart bpend
    [Name ...]``, ``#`` starts a comment; a missing name is ``chr_id_bpstart_bpend``."""
    out = []
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].rstrip("\r\n")
            if not line.strip():
                continue
            c = line.split("\t")
            if len(c) < 3 or not c[0] or not c[1].strip() or not c[2].strip():
                continue          # (the reference drops rows without the three columns)
            s, e = int(float(c[1])), int(float(c[2]))
            name = c[3] if len(c) > 3 and c[3] else "_".join(map(str, (c[0], s, e)))
            out.append((c[0], s, e, name))
    if len({r[3] for r in out}) != len(out):
        raise ValueError("The amplicon names should be all distinct!")
    return out


class RegionReads:
    """The reads of every target of one call; target ``g`` in the caller's order."""

    def __init__(self, bam: BamRecords, names: List[str], region_off, src, st, en, toff, text, qual, n_no_seq: int,
                 kernel_ms: float, upload_ms: float, by_reference: bool):
        self.bam, self.target_names = bam, names
        self.region_offsets, self.src, self.st, self.en = region_off, src, st, en
        self.text_offsets, self.text, self.qual = toff, text, qual
        self.n_reads = np.diff(region_off)
        self.n_no_seq, self.kernel_ms, self.upload_ms = n_no_seq, kernel_ms, upload_ms
        self.by_reference = by_reference

    def __len__(self) -> int:
        return len(self.n_reads)

    def _range(self, g: int) -> Tuple[int, int]:
        return int(self.region_offsets[g]), int(self.region_offsets[g + 1])

    def reads(self, g: int):
        """``(buf, offsets)`` of target ``g``: what :func:`pooled.align_pooled` takes."""
        a, b = self._range(g)
        off = self.text_offsets[a:b + 1]
        return self.text[int(off[0]):int(off[-1])], off - off[0]

    def quals(self, g: int):
        a, b = self._range(g)
        off = self.text_offsets[a:b + 1]
        return self.qual[int(off[0]):int(off[-1])], off - off[0]

    def names(self, g: int) -> List[bytes]:
        """The reads' names, built on the host from the record bytes: ``name_k`` for the k-th hit
        of a region (from 1), the plain name by reference."""
        a, b = self._range(g)
        if self.by_reference:
            return [self.bam.name(int(r)) for r in self.src[a:b]]
        return [self.bam.name(int(r)) + b"_%d" % (k + 1) for k, r in enumerate(self.src[a:b])]

    def _fields(self, g: int):
        (tb, off), (qb, _) = self.reads(g), self.quals(g)
        t, q, o = tb.tobytes(), qb.tobytes(), off.tolist()
        return [(nm, t[o[k]:o[k + 1]], q[o[k]:o[k + 1]]) for k, nm in enumerate(self.names(g))]

    def fastq_bytes(self, g: int, order: Optional[Sequence[int]] = None) -> bytes:
        """``@name\\nseq\\n+\\nqual\\n`` per read, the text the reference writes; ``order`` is a
        permutation of the target's reads (:meth:`reference_order`), default: as they are."""
        f = self._fields(g)
        return b"".join(b"@%s\n%s\n+\n%s\n" % f[k] for k in (range(len(f)) if order is None else order))

    def write_fastq_gz(self, g: int, path: str, order: Optional[Sequence[int]] = None) -> int:
        with gzip.open(path, "wb") as f:
            f.write(self.fastq_bytes(g, order))
        return int(self.n_reads[g])

    def strand(self, g: int) -> np.ndarray:
        """``+`` or ``-`` per read of target ``g`` (uint8), from the records' flags on the host:
        ``-`` iff ``(flag % 32) >= 16``, as the reference's ``awk`` decides it."""
        a, b = self._range(g)
        o = self.bam.offsets[self.src[a:b]]
        reverse = (self.bam.data[o + 18] & 16) != 0      # (the flag's low byte)
        return np.where(reverse, np.uint8(ord("-")), np.uint8(ord("+"))).astype(np.uint8)

    def reference_order(self, g: int) -> List[int]:
        """The permutation of target ``g``'s reads that the reference's ``sort`` leaves inside a
        region's file: its last-resort comparison of the whole line -- strand, name, sequence and
        qualities joined by tabs -- bytewise, which is what ``sort`` does under ``LC_ALL=C``
        (another locale gives the reference another order).  Host side; equal lines keep record
        order."""
        s = self.strand(g).tobytes()
        keys = [b"\t".join((s[k:k + 1],) + f) for k, f in enumerate(self._fields(g))]
        return sorted(range(len(keys)), key=keys.__getitem__)


class ResidentRegionReads(RegionReads):
    """The reads of every target of one ``NWR_PACKED`` call, 2-bit packed in HBM as the aligner's
    batch (``include/crispr_regions.h``): everything a :class:`RegionReads` has except ``text``
    and ``qual`` (both ``None``: no base and no quality reaches the host) and the methods that need
    them, which raise :class:`RegionsError`.  Beside that: ``lens`` (uint16 per read),
    ``region_exc`` (int64 ``[targets + 1]``: target ``g``'s slots of the exception list), ``n_exc``,
    ``pack_ms`` (the packer's device time), :meth:`fetch_packed`, :meth:`adopt`, :meth:`close`.
    A context manager; released at :meth:`close` or at garbage collection.  It stays valid after
    the extractor that made it is closed."""

    def __init__(self, lib, res, bam, names, region_off, src, st, en, toff, by_reference: bool):
        super().__init__(bam, names, region_off, src, st, en, toff, None, None, int(res.n_no_seq), float(res.kernel_ms),
                         float(res.upload_ms), by_reference)
        self._lib, self._res = lib, res
        self.lens = np.zeros(len(src), np.uint16)
        self.region_exc = np.zeros(len(region_off), np.int64)
        ne, ms = ctypes.c_int64(), ctypes.c_float()
        rc = lib.nwr_packed_info(ctypes.byref(res), _lib.ptr(self.lens) if len(src) else None, _lib.ptr(self.region_exc),
                                 ctypes.byref(ne), ctypes.byref(ms))
        if rc != 0:
            raise RegionsError(f"nwr_packed_info failed ({rc})")
        self.n_exc, self.pack_ms = int(ne.value), float(ms.value)

    @property
    def closed(self) -> bool:
        return self._res is None

    def close(self) -> None:
        if getattr(self, "_res", None) is not None:
            self._lib.nwr_release(ctypes.byref(self._res))
            self._res = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover - runs at garbage collection
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if self._res is None:
            raise RegionsError("the resident region reads were released")
        return ctypes.byref(self._res)

    def _no_text(self, what: str):
        raise RegionsError(f"{what} needs the reads' bases on the host: these are resident in HBM (packed=True); "
                           "run the call without it for text and qualities")

    def reads(self, g: int):
        self._no_text("reads()")

    def quals(self, g: int):
        self._no_text("quals()")

    def _fields(self, g: int):
        self._no_text("the FASTQ text")

    def fetch_packed(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(packed, exc_pos, exc_byte) of the whole call, copied to the host (for tests)."""
        nbytes = (int(self.text_offsets[-1]) + 3) // 4
        packed = np.zeros(max(nbytes, 1), np.uint8)
        pos, byt = np.empty(self.n_exc, np.int64), np.empty(self.n_exc, np.uint8)
        rc = self._lib.nwr_fetch_packed(self._live(), _lib.ptr(packed), nbytes, _lib.ptr(pos) if self.n_exc else None,
                                        _lib.ptr(byt) if self.n_exc else None, None)
        if rc != 0:
            raise RegionsError(f"nwr_fetch_packed failed ({rc})")
        return packed[:nbytes], pos, byt

    def adopt(self, aligner, g: int) -> int:
        """Make target ``g``'s reads the resident batch of ``aligner`` (ops output, its reference
        set, on this device): ``nwr_adopt_region``.  Returns the target's number of reads."""
        rc = self._lib.nwr_adopt_region(self._live(), aligner._h, int(g))
        if rc != 0:
            msg = aligner.lib.nw_last_error(aligner._h).decode(errors="replace")
            raise RegionsError(f"nwr_adopt_region of target {g} failed ({rc}): the aligner says: {msg}", rc)
        lo, hi = self._range(g)
        aligner.adopted(None, self.text_offsets[lo:hi + 1])
        return hi - lo


class GpuRegionExtractor:
    """One ``nwr_ctx`` (one GPU).  Not thread-safe, like the aligner context."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        ctx = ctypes.c_void_p()
        rc = self._lib.nwr_create(int(device), ctypes.byref(ctx))
        if rc != 0:
            raise NativeLibraryError(f"nwr_create(device={device}) failed with code {rc} (no GPU?)")
        self._ctx = ctx
        self.device = device

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.nwr_destroy(self._ctx)
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

    def extract(self, bam: BamRecords, table: Optional[np.ndarray], names: List[str], flags: int,
                packed: bool = False) -> RegionReads:
        """``nwr_extract``; ``packed=True`` adds ``NWR_PACKED`` and returns a
        :class:`ResidentRegionReads`."""
        lib = self._lib
        res = _lib.NwrResult()
        n_reg = 0 if table is None else len(table)
        if packed:
            flags |= _lib.NWR_PACKED
        rc = lib.nwr_extract(self._ctx, bam._h, _lib.ptr(table) if n_reg else None, n_reg, flags, ctypes.byref(res))
        if rc != 0:
            msg = lib.nwr_last_error(self._ctx).decode(errors="replace")
            raise RegionsError(f"nwr_extract failed ({rc}): {msg}", rc)
        if flags & _lib.NWR_PACKED:
            return self._resident(res, bam, names, bool(flags & _lib.NWR_BY_REFERENCE))
        try:
            arrays = self._fetch(res)
        finally:
            lib.nwr_release(ctypes.byref(res))
        return RegionReads(bam, names, *arrays, int(res.n_no_seq),
                           float(res.kernel_ms), float(res.upload_ms), bool(flags & _lib.NWR_BY_REFERENCE))

    def _fetch(self, res, with_text: bool = True):
        R, H, B = int(res.n_regions), int(res.n_hits), int(res.n_bytes)
        region_off = np.zeros(R + 1, np.int64)
        src, st, en = np.empty(H, np.int64), np.empty(H, np.int32), np.empty(H, np.int32)
        toff = np.zeros(H + 1, np.int64)
        text, qual = (np.empty(B, np.uint8), np.empty(B, np.uint8)) if with_text else (None, None)
        rc = self._lib.nwr_fetch(ctypes.byref(res), _lib.ptr(region_off), _lib.ptr(src), _lib.ptr(st), _lib.ptr(en),
                                 _lib.ptr(toff), _lib.ptr(text) if with_text else None,
                                 _lib.ptr(qual) if with_text else None)
        if rc != 0:
            raise RegionsError(f"nwr_fetch failed ({rc})", rc)
        return region_off, src, st, en, toff, text, qual

    def _resident_from(self, res, bam, names, arrays) -> "ResidentRegionReads":
        try:
            return ResidentRegionReads(self._lib, res, bam, names, *arrays[:5], True)
        except Exception:
            self._lib.nwr_release(ctypes.byref(res))
            raise

    def _resident(self, res, bam, names, by_reference: bool) -> "ResidentRegionReads":
        """The index arrays of a packed result and the result itself, which stays in HBM."""
        try:
            return ResidentRegionReads(self._lib, res, bam, names, *self._fetch(res, False)[:5], by_reference)
        except Exception:
            self._lib.nwr_release(ctypes.byref(res))
            raise

    def discover(self, bam: BamRecords, min_reads: int, flags: int, packed: bool = False) -> RegionReads:
        """``nwr_discover``; ``packed=True`` adds ``NWR_PACKED`` and returns a
        :class:`ResidentRegionReads` with the same extra attributes."""
        lib = self._lib
        res = _lib.NwrResult()
        if packed:
            flags |= _lib.NWR_PACKED
        packed = bool(flags & _lib.NWR_PACKED)
        rc = lib.nwr_discover(self._ctx, bam._h, flags, int(min_reads), ctypes.byref(res))
        if rc != 0:
            msg = lib.nwr_last_error(self._ctx).decode(errors="replace")
            raise RegionsError(f"nwr_discover failed ({rc}): {msg}", rc)
        done = False
        try:
            arrays = self._fetch(res, not packed)
            table = np.zeros(int(res.n_regions), REGION_DTYPE)
            n_records, stats = np.zeros(len(table), np.int64), np.zeros(4, np.int64)
            rc = lib.nwr_fetch_regions(ctypes.byref(res), _lib.ptr(table) if len(table) else None,
                                       _lib.ptr(n_records) if len(table) else None, _lib.ptr(stats))
            if rc != 0:
                raise RegionsError(f"nwr_fetch_regions failed ({rc})", rc)
            done = True
        finally:
            if not (packed and done):
                lib.nwr_release(ctypes.byref(res))
        regs = [(bam.ref_names[int(r)], int(s), int(e)) for r, s, e in zip(table["ref_id"], table["bpstart"], table["bpend"])]
        names = ["REGION_%s_%d_%d" % r for r in regs]
        if packed:
            out = self._resident_from(res, bam, names, arrays)
        else:
            out = RegionReads(bam, names, *arrays, int(res.n_no_seq), float(res.kernel_ms), float(res.upload_ms), True)
        out.regions, out.region_table, out.n_records = regs, table, n_records
        out.n_aligned, out.n_kept, out.n_emitted = int(stats[0]), int(stats[1]), int(stats[2])
        return out


_DEFAULT: Dict[int, GpuRegionExtractor] = {}


def default_extractor(device: int = 0) -> GpuRegionExtractor:
    x = _DEFAULT.get(device)
    if x is None:
        x = _DEFAULT[device] = GpuRegionExtractor(device)
    return x


REGION_DTYPE = np.dtype([("bpstart", "<i8"), ("bpend", "<i8"), ("ref_id", "<i4"), ("reserved", "<i4")])


def region_table(bam: BamRecords, regions: Sequence[Region]) -> Tuple[np.ndarray, List[str]]:
    """The ``nwr_region`` array and the names of ``regions``; a ``chr_id`` the BAM does not have
    gets reference -1, on which no record lies."""
    if len(regions) > MAX_REGIONS:
        raise ValueError(f"{len(regions)} regions: at most {MAX_REGIONS} are supported")
    table = np.zeros(len(regions), REGION_DTYPE)
    names = []
    for g, r in enumerate(regions):
        chr_id, s, e = r[0], int(r[1]), int(r[2])
        table[g] = (s, e, chr_id if isinstance(chr_id, (int, np.integer)) else bam.ref_id(str(chr_id)), 0)
        names.append(str(r[3]) if len(r) > 3 else "_".join(map(str, (chr_id, s, e))))
    return table, names


def extract_regions(bam: BamRecords, regions: Union[str, Sequence[Region]], eqx_as_match: bool = False,
                    device: int = 0, extractor: Optional[GpuRegionExtractor] = None) -> RegionReads:
    """The reads of every region: ``regions`` is a list of ``(chr_id, bpstart, bpend[, name])``
    (``chr_id`` a reference name or index; positions 1-based as in the region file) or the path
    of the reference's region file.  Target ``g`` of the result is ``regions[g]``."""
    if isinstance(regions, str):
        regions = read_region_file(regions)
    table, names = region_table(bam, regions)
    flags = _lib.NWR_EQX_AS_MATCH if eqx_as_match else 0
    return (extractor or default_extractor(device)).extract(bam, table, names, flags)


def demux_by_reference(bam: BamRecords, device: int = 0, extractor: Optional[GpuRegionExtractor] = None) -> RegionReads:
    """Every record with ``flag & 4 == 0`` to the set of its reference, whole, in file order
    (CRISPRessoPooled's amplicon mode); target ``g`` is reference ``g`` of the BAM."""
    return (extractor or default_extractor(device)).extract(bam, None, list(bam.ref_names), _lib.NWR_BY_REFERENCE)


def discover_regions(bam: BamRecords, min_reads: int = 0, eqx_as_match: bool = False, device: int = 0,
                     extractor: Optional[GpuRegionExtractor] = None) -> RegionReads:
    """CRISPRessoPooled's genome mode (CRISPRessoPooledCORE.py:1045-1082): every mapped record's
    clip-extended span ``(chr_id, bpstart, bpend)`` is a region, every distinct span one target
    with the records that have it, whole, in BAM record order.  The walk and its ``=`` / ``X``
    quirk are stated in ``include/crispr_regions.h``.

    The targets come in ascending ``(reference index, bpstart, bpend)`` order, compared as numbers;
    ``target_names[g]`` is ``REGION_<chr>_<bpstart>_<bpend>``, names are plain.  Beside what every
    :class:`RegionReads` has: ``regions`` (a list of ``(chr_id, bpstart, bpend)``, the name of
    the reference and two Python ints, which may be zero or negative), ``region_table`` (the same
    with reference indices, int64 ends), ``n_records`` (int64, the records of every region in the
    whole BAM), ``n_aligned`` (records with ``flag & 0x904 == 0``, the reference's denominator of
    ``n_reads_aligned_%``), ``n_kept`` and ``n_emitted``.

    A region with fewer than ``min_reads`` records is reported (name, key, ``n_records``) but
    its reads are not produced: its range in ``region_offsets`` is empty and ``n_reads`` is 0.
    The reference runs a region iff ``n_reads > min_reads_to_use_region`` in ``ONLY_GENOME`` mode
    (pass that value + 1) and iff ``>=`` in ``AMPLICONS_AND_GENOME`` mode (pass it as it is); its
    default is 1000, the default here emits everything.

    Three deliberate differences from the reference: a record without sequence or qualities is
    dropped and counted in ``n_no_seq``; a mapped record without a reference (``*``) is dropped,
    where the reference writes ``REGION_*_0_0``; reads come in record order, not in the order of
    ``sort``'s whole-line comparison -- :meth:`RegionReads.reference_order` restores that."""
    flags = _lib.NWR_EQX_AS_MATCH if eqx_as_match else 0
    return (extractor or default_extractor(device)).discover(bam, min_reads, flags)


def extract_regions_resident(bam: BamRecords, regions: Union[str, Sequence[Region]], eqx_as_match: bool = False,
                             device: int = 0, extractor: Optional[GpuRegionExtractor] = None) -> ResidentRegionReads:
    """:func:`extract_regions` with the reads left in HBM as the aligner's packed batch
    (``NWR_PACKED``): the same hits, no text and no qualities on the host."""
    if isinstance(regions, str):
        regions = read_region_file(regions)
    table, names = region_table(bam, regions)
    flags = _lib.NWR_EQX_AS_MATCH if eqx_as_match else 0
    return (extractor or default_extractor(device)).extract(bam, table, names, flags, packed=True)


def demux_by_reference_resident(bam: BamRecords, device: int = 0,
                                extractor: Optional[GpuRegionExtractor] = None) -> ResidentRegionReads:
    """:func:`demux_by_reference` with the reads left in HBM (``NWR_PACKED``)."""
    return (extractor or default_extractor(device)).extract(bam, None, list(bam.ref_names), _lib.NWR_BY_REFERENCE,
                                                            packed=True)


def discover_regions_resident(bam: BamRecords, min_reads: int = 0, eqx_as_match: bool = False, device: int = 0,
                              extractor: Optional[GpuRegionExtractor] = None) -> ResidentRegionReads:
    """:func:`discover_regions` with the reads left in HBM (``NWR_PACKED``); ``regions``,
    ``n_records`` and the other attributes of that call are the same."""
    flags = _lib.NWR_EQX_AS_MATCH if eqx_as_match else 0
    return (extractor or default_extractor(device)).discover(bam, min_reads, flags, packed=True)


def align_regions_resident(region_reads: ResidentRegionReads, amplicons: Sequence[str], aligner, *, min_reads: int = 0,
                           on_group=None):
    """Align every target's resident reads to its amplicon where they lie: the counterpart of
    :func:`crispresso_amd.demux.align_demultiplexed_resident` for BAM-fed reads.

    For every target ``g`` with ``n_reads[g] >= max(min_reads, 1)``, in index order:
    ``set_reference(amplicons[g])``, ``region_reads.adopt(aligner, g)`` (device to device), one
    synchronised pass, ``on_group(g, aligner, n)`` while the group is resident, ``download_ops``.

    Returns ``(ops_batches, skipped)``: one :class:`~crispresso_amd.aligner.OpsBatch` per target
    (``None`` for a skipped one) and the skipped indices.  ``aligner`` must be on the reads'
    device; its output mode is ops during the call and restored after."""
    if len(amplicons) != len(region_reads):
        raise ValueError(f"{len(amplicons)} amplicons for {len(region_reads)} targets")
    bound = max(int(min_reads), 1)      # (a target without a read has nothing to adopt)
    keep = [g for g in range(len(amplicons)) if int(region_reads.n_reads[g]) >= bound]
    skipped = [g for g in range(len(amplicons)) if int(region_reads.n_reads[g]) < bound]
    batches: list = [None] * len(amplicons)
    mode = getattr(aligner, "output_mode", "rows")
    aligner.set_output("ops")
    try:
        for g in keep:
            aligner.set_reference(amplicons[g])
            n = region_reads.adopt(aligner, g)
            aligner.run_async()
            aligner.sync()
            if on_group is not None:
                on_group(g, aligner, n)
            batches[g] = aligner.download_ops(n)
    finally:
        aligner.set_output(mode)
    return batches, skipped


class RegionSummary:
    """One :func:`summarize_regions` call: ``counts`` (int64 ``[regions, 16]``, ``nws_summary``'s
    slots, zeros for a region that was not analysed), ``frame`` (the rows of
    SAMPLES_QUANTIFICATION_SUMMARY.txt), ``skipped`` (the indices not analysed), ``kernel_ms``
    (device ms of the flags, quantify and summary kernels, summed over the regions) and
    ``n_reads`` (what ``Reads_total`` reports)."""

    def __init__(self, counts, frame, skipped, kernel_ms, n_reads):
        self.counts, self.frame, self.skipped, self.kernel_ms, self.n_reads = counts, frame, skipped, kernel_ms, n_reads


def summarize_regions(rows: Sequence[dict], region_reads: ResidentRegionReads, aligner, *, min_reads: int = 10,
                      min_identity_score: float = 60.0, window_around_sgrna: int = 1, cleavage_offset: int = -3,
                      exclude_bp_from_left: int = 15, exclude_bp_from_right: int = 15,
                      ignore_substitutions: bool = False, ignore_insertions: bool = False,
                      ignore_deletions: bool = False, hide_mutations_outside_window_NHEJ: bool = False, on_group=None,
                      quantifier=None, summarizer=None, allow_hdr: bool = False,
                      hdr_perfect_alignment_threshold: float = 98.0, reports=None, alleles: bool = False,
                      offset_around_cut: int = 20) -> RegionSummary:
    """A BAM's region reads to SAMPLES_QUANTIFICATION_SUMMARY.txt (CRISPRessoWGS, and
    CRISPRessoPooled's genome mode) with the reads in HBM from the BAM's 4-bit codes to the 16
    counters: what :func:`crispresso_amd.demux.summarize_pooled` is for amplicon mode.

    ``region_reads``: a :class:`ResidentRegionReads` (:func:`extract_regions_resident`,
    :func:`discover_regions_resident`); ``rows[g]`` describes its target ``g`` and needs ``Name``
    and ``Amplicon_Sequence``, ``sgRNA`` and ``Coding_sequence`` are optional (:func:`wgs_rows`,
    :func:`discovered_rows`).  ``aligner`` must be on the reads' device.  Per analysed region:
    ``set_reference``, adoption (device to device), one pass, ``nws_flags``, the quantifier on the
    resident ops, ``nws_summary``, ``on_group(g, aligner, n)``; only 16 integers come back.

    The reference's rules that are kept:

    * a region runs iff ``n_reads >= min_reads`` (CRISPRessoWGSCORE.py:721, default 10 at :304) --
      not CRISPRessoPooled's strict ``>``; for genome mode pass ``min_reads`` as
      :func:`discover_regions` explains;
    * the amplicon is the region's sequence upper-cased and stripped (CRISPRessoCORE.py:1283);
    * a row whose sequence is empty is not analysed and reports ``Reads_total`` 0 (WGSCORE:667);
    * the sgRNA rules of WGSCORE:613-641 are :func:`wgs_rows`' business.

    With ``allow_hdr`` a row's ``Expected_HDR`` (the region file's sixth column; checked by
    :func:`crispresso_amd.demux.checked_expected_hdr`) is used as the reference does with ``-e``:
    the region is adopted and aligned twice, ``nws_printed`` keeps the printed identity to the
    Expected_HDR amplicon and ``nws_flags_dual`` applies the reference's rule on the two printed
    identities with ``hdr_perfect_alignment_threshold``, as ``summarize_pooled`` explains.

    With ``reports``, a callable ``reports(g, report)``, every analysed region also yields a
    :class:`crispresso_amd.report.GroupReport` (the quantifier's totals over the kept reads and
    the size histograms, both made in HBM), as ``summarize_pooled`` explains; ``counts`` and
    ``frame`` are the same with and without it.  With ``alleles`` (needs ``reports``) every
    report also carries the region's allele table and its tables around the cut sites
    (``offset_around_cut`` columns each side), built from the resident batch in HBM without a
    read's text on the host and upper case, as ``summarize_pooled`` explains.

    Deliberate differences: an ``Expected_HDR`` row is refused unless ``allow_hdr``, as in
    ``summarize_pooled``; discovered regions carry no ``Expected_HDR``; there
    is no reverse-complement retry (BAM reads are in reference orientation); hits of records
    without sequence or qualities are dropped (``n_no_seq``); a region without a read is never
    analysed, whatever ``min_reads``.  Errors from the aligner (an amplicon it cannot take) and
    from the quantifier (``MAX_QUANT_AMPLICON`` bases or more) name the region."""
    from . import demux, quantify
    from .aligner import NeedleError

    if alleles and reports is None:
        raise ValueError("alleles=True fills the regions' reports: pass reports as well")
    if not isinstance(region_reads, ResidentRegionReads):
        raise TypeError("summarize_regions takes the resident reads of a packed call (extract_regions_resident)")
    if region_reads.closed:
        raise ValueError("the resident region reads were released")
    if len(rows) != len(region_reads):
        raise ValueError(f"{len(rows)} rows for {len(region_reads)} regions")
    amplicons, hdrs = [], []
    for row in rows:
        amp = str(row.get("Amplicon_Sequence") or "").upper().strip()
        if row.get("Expected_HDR") and not allow_hdr:
            raise ValueError(f"region {row['Name']}: Expected_HDR is given, and dual alignment per region is not built")
        hdrs.append(demux.checked_expected_hdr(row, amp, "region") if allow_hdr and amp else None)
        if len(amp) >= demux.MAX_QUANT_AMPLICON:
            raise ValueError(f"region {row['Name']} has {len(amp)} bases: fewer than {demux.MAX_QUANT_AMPLICON} are "
                             "supported by the quantifier")
        amplicons.append(amp)
    device = int(getattr(aligner, "device", 0))
    for what, stage in (("quantifier", quantifier), ("summarizer", summarizer)):
        if stage is not None and int(stage.device) != device:
            raise ValueError(f"the aligner is on device {device}, the {what} on device {stage.device}")
    q = quantifier or quantify.default_quantifier(device)
    s = summarizer or demux.default_summarizer(device)
    n_reads = [int(n) if amp else 0 for n, amp in zip(region_reads.n_reads, amplicons)]
    bound = max(int(min_reads), 1)
    keep = [g for g in range(len(rows)) if n_reads[g] >= bound]
    skipped = [g for g in range(len(rows)) if n_reads[g] < bound]
    out = np.zeros((len(rows), _lib.NWS_SLOTS), np.int64)

    def prepare(g: int, reference: str) -> int:
        try:
            aligner.set_reference(reference)
            return region_reads.adopt(aligner, g)
        except NeedleError as exc:
            raise NeedleError(f"region {rows[g]['Name']}: {exc}") from None
        except RegionsError as exc:
            raise RegionsError(f"region {rows[g]['Name']}: {exc}", exc.code) from None

    times = demux._summarize_groups(
        rows, amplicons, keep, max((n_reads[g] for g in keep), default=0), prepare, aligner, q, s, out, "region",
        min_identity_score,
        dict(window_around_sgrna=window_around_sgrna, cleavage_offset=cleavage_offset,
             exclude_bp_from_left=exclude_bp_from_left, exclude_bp_from_right=exclude_bp_from_right,
             ignore_substitutions=ignore_substitutions, ignore_insertions=ignore_insertions,
             ignore_deletions=ignore_deletions, hide_mutations_outside_window_NHEJ=hide_mutations_outside_window_NHEJ),
        on_group, hdrs if allow_hdr else None, float(hdr_perfect_alignment_threshold), reports, bool(alleles),
        int(offset_around_cut))
    frame = demux.summary_frame([row["Name"] for row in rows], out, n_reads, skipped)
    return RegionSummary(out, frame, skipped, times, n_reads)


WGS_COLUMNS = ("chr_id", "bpstart", "bpend", "Name", "sgRNA", "Expected_HDR", "Coding_sequence")


def read_wgs_region_file(path: str) -> List[dict]:
    """The reference's region file with all its seven columns (WGSCORE:553-583) as dict rows:
    ``chr_id bpstart bpend Name sgRNA Expected_HDR Coding_sequence``, tab-separated, ``#`` starts
    a comment; missing trailing columns are ``""``, a missing name is ``chr_id_bpstart_bpend``, the
    three sequences upper-cased (``capitalize_sequence``), spaces in a name ``_``.  Names that are
    not all distinct raise, as in :func:`read_region_file`."""
    out = []
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].rstrip("\r\n")
            if not line.strip():
                continue
            c = line.split("\t")
            if len(c) < 3 or not c[0] or not c[1].strip() or not c[2].strip():
                continue          # (the reference drops rows without the three columns)
            c = (c + [""] * len(WGS_COLUMNS))[:len(WGS_COLUMNS)]
            s, e = int(float(c[1])), int(float(c[2]))
            name = c[3] if c[3] else "_".join(map(str, (c[0], s, e)))
            out.append({"chr_id": c[0], "bpstart": s, "bpend": e, "Name": name, "sgRNA": c[4].upper(),
                        "Expected_HDR": c[5].upper(), "Coding_sequence": c[6].upper()})
    if len({r["Name"] for r in out}) != len(out):
        raise ValueError("The amplicon names should be all distinct!")
    for r in out:
        r["Name"] = r["Name"].replace(" ", "_")
    return out


def _reverse_complement(seq: str) -> str:
    return seq.translate(str.maketrans("ACGTNacgtn", "TGCANtgcan"))[::-1]


def checked_guides(sgrna: str, sequence: str) -> str:
    """The sgRNA column after the reference's check (WGSCORE:613-641): every comma-separated
    guide, stripped and upper-cased, must hold only ``ACGTN`` (else ``ValueError``, the
    reference's ``find_wrong_nt`` exception); the column is kept as it is when one of the guides
    or its reverse complement occurs in ``sequence``, else it is ``""``.  The reference searches the
    sequence as ``faidx`` printed it, before its upper-casing, and so does this."""
    if not sgrna:
        return ""
    found = False
    for guide in sgrna.strip().upper().split(","):
        wrong = sorted(set(guide) - set("ATCGN"))
        if wrong:
            raise ValueError("The sgRNA sequence %s contains wrong characters:%s" % (guide, " ".join(wrong)))
        if guide and (guide in sequence or _reverse_complement(guide) in sequence):
            found = True
    return sgrna if found else ""


def wgs_rows(region_rows: Sequence[dict], fasta_path: str) -> List[dict]:
    """The rows :func:`summarize_regions` takes from those of :func:`read_wgs_region_file`: each
    region's sequence from the FASTA (:func:`region_sequences`), upper-cased and stripped as
    ``Amplicon_Sequence`` (CRISPRessoCORE.py:1283; empty for a region outside its contig), the
    sgRNA through :func:`checked_guides`; the other columns as they are."""
    seqs = region_sequences(fasta_path, [(r["chr_id"], r["bpstart"], r["bpend"]) for r in region_rows])
    out = []
    for r, seq in zip(region_rows, seqs):
        row = dict(r)
        row["sgRNA"] = checked_guides(r.get("sgRNA") or "", seq)
        row["Amplicon_Sequence"] = seq.upper().strip()
        out.append(row)
    return out


def discovered_rows(region_reads: RegionReads, fasta_path: str) -> List[dict]:
    """Rows for genome mode from a :func:`discover_regions` result: ``Name`` is
    ``REGION_<chr>_<bpstart>_<bpend>``, the sequence from the FASTA, no guide."""
    seqs = region_sequences(fasta_path, region_reads.regions)
    return [{"chr_id": c, "bpstart": s, "bpend": e, "Name": name, "sgRNA": "", "Expected_HDR": "", "Coding_sequence": "",
             "Amplicon_Sequence": seq.upper().strip()}
            for name, (c, s, e), seq in zip(region_reads.target_names, region_reads.regions, seqs)]


def _fasta_index(fasta_path: str) -> Dict[str, Tuple[int, int, int, int]]:
    """name -> (length, offset of the first base, bases per line, bytes per line): the ``.fai``
    beside the file when there is one, else one pass over the file."""
    import os

    index: Dict[str, Tuple[int, int, int, int]] = {}
    if os.path.exists(fasta_path + ".fai"):
        with open(fasta_path + ".fai") as f:
            for line in f:
                c = line.rstrip("\n").split("\t")
                if len(c) >= 5:
                    index.setdefault(c[0], (int(c[1]), int(c[2]), int(c[3]), int(c[4])))
        return index
    with open(fasta_path, "rb") as f:
        name, at = None, 0
        length = start = bases = width = 0
        for line in f:
            if line.startswith(b">"):
                if name is not None:
                    index.setdefault(name, (length, start, bases, width))
                name = line[1:].split()[0].decode("latin-1") if line[1:].split() else ""
                length, start, bases, width = 0, at + len(line), 0, 0
            elif name is not None:
                body = line.rstrip(b"\r\n")
                if bases == 0 and body:
                    bases, width = len(body), len(line)
                length += len(body)
            at += len(line)
        if name is not None:
            index.setdefault(name, (length, start, bases, width))
    return index


def region_sequences(fasta_path: str, regions: Sequence[Region]) -> List[str]:
    """The genome's bases of every ``(chr_id, bpstart, bpend)``: ``[bpstart, bpend)`` 1-based, which
    is the ``chr:bpstart-(bpend-1)`` that the reference's ``get_region_from_fa`` asks of
    ``samtools faidx``, as stored (no case change).  Host side, a plain (uncompressed) FASTA whose
    sequence lines have one width, as ``faidx`` requires; its ``.fai`` is used when present.

    The interval is cut to ``[1, length]``; a region outside it, or on a name the FASTA does not
    have, gives ``""``.  That cut is this function's choice, not pinned against ``samtools``."""
    index = _fasta_index(fasta_path)
    out = []
    with open(fasta_path, "rb") as f:
        for r in regions:
            entry = index.get(str(r[0]))
            if entry is None:
                out.append("")
                continue
            length, start, bases, width = entry
            a, b = max(int(r[1]), 1) - 1, min(int(r[2]) - 1, length)      # 0-based [a, b)
            if b <= a or bases <= 0:
                out.append("")
                continue
            lo, hi = start + a // bases * width + a % bases, start + (b - 1) // bases * width + (b - 1) % bases + 1
            f.seek(lo)
            out.append(f.read(hi - lo).replace(b"\n", b"").replace(b"\r", b"").decode("latin-1"))
    return out


def _summary_main(args, bam: BamRecords, hdr_options: dict) -> int:
    """``--summary``: SAMPLES_QUANTIFICATION_SUMMARY.txt of the regions of a file (CRISPRessoWGS;
    --min-reads defaults to its 10) or of the discovered ones (genome mode: --min-reads as given).
    With ``--reports`` also a ``CRISPResso_on_<name>`` folder per analysed region with a kept read,
    with ``--alleles`` the allele tables in it."""
    import os

    from . import demux
    from .aligner import GpuAligner

    if args.discover:
        res = discover_regions_resident(bam, args.min_reads, args.eqx_as_match, args.device)
        rows, min_reads = discovered_rows(res, args.genome), args.min_reads
    else:
        region_rows = read_wgs_region_file(args.regions)
        rows = wgs_rows(region_rows, args.genome)
        res = extract_regions_resident(bam, [(r["chr_id"], r["bpstart"], r["bpend"], r["Name"]) for r in region_rows],
                                       args.eqx_as_match, args.device)
        min_reads = args.min_reads or 10
    os.makedirs(args.out, exist_ok=True)
    folders: dict = {}
    refused: list = []
    writer = demux._folder_writer(args.out, folders, refused) if args.reports else None
    with res, GpuAligner(args.device) as aligner:
        tables = dict(alleles=True, offset_around_cut=20 if args.offset_around_cut_to_plot is None
                      else args.offset_around_cut_to_plot) if args.alleles else {}
        summary = summarize_regions(rows, res, aligner, min_reads=min_reads, reports=writer, **tables, **hdr_options)
    demux.write_summary(os.path.join(args.out, "SAMPLES_QUANTIFICATION_SUMMARY.txt"), summary.frame)
    for row, n in zip(rows, summary.n_reads):
        print(f"{row['Name']}\t{n}")
    for g in refused:
        print(f"region {rows[g]['Name']}: no read passed the identity filter, no folder is written")
    return 0


def build_parser():
    import argparse

    p = argparse.ArgumentParser(prog="python -m crispresso_amd.regions",
                                description="The reads of every target region or reference of a BAM, one .fastq.gz each")
    p.add_argument("--bam", required=True, help="BAM file (BGZF or uncompressed)")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--regions", help="region file: chr_id, bpstart, bpend[, name], tab-separated")
    g.add_argument("--by-reference", action="store_true", help="one read set per reference of the BAM")
    g.add_argument("--discover", action="store_true",
                   help="one read set per distinct clip-extended span of the mapped records (CRISPRessoPooled's genome mode)")
    p.add_argument("--eqx-as-match", action="store_true", help="treat the CIGAR operations = and X as M")
    p.add_argument("--min-reads", type=int, default=0, help="with --discover: write only regions with at least N reads")
    p.add_argument("--genome", help="a plain FASTA: with --discover regions.tsv gets the regions' sequences; "
                                    "with --summary the regions' amplicons")
    p.add_argument("--summary", action="store_true",
                   help="with --regions or --discover, and --genome: align and quantify every region in HBM and write "
                        "SAMPLES_QUANTIFICATION_SUMMARY.txt; no FASTQ is written, the bases never reach the host")
    p.add_argument("--reports", action="store_true",
                   help="with --summary: write a CRISPResso_on_<name> folder per analysed region (editing frequencies, "
                        "effect vectors, size histograms), as CRISPRessoCompare reads them")
    p.add_argument("--alleles", action="store_true",
                   help="with --reports: also write Alleles_frequency_table.txt and, per sgRNA, "
                        "Alleles_frequency_table_around_cut_site_for_<sgRNA>.txt into every folder (upper case)")
    p.add_argument("--offset_around_cut_to_plot", type=int, default=None,
                   help="with --alleles: the columns each side of the cut site in the around-cut tables (default 20)")
    p.add_argument("--reference-order", action="store_true",
                   help="with --discover: reads in the order the reference's sort leaves them (C locale)")
    p.add_argument("--out", required=True, help="output directory")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--hdr", action="store_true",
                   help="with --summary: use the region file's Expected_HDR column (align every read to it as well and "
                        "report HDR%% and Mixed_HDR-NHEJ%%); without this option a file with the column filled is refused")
    p.add_argument("--hdr_perfect_alignment_threshold", type=float, default=None,
                   help="with --hdr: the printed identity to the Expected_HDR amplicon from which a read is HDR and not "
                        "mixed (default 98.0)")
    return p


def summary_options(p, args) -> dict:
    """The keyword arguments ``--hdr`` and ``--hdr_perfect_alignment_threshold`` add to the
    ``--summary`` call of :func:`summarize_regions`: none without ``--hdr``.  A usage error
    (``p.error``) for ``--hdr`` without ``--summary`` and for the threshold without ``--hdr``."""
    if args.hdr:
        if not args.summary:
            p.error("--hdr is used only with --summary")
        return {"allow_hdr": True, "hdr_perfect_alignment_threshold":
                98.0 if args.hdr_perfect_alignment_threshold is None else args.hdr_perfect_alignment_threshold}
    if args.hdr_perfect_alignment_threshold is not None:
        p.error("--hdr_perfect_alignment_threshold is used only with --hdr")
    return {}


def main(argv=None) -> int:
    import os

    p = build_parser()
    args = p.parse_args(argv)
    hdr_options = summary_options(p, args)
    if args.reports and not args.summary:
        p.error("--reports is used only with --summary")
    if args.alleles and not args.reports:
        p.error("--alleles is used only with --reports")
    if args.offset_around_cut_to_plot is not None and not args.alleles:
        p.error("--offset_around_cut_to_plot is used only with --alleles")
    if args.summary and not args.genome:
        p.error("--summary needs --genome, the regions' amplicons come from it")
    if args.summary and (args.by_reference or args.reference_order):
        p.error("--summary goes with --regions or --discover, and not with --reference-order")
    if not args.discover and not args.summary and (args.min_reads or args.genome or args.reference_order):
        p.error("--min-reads, --genome and --reference-order go with --discover")
    if args.min_reads < 0:
        p.error("--min-reads must not be negative")
    for f in (args.bam, args.regions, args.genome):
        if f and not os.path.exists(f):
            p.error(f"cannot open {f}")
    bam = read_bam(args.bam)
    if args.summary:
        return _summary_main(args, bam, hdr_options)
    if args.discover:
        res = discover_regions(bam, args.min_reads, args.eqx_as_match, args.device)
        os.makedirs(args.out, exist_ok=True)
        seqs = region_sequences(args.genome, res.regions) if args.genome else None
        with open(os.path.join(args.out, "regions.tsv"), "w") as tsv:
            tsv.write("\t".join(["chr_id", "bpstart", "bpend", "n_reads", "n_reads_aligned_%"] + (["sequence"] if seqs is not None else []))
                      + "\n")
            for t, (name, (chr_id, s, e)) in enumerate(zip(res.target_names, res.regions)):
                n = int(res.n_records[t])
                pct = "%.6g" % (n / float(res.n_aligned) * 100.0) if res.n_aligned else "NA"
                tsv.write("\t".join(map(str, [chr_id, s, e, n, pct] + ([seqs[t]] if seqs is not None else []))) + "\n")
                if n >= args.min_reads:
                    order = res.reference_order(t) if args.reference_order else None
                    res.write_fastq_gz(t, os.path.join(args.out, name.replace(os.sep, "_") + ".fastq.gz"), order)
                    print(f"{name}\t{n}")
        return 0
    if args.by_reference:
        res = demux_by_reference(bam, args.device)
    else:
        res = extract_regions(bam, args.regions, args.eqx_as_match, args.device)
    os.makedirs(args.out, exist_ok=True)
    if len(set(res.target_names)) != len(res.target_names):
        raise SystemExit("the target names are not distinct")
    for t, name in enumerate(res.target_names):
        n = res.write_fastq_gz(t, os.path.join(args.out, name.replace(os.sep, "_") + ".fastq.gz"))
        print(f"{name}\t{n}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
