"""BAM records to the reads of every target on the GPU, behind the C ABI of
``include/crispr_regions.h``.

Two loops of the reference end here:

* ``CRISPRessoWGS`` (CRISPResso/CRISPRessoWGSCORE.py:166-221, called at :653-703): per region
  ``samtools view | cut`` into Python, per read a list with one entry per base
  (``get_reference_positions``), ``in`` / ``index`` on it and a slice of sequence and qualities;
* ``CRISPRessoPooled``, amplicon mode (CRISPRessoPooledCORE.py:870-878): ``samtools view -F 4 |
  awk`` appends every mapped record to the FASTQ of its reference.

Here the BAM is inflated and validated on the host (crispresso_amd/csrc/nw_bam.cpp), the CIGAR
walk, the region lookup and the slices run in HBM (crispresso_amd/csrc/nw_regions.hip), and a
region's reads come back as the packed ``(buf, offsets)`` pair :func:`pooled.align_pooled` takes.

* :func:`read_bam`           -- a BAM file or its bytes (BGZF or uncompressed) -> :class:`BamRecords`
* :func:`records_from_sam`   -- SAM text (what ``samtools view [-h]`` prints) -> :class:`BamRecords`
* :func:`extract_regions`    -- the reads of every ``(chr_id, bpstart, bpend)`` -> :class:`RegionReads`
* :func:`demux_by_reference` -- every mapped record to its reference's set -> :class:`RegionReads`
* ``python -m crispresso_amd.regions`` -- one ``.fastq.gz`` per target

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
    """A failed read or extraction."""


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

    def fastq_bytes(self, g: int) -> bytes:
        """``@name\\nseq\\n+\\nqual\\n`` per read, the text the reference writes."""
        (tb, off), (qb, _) = self.reads(g), self.quals(g)
        t, q, o = tb.tobytes(), qb.tobytes(), off.tolist()
        return b"".join(b"@%s\n%s\n+\n%s\n" % (nm, t[o[k]:o[k + 1]], q[o[k]:o[k + 1]])
                        for k, nm in enumerate(self.names(g)))

    def write_fastq_gz(self, g: int, path: str) -> int:
        with gzip.open(path, "wb") as f:
            f.write(self.fastq_bytes(g))
        return int(self.n_reads[g])


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

    def extract(self, bam: BamRecords, table: Optional[np.ndarray], names: List[str], flags: int) -> RegionReads:
        lib = self._lib
        res = _lib.NwrResult()
        n_reg = 0 if table is None else len(table)
        rc = lib.nwr_extract(self._ctx, bam._h, _lib.ptr(table) if n_reg else None, n_reg, flags, ctypes.byref(res))
        if rc != 0:
            msg = lib.nwr_last_error(self._ctx).decode(errors="replace")
            raise RegionsError(f"nwr_extract failed ({rc}): {msg}")
        try:
            R, H, B = int(res.n_regions), int(res.n_hits), int(res.n_bytes)
            region_off = np.zeros(R + 1, np.int64)
            src, st, en = np.empty(H, np.int64), np.empty(H, np.int32), np.empty(H, np.int32)
            toff, text, qual = np.zeros(H + 1, np.int64), np.empty(B, np.uint8), np.empty(B, np.uint8)
            rc = lib.nwr_fetch(ctypes.byref(res), _lib.ptr(region_off), _lib.ptr(src), _lib.ptr(st), _lib.ptr(en),
                               _lib.ptr(toff), _lib.ptr(text), _lib.ptr(qual))
            if rc != 0:
                raise RegionsError(f"nwr_fetch failed ({rc})")
        finally:
            lib.nwr_release(ctypes.byref(res))
        return RegionReads(bam, names, region_off, src, st, en, toff, text, qual, int(res.n_no_seq),
                           float(res.kernel_ms), float(res.upload_ms), bool(flags & _lib.NWR_BY_REFERENCE))


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


def main(argv=None) -> int:
    import argparse
    import os

    p = argparse.ArgumentParser(prog="python -m crispresso_amd.regions",
                                description="The reads of every target region or reference of a BAM, one .fastq.gz each")
    p.add_argument("--bam", required=True, help="BAM file (BGZF or uncompressed)")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--regions", help="region file: chr_id, bpstart, bpend[, name], tab-separated")
    g.add_argument("--by-reference", action="store_true", help="one read set per reference of the BAM")
    p.add_argument("--eqx-as-match", action="store_true", help="treat the CIGAR operations = and X as M")
    p.add_argument("--out", required=True, help="output directory")
    p.add_argument("--device", type=int, default=0)
    args = p.parse_args(argv)
    for f in (args.bam, args.regions):
        if f and not os.path.exists(f):
            p.error(f"cannot open {f}")
    bam = read_bam(args.bam)
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
