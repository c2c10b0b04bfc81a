"""FASTQ ingest with qualities on the GPU: a FASTQ(.gz) file to dense bases, qualities and names.

CRISPResso hands its raw files to Trimmomatic (``CRISPResso/CRISPRessoCORE.py:1585-1640``) and
FLASH (``CORE:1655-1677``); :func:`crispresso_amd.flash.read_fastq` reads them here with an
interpreter pass.  This module is that reader on the device (C ABI ``nwi_*``,
``include/crispr_ingest.h``, kernels ``crispresso_amd/csrc/fastq_parse.hip``): the inflated text
is uploaded once, the records are found there, and the bases and qualities stay in HBM where
:func:`crispresso_amd.frontend.prepare_fastq_device` hands them to the front end's kernels.  The
records are exactly ``read_fastq``'s (the header restates the semantics); each also has a flag
byte that reader never computes.  There is no CPU fallback: without the library or a GPU every
call raises :class:`crispresso_amd._lib.NativeLibraryError`.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional, Tuple, Union

import numpy as np

from . import _lib

BAD_HEADER, BAD_PLUS, LEN_MISMATCH, BAD_QUAL = (
    _lib.NWI_BAD_HEADER, _lib.NWI_BAD_PLUS, _lib.NWI_LEN_MISMATCH, _lib.NWI_BAD_QUAL)
FLAG_REASONS = (
    (BAD_HEADER, "the header line is empty or does not start with '@'"),
    (BAD_PLUS, "the third line is empty or does not start with '+'"),
    (LEN_MISMATCH, "the sequence and its quality line differ in length"),
    (BAD_QUAL, "a quality byte outside 33..126 (phred 33)"),
)
_INFO_FIELDS = ("n", "lines", "trailing_lines", "lmax", "first_bad", "seq_bytes", "qual_bytes", "name_bytes",
                "text_bytes", "upload_ms", "kernel_ms", "inflate_ms")


class IngestError(_lib.NativeLibraryError):
    """A failed nwi_* call (the message is the library's); ``code`` is its return."""

    def __init__(self, msg: str, code: int):
        super().__init__(f"{msg} (code {code})")
        self.code = code


class FastqFormatError(ValueError):
    """A flagged record under ``strict=True``: ``record`` is its index, ``flags`` its flag byte."""

    def __init__(self, record: int, flags: int):
        reason = next((text for bit, text in FLAG_REASONS if flags & bit), "flagged")
        super().__init__(f"FASTQ record {record}: {reason}")
        self.record, self.flags = record, flags


class FastqRecords:
    """One parsed text.  ``info`` always; the arrays only after a fetch (``fetch=True`` or
    :meth:`fetch`): ``seq`` / ``qual`` / ``names`` are dense uint8 streams, ``off`` / ``name_off``
    their int64 offsets (n + 1, from 0); ``qual_off`` is None unless it differs from ``off`` (a
    record whose lines differ in length).  The streams stay on the device until :meth:`close`."""

    def __init__(self, lib, handle: int):
        self._lib, self._h = lib, handle
        s = _lib.NwiSummary()
        lib.nwi_info(handle, ctypes.byref(s))
        self.info: Dict[str, Union[int, float]] = {k: getattr(s, k) for k in _INFO_FIELDS}
        for k, name in enumerate(("bad_header", "bad_plus", "len_mismatch", "bad_qual")):
            self.info[name] = int(s.flagged[k])
        self.names = self.name_off = self.seq = self.qual = self.off = self.qual_off = self.flags = None

    def __len__(self) -> int:
        return int(self.info["n"])

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise IngestError(self._lib.nwi_last_error().decode(errors="replace"), rc)

    def fetch(self) -> "FastqRecords":
        """Copies every array to the host."""
        if self._h is None:
            raise IngestError("FastqRecords: closed", -1)
        n, i = len(self), self.info
        self.flags = np.zeros(n, np.uint8)
        self.seq, self.qual = np.zeros(i["seq_bytes"], np.uint8), np.zeros(i["qual_bytes"], np.uint8)
        self.names = np.zeros(i["name_bytes"], np.uint8)
        self.off, qual_off, self.name_off = (np.zeros(n + 1, np.int64) for _ in range(3))
        p = _lib.ptr
        self._check(self._lib.nwi_fetch(self._h, p(self.flags), p(self.seq), p(self.off), p(self.qual), p(qual_off),
                                        p(self.names), p(self.name_off)))
        self.qual_off = None if np.array_equal(qual_off, self.off) else qual_off
        return self

    def fetch_names(self) -> Tuple[np.ndarray, np.ndarray]:
        """Only the name stream and its offsets."""
        if self._h is None:
            raise IngestError("FastqRecords: closed", -1)
        names, name_off = np.zeros(self.info["name_bytes"], np.uint8), np.zeros(len(self) + 1, np.int64)
        self._check(self._lib.nwi_fetch(self._h, None, None, None, None, None, _lib.ptr(names), _lib.ptr(name_off)))
        return names, name_off

    def fetch_offsets(self) -> np.ndarray:
        """Only the sequences' offsets."""
        if self._h is None:
            raise IngestError("FastqRecords: closed", -1)
        off = np.zeros(len(self) + 1, np.int64)
        self._check(self._lib.nwi_fetch(self._h, None, None, _lib.ptr(off), None, None, None, None))
        return off

    def fetch_flags(self) -> np.ndarray:
        flags = np.zeros(len(self), np.uint8)
        if self._h is None:
            raise IngestError("FastqRecords: closed", -1)
        self._check(self._lib.nwi_fetch(self._h, _lib.ptr(flags), None, None, None, None, None, None))
        return flags

    def lists(self) -> Tuple[List[bytes], List[bytes], List[bytes]]:
        """(names, seqs, quals) as ``flash.read_fastq`` returns them (after a fetch)."""
        qo = self.off if self.qual_off is None else self.qual_off
        out = []
        for buf, off in ((self.names, self.name_off), (self.seq, self.off), (self.qual, qo)):
            raw, o = buf.tobytes(), off.tolist()
            out.append([raw[o[k]:o[k + 1]] for k in range(len(self))])
        return out[0], out[1], out[2]

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            self._lib.nwi_release(self._h)
            self._h = None

    def __enter__(self) -> "FastqRecords":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):  # pragma: no cover - runs at garbage collection
        try:
            self.close()
        except Exception:
            pass


def _finish(lib, rc: int, handle: ctypes.c_void_p, strict: bool, fetch: bool) -> FastqRecords:
    if rc != 0:
        raise IngestError(lib.nwi_last_error().decode(errors="replace"), rc)
    rec = FastqRecords(lib, handle.value)
    try:
        bad = int(rec.info["first_bad"])
        if strict and bad >= 0:
            raise FastqFormatError(bad, int(rec.fetch_flags()[bad]))
        if fetch:
            rec.fetch()
    except Exception:
        rec.close()
        raise
    return rec


def parse_fastq_bytes(data: Union[bytes, bytearray, memoryview, np.ndarray], device: int = 0, strict: bool = True,
                      fetch: bool = True) -> FastqRecords:
    """Parses FASTQ text (not gzip) held in host memory on ``device``.  ``strict`` raises
    :class:`FastqFormatError` for the first flagged record; ``strict=False`` returns the flags.
    ``fetch=False`` leaves every array on the device (for the front end's hand-off)."""
    lib = _lib.load()
    a = data if isinstance(data, np.ndarray) else np.frombuffer(data, np.uint8)
    a = np.ascontiguousarray(a, np.uint8)
    h = ctypes.c_void_p()
    rc = lib.nwi_parse_text(int(device), _lib.ptr(a) if a.size else None, int(a.size), ctypes.byref(h))
    return _finish(lib, rc, h, strict, fetch)


def read_fastq_records(path: str, device: int = 0, strict: bool = True, fetch: bool = True) -> FastqRecords:
    """:func:`parse_fastq_bytes` on a FASTQ(.gz) file: mapped, inflated when its first two bytes
    say gzip (every member; a damaged or truncated member is an error), parsed on ``device``."""
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.nwi_parse_file(int(device), os.fsencode(path), ctypes.byref(h))
    return _finish(lib, rc, h, strict, fetch)


def read_fastq(path: str, device: int = 0) -> Tuple[List[bytes], List[bytes], List[bytes]]:
    """Drop-in for :func:`crispresso_amd.flash.read_fastq`: (header lines without their first
    byte, sequences, qualities).  Like that reader it checks nothing."""
    with read_fastq_records(path, device, strict=False, fetch=True) as rec:
        return rec.lists()
