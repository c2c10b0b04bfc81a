"""The FASTQ ingest (crispresso_amd/ingest.py, include/crispr_ingest.h, fastq_parse.hip) restated
on the CPU, twice: `parse_lines` splits the text like the interpreter (flash.read_fastq's own
steps), `parse_positions` does the kernels' position arithmetic (the newline index, the five line
bounds of a record, the '\\r' strip by moving an end, the scans into offsets) and `gather_lanes`
the gather kernel's lane: four output bytes from a binary search on the offsets.

The specification both restate:
  lines    the pieces between '\\n' bytes, an empty final piece is not a line:
           L = count('\\n') + (0 if T == 0 or the last byte is '\\n' else 1)
  records  n = L // 4, record r is lines 4r .. 4r+3, the L % 4 lines after them are ignored
  '\\r'     header, sequence and quality line lose all trailing '\\r' bytes
  fields   name = stripped header without its first byte; seq, qual = the stripped lines
  flags    1 header empty or not '@...'; 2 line 2 empty or not '+...'; 4 len(seq) != len(qual);
           8 a quality byte outside 33..126
"""
from dataclasses import dataclass
from typing import List

import numpy as np

BAD_HEADER, BAD_PLUS, LEN_MISMATCH, BAD_QUAL = 1, 2, 4, 8
INFO_KEYS = ("n", "lines", "trailing_lines", "lmax", "first_bad", "seq_bytes", "qual_bytes", "name_bytes",
             "text_bytes", "bad_header", "bad_plus", "len_mismatch", "bad_qual")


@dataclass
class Parsed:
    text_bytes: int
    lines: int
    names: List[bytes]
    seqs: List[bytes]
    quals: List[bytes]
    flags: np.ndarray   # uint8 [n]

    @property
    def n(self) -> int:
        return len(self.seqs)

    def info(self) -> dict:
        f = self.flags
        bad = np.flatnonzero(f)
        return {
            "n": self.n, "lines": self.lines, "trailing_lines": self.lines % 4,
            "lmax": max((len(s) for s in self.seqs), default=0),
            "first_bad": int(bad[0]) if len(bad) else -1,
            "seq_bytes": sum(map(len, self.seqs)), "qual_bytes": sum(map(len, self.quals)),
            "name_bytes": sum(map(len, self.names)), "text_bytes": self.text_bytes,
            "bad_header": int(np.sum(f & BAD_HEADER != 0)), "bad_plus": int(np.sum(f & BAD_PLUS != 0)),
            "len_mismatch": int(np.sum(f & LEN_MISMATCH != 0)), "bad_qual": int(np.sum(f & BAD_QUAL != 0)),
        }

    def streams(self) -> dict:
        """The three dense streams and their offsets, as nwi_fetch fills them."""
        out = {}
        for key, okey, items in (("seq", "off", self.seqs), ("qual", "qual_off", self.quals),
                                 ("names", "name_off", self.names)):
            off = np.zeros(len(items) + 1, np.int64)
            np.cumsum([len(x) for x in items], out=off[1:])
            out[key], out[okey] = np.frombuffer(b"".join(items), np.uint8), off
        return out


def _qual_bad(q: bytes) -> bool:
    return bool(q) and (min(q) < 33 or max(q) > 126)


def parse_lines(text: bytes) -> Parsed:
    """The interpreter's way: split, pop the empty final piece, strip, slice."""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    n = len(lines) // 4
    names, seqs, quals = [], [], []
    flags = np.zeros(n, np.uint8)
    for r in range(n):
        h, s, p, q = lines[4 * r:4 * r + 4]
        h, s, q = h.rstrip(b"\r"), s.rstrip(b"\r"), q.rstrip(b"\r")
        f = 0
        if not h.startswith(b"@"):
            f |= BAD_HEADER
        if not p.startswith(b"+"):
            f |= BAD_PLUS
        if len(s) != len(q):
            f |= LEN_MISMATCH
        if _qual_bad(q):
            f |= BAD_QUAL
        names.append(h[1:]), seqs.append(s), quals.append(q)
        flags[r] = f
    return Parsed(len(text), len(lines), names, seqs, quals, flags)


@dataclass
class Positions:
    """What the records kernel stores: per stream (seq, qual, name) the starts and lengths."""
    start: np.ndarray   # int64 [3, n]
    length: np.ndarray  # int64 [3, n]
    off: np.ndarray     # int64 [3, n + 1]
    flags012: np.ndarray
    lines: int


def positions(text: bytes) -> Positions:
    """The kernels' arithmetic: the ascending newline positions nl[]; line i is
    [nl[i-1] + 1, nl[i]) with nl[-1] = -1, and the last line of a text with no final newline ends
    at T; trailing '\\r's are stripped by moving the end down."""
    T = len(text)
    t = np.frombuffer(text, np.uint8)
    nl = np.flatnonzero(t == 10).tolist()
    n_nl = len(nl)
    L = n_nl + (0 if T == 0 or text[-1] == 10 else 1)
    n = L // 4
    start, length = np.zeros((3, n), np.int64), np.zeros((3, n), np.int64)
    flags = np.zeros(n, np.uint8)

    def strip(s, e):
        while e > s and text[e - 1] == 13:
            e -= 1
        return e

    for r in range(n):
        i = 4 * r
        s0 = 0 if r == 0 else nl[i - 1] + 1
        e0, e1, e2 = nl[i], nl[i + 1], nl[i + 2]
        e3 = nl[i + 3] if i + 3 < n_nl else T
        s1, s2, s3 = e0 + 1, e1 + 1, e2 + 1
        h, q1, q3 = strip(s0, e0), strip(s1, e1), strip(s3, e3)
        f = 0
        if h == s0 or text[s0] != ord("@"):
            f |= BAD_HEADER
        if e2 == s2 or text[s2] != ord("+"):
            f |= BAD_PLUS
        if q1 - s1 != q3 - s3:
            f |= LEN_MISMATCH
        ns = s0 + 1 if h > s0 else s0
        start[:, r] = (s1, s3, ns)
        length[:, r] = (q1 - s1, q3 - s3, h - ns)
        flags[r] = f
    off = np.zeros((3, n + 1), np.int64)
    np.cumsum(length, axis=1, out=off[:, 1:])
    return Positions(start, length, off, flags, L)


def gather_lanes(text: bytes, start: np.ndarray, off: np.ndarray, check: bool):
    """The gather kernel lane by lane for one stream: lane t holds output bytes 4t .. 4t+3, finds
    the record of byte 4t as the last r with off[r] <= 4t, and steps into the following records
    (past empty ones) as its bytes cross their ends.  -> (the stream, the records with a byte
    outside 33..126 when `check`)."""
    n, total = len(off) - 1, int(off[-1])
    out = bytearray(total)
    bad = np.zeros(n, bool)
    for t in range((total + 3) // 4):
        b0 = 4 * t
        lo, hi = 0, n
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if off[mid] <= b0:
                lo = mid
            else:
                hi = mid
        r = lo
        h0, h1 = int(off[r]), int(off[r + 1])
        for k in range(4):
            b = b0 + k
            if b >= total:
                break
            if b >= h1:
                while True:
                    r += 1
                    h1 = int(off[r + 1])
                    if b < h1:
                        break
                h0 = int(off[r])
            c = text[int(start[r]) + (b - h0)]
            out[b] = c
            if check and (c < 33 or c > 126):
                bad[r] = True
    return bytes(out), bad


def parse_positions(text: bytes, lanes: bool = False) -> Parsed:
    """The kernels' way.  lanes: the streams through `gather_lanes` (small texts), else by slices
    of the same starts and lengths."""
    p = positions(text)
    n = p.start.shape[1]
    flags = p.flags012.copy()
    fields = []
    for q in range(3):
        if lanes:
            dense, bad = gather_lanes(text, p.start[q], p.off[q], check=(q == 1))
            items = [dense[int(p.off[q, r]):int(p.off[q, r + 1])] for r in range(n)]
        else:
            items = [text[int(s):int(s) + int(k)] for s, k in zip(p.start[q], p.length[q])]
            bad = np.array([_qual_bad(x) for x in items], bool) if q == 1 else None
        if q == 1:
            flags[bad] |= BAD_QUAL
        fields.append(items)
    return Parsed(len(text), p.lines, fields[2], fields[0], fields[1], flags)
