"""Inputs of the FASTQ ingest's tests (tests/test_ingest_model.py on the CPU,
tests/test_gpu_ingest.py on the GPU): texts, what each is there for, and hand-written flags.

The count, line and gather kernels work on 16-byte chunks, 256 lanes a block (4 KiB of text a
block of the line index, 256 records a block of the record kernels); one scan block takes 1024
blocks a step."""
import functools
import gzip
from typing import Dict, List, Tuple

import numpy as np

BLOCK = 4096


def record(k: int, seq_len: int = 10, name: bytes = None, eol: bytes = b"\n") -> bytes:
    name = b"r%d" % k if name is None else name
    seq = (b"ACGTTGCA" * (seq_len // 8 + 1))[:seq_len]
    qual = bytes(33 + (k + j) % 94 for j in range(seq_len))
    return b"@" + name + eol + seq + eol + b"+" + eol + qual + eol


def records(n: int, eol: bytes = b"\n", lens=(10, 3, 0, 17, 1, 150)) -> bytes:
    return b"".join(record(k, lens[k % len(lens)], eol=eol) for k in range(n))


def text_of_size(size: int) -> bytes:
    """Records cut at exactly `size` bytes (a partial last record, usually no final newline)."""
    return records(size // 8 + 2)[:size]


def newline_at_block_edge() -> bytes:
    """A '\\n' as byte 4095 and another as byte 4096: the header of a record ends one block, its
    empty sequence line is the first byte of the next; the record straddles the two blocks."""
    head = records(40)
    assert len(head) < BLOCK - 40
    pad = BLOCK - 1 - len(head) - 1
    t = head + b"@" + b"n" * pad + b"\n" + b"\n" + b"+\n" + b"\n" + records(5)
    assert t[BLOCK - 1] == 10 and t[BLOCK] == 10
    return t


def header_lengths() -> bytes:
    """Headers of 1..8 bytes (names of 0..7) before sequences of 0..9 bases: every source
    alignment of the three gathers, fields that start and end inside one output dword."""
    out = []
    for k in range(40):
        out.append(record(k, k % 10, name=b"hdrname"[:k % 8]))
    return b"".join(out)


def long_record() -> bytes:
    return records(9) + record(9, 70000) + records(7)


@functools.lru_cache(maxsize=None)
def many_short_records() -> bytes:
    """About 7 MB of short records: more 4 KiB blocks (and more 256-record blocks) than the 1024
    threads of a scan block, so each takes several."""
    rng = np.random.Generator(np.random.PCG64(411))
    lens = rng.integers(0, 7, size=420000).tolist()
    t = b"".join(b"@%d\n%s\n+\n%s\n" % (k, b"ACGTAC"[:l], b"IHGFED"[:l]) for k, l in enumerate(lens))
    assert len(t) > 1024 * BLOCK and len(lens) > 1024 * 256
    return t


FLAG_TEXT = (b"@a\nAC\n+\nII\n"          # 0: clean
             b"a\nAC\n+\nII\n"           # 1: no '@'
             b"@b\nAC\n-\nII\n"          # 2: no '+'
             b"@c\nACG\n+\nII\n"         # 3: lengths differ
             b"@d\nAC\n+\nI \n"          # 4: a quality byte 32
             b"\nAC\n\nI\x7f!\n"         # 5: all four
             b"@e\nAC\n+e\nI~\n"         # 6: clean ('+' with the name repeated, quality 126)
             b"\r\n\n+\n\n"              # 7: a header of '\r' only: empty after the strip
             b"@f\n\n\r\n\n"             # 8: line 2 is '\r': not '+'
             b"@g\nAC\n+\n!~\n")         # 9: clean (qualities 33 and 126)
FLAG_EXPECTED = [0, 1, 2, 4, 8, 15, 0, 1, 2, 0]

# (text, flags) written by hand
HAND_FLAGS: List[Tuple[bytes, List[int]]] = [
    (FLAG_TEXT, FLAG_EXPECTED),
    (b"@a\nAC\n+\nII", [0]),
    (b"@a\r\nAC\r\n+\r\nII\r\n", [0]),
    (b"@a\nAC\r\r\n+\nII\n", [0]),                 # every trailing '\r' goes
    (b"@a\nA\rC\n+\nII\n", [4]),                   # a '\r' inside stays: three bases
    (b"@a\nA\rC\n+\nI\rI\n", [8]),                 # and is no quality
    (b"@a\nAC\n+\n\x1fI\n@b\nAC\n+\n\x80I\n", [8, 8]),
    (b"x\n\n\n\n", [3]),
    (b"\n\n\n\n", [3]),
    (b"@\n\n+\n\n", [0]),                          # empty name, empty read
]


@functools.lru_cache(maxsize=None)
def cases() -> Dict[str, bytes]:
    c: Dict[str, bytes] = {}
    for size in (0, 1, 15, 16, 17, 4095, 4096, 4097):
        c[f"size_{size}"] = text_of_size(size)
    c["newline_at_block_edge"] = newline_at_block_edge()
    c["straddle"] = records(200)                   # 200 records over three blocks
    base = records(5)
    for extra in range(4):
        c[f"lines_mod4_{extra}"] = base + b"".join([b"@tail\n", b"ACGT\n", b"+\n"][:extra])
    c["no_final_newline"] = records(6)[:-1]
    c["no_final_newline_cr"] = records(6, eol=b"\r\n")[:-1]
    c["only_newlines"] = b"\n" * 37
    c["one_newline"] = b"\n"
    c["no_newline"] = b"@abc"
    c["empty_lines"] = b"@a\n\n+\n\n@b\n\n+\n\n@c\nA\n+\nI\n"
    for n in (255, 256, 257):
        c[f"records_{n}"] = records(n, lens=(4, 0, 9))
    c["crlf"] = records(300, eol=b"\r\n")
    c["cr_only_lines"] = b"\r\n\r\n\r\n\r\n@a\r\r\n\r\r\r\n+\r\n\r\n" * 3
    c["cr_inside"] = b"@a\rb\nAC\rGT\n+\nII\rII\n@c\r\nA\r\rC\r\n+x\r\nI\r\rI\r\n"
    c["header_lengths"] = header_lengths()
    c["long_record"] = long_record()
    c["high_bytes"] = b"@\xc3\xa9\xff\x80name\nAC\n+\nII\n@\x80\nA\n+\nI\n"
    c["quality_edges"] = b"@a\nACGT\n+\n !~\x7f\n@b\nAC\n+\n!~\n@c\nAC\n+\n~\x7f\n@d\nA\n+\n \n"
    c["flags"] = FLAG_TEXT
    c["flags_late"] = records(700) + b"@x\nACG\n+\nII\n" + records(300) + b"y\nAC\n+\nII\n" + records(3)
    c["many_short_records"] = many_short_records()
    return c


SMALL = 1 << 14   # cases up to this size also go through the lane-by-lane gather model


def random_texts(count: int, max_len: int, seed: int = 20000) -> List[bytes]:
    """Random texts over '\\n \\r @ + A I', '\\n' weighted."""
    rng = np.random.Generator(np.random.PCG64(seed))
    alphabet = np.frombuffer(b"\n\r@+AI", np.uint8)
    p = np.array([0.4, 0.12, 0.12, 0.12, 0.12, 0.12])
    out = []
    for _ in range(count):
        out.append(alphabet[rng.choice(6, size=int(rng.integers(0, max_len + 1)), p=p)].tobytes())
    return out


def gz_members(*parts: bytes) -> bytes:
    return b"".join(gzip.compress(p, mtime=0) for p in parts)
