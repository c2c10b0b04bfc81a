"""The grouped-read packer of include/crispr_demux.h (nwd_pack) in plain Python: dword ``w`` of
the 2-bit stream and the ordered exceptions, straight from the input reads, without the gathered
text.  tests/test_demux_pack_model.py holds it to the host packer (``aligner.pack_2bit``) on the
gathered text; tests/test_gpu_demux_resident.py holds the kernels to it.

Gathered position ``dst[j] + p`` is base p of gathered read j: ``reads[order[j]]`` as given, or
reversed and complemented when ``strands[j]`` is 1.  A base's code is ``(byte >> 1) & 3`` (A C T
G = 0 1 2 3), so the complement's code is ``code ^ 2``; a byte that is none of A C G T a c g t is
an exception (complementing leaves it as it is) and gives 0 bits, as does a position past the end.
"""
import bisect

import numpy as np

ACGT = frozenset(b"ACGTacgt")


def base_at(p, order, strands, dst, reads):
    """(byte, reversed) that gathered position p shows before complementing."""
    j = bisect.bisect_right(dst, p) - 1             # the last j with dst[j] <= p
    q, n = p - dst[j], dst[j + 1] - dst[j]
    read = reads[order[j]]
    assert len(read) == n
    return (read[n - 1 - q], 1) if strands[j] else (read[q], 0)


def dword(w, order, strands, dst, reads):
    """(the 32 bits, [(position, byte), ...]) of gathered positions 16 w .. 16 w + 15."""
    out, exc = 0, []
    for k in range(16):
        p = 16 * w + k
        if p >= dst[-1]:
            break
        c, rev = base_at(p, order, strands, dst, reads)
        if c in ACGT:
            out |= (((c >> 1) & 3) ^ (2 * rev)) << (2 * k)
        else:
            exc.append((p, c))
    return out, exc


def pack(order, strands, dst, reads):
    """(packed uint8 [(dst[-1] + 3) // 4], exc_pos int64, exc_byte uint8) of the whole call."""
    dst = [int(x) for x in dst]
    nwords = (dst[-1] + 15) // 16
    words, exc = np.zeros(nwords, "<u4"), []
    for w in range(nwords):
        words[w], e = dword(w, order, strands, dst, reads)
        exc += e
    packed = words.view(np.uint8)[:(dst[-1] + 3) // 4].copy()
    return packed, np.array([p for p, _ in exc], np.int64), np.array([c for _, c in exc], np.uint8)


def layout(want, reads):
    """(order, strands per gathered read, dst) of a tests/demux_model.py result."""
    order = list(want["order"])
    strands = [want["strand"][r] for r in order]
    dst = [0]
    for r in order:
        dst.append(dst[-1] + len(reads[r]))
    return order, strands, dst


def group_exceptions(exc_pos, dst, group_offsets):
    """group_exc [groups + 1]: group g's exceptions are the slots group_exc[g] .. group_exc[g + 1]."""
    pos = [int(p) for p in exc_pos]
    return [bisect.bisect_left(pos, dst[j]) for j in group_offsets]


def decode_slice(packed, exc_pos, exc_byte, offsets, fill=0xA5):
    """The reads of a slice of the shared stream, decoded as the aligner's adoption sees them
    (nw_front::set_packed_batch): it copies bytes q0 = offsets[0] // 4 .. pk_hi = (offsets[n] + 3)
    // 4 of the stream to byte q0 - P0 of its own buffer, P0 = (offsets[0] // 16) * 4, and reads
    position p at byte p // 4 - P0; what lies before q0 is not the stream's (``fill``).  The
    exceptions are the slice's own, in the stream's coordinates."""
    offsets = [int(x) for x in offsets]
    base0, end = offsets[0], offsets[-1]
    q0, pk_hi, p0 = base0 // 4, (end + 3) // 4, (base0 // 16) * 4
    mine = np.full(pk_hi - p0, fill, np.uint8)
    mine[q0 - p0:] = packed[q0:pk_hi]
    text = bytearray(end - base0)
    for p in range(base0, end):
        text[p - base0] = b"ACTG"[(int(mine[p // 4 - p0]) >> (2 * (p % 4))) & 3]
    for p, c in zip(exc_pos, exc_byte):
        assert base0 <= int(p) < end, "an exception outside its slice"
        text[int(p) - base0] = int(c)
    return [bytes(text[a - base0:b - base0]) for a, b in zip(offsets[:-1], offsets[1:])]


def as_decoded(read):
    """What decoding a packed read gives: its bases in upper case, its exceptions as they are."""
    return bytes((c & 0xDF) if c in ACGT else c for c in read)
