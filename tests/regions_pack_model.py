"""The packed batch of an ``NWR_PACKED`` call (include/crispr_regions.h) in plain Python, from the
BAM's 4-bit codes: base ``i`` of the reads laid end to end, in result order, is in bits
``2 (i % 4)`` of byte ``i // 4`` with codes 1 2 8 4 (A C T G) as 0 1 2 3; every other code is an
exception (position, upper-case letter) and gives 0 bits.  tests/test_regions_pack_model.py holds
it to the library's host packer on the same reads; tests/test_gpu_regions_resident.py holds the
kernels to that packer.
"""
import numpy as np

NIBBLES = "=ACMGRSVTWYHKDBN"
BASE_OF = {1: 0, 2: 1, 8: 2, 4: 3}


def flat_reads(want):
    """The reads of a tests/regions_model.py result in result order: region-major, record order."""
    return [h[3] for hits in want["hits"] for h in hits]


def offsets_of(reads):
    return np.cumsum([0] + [len(r) for r in reads]).astype(np.int64)


def pack(reads):
    """(packed uint8 [(total + 3) // 4], exc_pos int64, exc_byte uint8, lens int64) of the reads; a
    length above 65535 is one the packed call refuses."""
    codes = [NIBBLES.index(chr(c)) for r in reads for c in r]
    packed = np.zeros((len(codes) + 3) // 4, np.uint8)
    pos, byt = [], []
    for i, n in enumerate(codes):
        if n in BASE_OF:
            packed[i // 4] |= BASE_OF[n] << (2 * (i % 4))
        else:
            pos.append(i)
            byt.append(ord(NIBBLES[n]))
    return packed, np.array(pos, np.int64), np.array(byt, np.uint8), np.array([len(r) for r in reads], np.int64)


def region_exc(want, exc_pos):
    """[regions + 1]: region g's exceptions are the slots region_exc[g] .. region_exc[g + 1]."""
    starts = np.cumsum([0] + [sum(len(h[3]) for h in hits) for hits in want["hits"]])
    return np.searchsorted(exc_pos, starts, side="left").astype(np.int64)
