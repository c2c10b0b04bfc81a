"""tests/regions_pack_model.py against the library's host packer (nw_pack_reads, through
``aligner.pack_2bit``) on the text tests/regions_model.py extracts: the bytes an ``NWR_PACKED``
call must leave in HBM, pinned without a GPU."""
import numpy as np
import pytest

from crispresso_amd.aligner import pack_2bit
from tests import regions_cases as rc
from tests import regions_model as rm
from tests import regions_pack_model as rpm


def cases():
    out = {}
    for name, make in (("cigar_edges", rc.cigar_edges), ("slice_edges", rc.slice_edges),
                       ("random", lambda: rc.random_case(500, 40))):
        refs, records, regs = make()
        out[name] = rm.extract(records, regs)
    return out


@pytest.mark.parametrize("name", ["cigar_edges", "slice_edges", "random"])
def test_model_equals_the_host_packer(name):
    want = cases()[name]
    reads = rpm.flat_reads(want)
    off = rpm.offsets_of(reads)
    text = np.frombuffer(b"".join(reads), np.uint8)
    packed, pos, byt, lens = rpm.pack(reads)
    if name == "slice_edges":            # hits of 69,999 and 69,997 bases: the packed call refuses these two regions
        assert sorted(lens[lens > 65535].tolist()) == [69997, 69999]
    host = pack_2bit(np.ascontiguousarray(text), off, nthreads=2)
    nbytes = (int(off[-1]) + 3) // 4
    assert np.array_equal(host.packed[:nbytes], packed) and len(packed) == nbytes
    assert np.array_equal(host.exc_pos, pos) and np.array_equal(host.exc_byte, byt)
    assert lens.tolist() == np.diff(off).tolist()
    assert int(off[-1]) > 100
    if name == "slice_edges":
        assert len(pos) > 0 and set(byt.tolist()) <= set(b"=MRSVWYHKDBN")
    bounds = rpm.region_exc(want, pos)
    assert bounds[0] == 0 and bounds[-1] == len(pos) and (np.diff(bounds) >= 0).all()


def test_every_code():
    reads = [rpm.NIBBLES.encode(), b"", b"N", rpm.NIBBLES[::-1].encode() * 3]
    packed, pos, byt, lens = rpm.pack(reads)
    text = np.frombuffer(b"".join(reads), np.uint8)
    host = pack_2bit(np.ascontiguousarray(text), rpm.offsets_of(reads), nthreads=1)
    assert np.array_equal(host.packed[:len(packed)], packed)
    assert np.array_equal(host.exc_pos, pos) and np.array_equal(host.exc_byte, byt)
    assert len(pos) == 12 + 1 + 36 and lens.tolist() == [16, 0, 1, 48]
    # A C T G of the first read sit at positions 1, 2, 8, 4
    first = int(packed[0]) | int(packed[1]) << 8 | int(packed[2]) << 16 | int(packed[3]) << 24
    assert [(first >> (2 * p)) & 3 for p in (1, 2, 8, 4)] == [0, 1, 2, 3]
