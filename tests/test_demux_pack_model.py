"""tests/demux_pack_model.py (nwd_pack's rule in plain Python) held to the host packer on the
gathered text, and the slice arithmetic nwd_adopt_group rests on.  No GPU."""
import numpy as np
import pytest

from crispresso_amd import aligner
from tests import demux_pack_cases as pc
from tests import demux_pack_model as pm


def test_cases_are_what_they_claim():
    """Each construction lands where its docstring says (the model's decisions)."""
    _, reads, want = pc.case("lengths")
    assert want["counts"] == [len(reads), 0, 0, 0, 0, 0] and want["strand"] == [i % 2 for i in range(len(reads))]
    assert {len(r) for r in reads} == {8, 15, 16, 17, 31, 32, 33, 4096}
    order, strands, dst = pm.layout(want, reads)
    three = [w for w in range(dst[-1] // 16) if len({j for j in range(len(order)) if dst[j] < 16 * w + 16 and dst[j + 1] > 16 * w}) >= 3]
    assert three, "no dword holds three reads"
    _, reads, want = pc.case("phases")
    order, strands, dst = pm.layout(want, reads)
    assert want["counts"] == [1, 1, 0, 1, 3, 1] and want["order"] == [1, 3, 5, 2, 4, 6, 0]
    starts = [dst[j] for j in want["group_offsets"][:-1]]
    assert starts == [0, 21, 31, 31, 50, 119]
    assert [s % 4 for s in (21, 50, 31)] == [1, 2, 3] and (21 % 16, 31 % 16) == (5, 15)
    _, reads, want = pc.case("one_group")
    assert want["counts"] == [0, 0, len(reads), 0, 0, 0]
    _, reads, want = pc.case("strand_breaks")
    assert want["counts"] == [0, len(reads), 0, 0, 0, 0] and sum(want["strand"]) >= 10
    order, strands, dst = pm.layout(want, reads)
    _, pos, _ = pm.pack(order, strands, dst, reads)
    # an N at the first and at the last base of a strand-1 read, and on both sides of a dword boundary inside one
    assert {dst[0], dst[2] - 1, dst[5], dst[6] - 1} <= set(pos.tolist())
    assert any(p % 16 == 15 and p + 1 in pos for p in pos.tolist())
    _, reads, want = pc.case("exception_blocks")
    assert want["counts"] == [4, 0, 0, 0, 0, 0]
    order, strands, dst = pm.layout(want, reads)
    _, pos, _ = pm.pack(order, strands, dst, reads)
    assert set(range(pc.BLOCK - 32, pc.BLOCK + 32)) <= set(pos.tolist())
    _, reads, want = pc.case("no_exceptions")
    assert sum(want["counts"]) == len(reads) and not any(set(r) - pm.ACGT for r in reads)
    _, reads, want = pc.case("long_group")
    assert want["counts"] == [0, 3, pc.LEN_GROUP + 1, 0, 0, 0] and want["group_offsets"][2] == 3
    _, reads, want = pc.case("none_assigned")
    assert sum(want["counts"]) == 0


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_model_equals_host_packer(name):
    amps, reads, want = pc.case(name)
    order, strands, dst = pm.layout(want, reads)
    packed, pos, byt = pm.pack(order, strands, dst, reads)
    text, off = pc.gathered(want)
    assert off.tolist() == dst
    host = aligner.pack_2bit(text, off)
    nbytes = (dst[-1] + 3) // 4
    assert len(packed) == nbytes and np.array_equal(packed, host.packed[:nbytes])
    assert np.array_equal(pos, host.exc_pos) and np.array_equal(byt, host.exc_byte)
    assert np.array_equal(host.lens, np.diff(off).astype(np.uint16)) or len(order) == 0
    assert (len(pos) > 0) == (name in ("strand_breaks", "exception_blocks", "long_group"))


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_every_group_decodes_from_its_slice(name):
    """The shared stream at a group's own offsets, with the group's slice of the exceptions, gives
    the group's reads: nothing of a neighbour's shows, whatever lies before the slice's first byte."""
    amps, reads, want = pc.case(name)
    order, strands, dst = pm.layout(want, reads)
    packed, pos, byt = pm.pack(order, strands, dst, reads)
    goff = want["group_offsets"]
    gexc = pm.group_exceptions(pos, dst, goff)
    assert gexc[0] == 0 and gexc[-1] == len(pos) and gexc == sorted(gexc)
    for g, group in enumerate(want["groups"]):
        if not group:
            assert gexc[g] == gexc[g + 1]
            continue
        offsets = dst[goff[g]:goff[g + 1] + 1]
        e0, e1 = gexc[g], gexc[g + 1]
        for fill in (0x00, 0xFF):
            got = pm.decode_slice(packed, pos[e0:e1], byt[e0:e1], offsets, fill)
            assert got == [pm.as_decoded(r) for r in group], (name, g)
