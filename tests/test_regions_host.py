"""The BAM reader (crispresso_amd/csrc/nw_bam.cpp through crispresso_amd/regions.py) without a
GPU: the round trip of the writer's BAMs (tests/regions_cases.py), BGZF block boundaries inside
records, stored blocks, no EOF block, many references, SAM text, and every malformed input."""
import struct
import zlib

import numpy as np
import pytest

from crispresso_amd import _lib, regions
from tests import regions_cases as rc


def records_of(bam):
    d, o = bam.data.tobytes(), bam.offsets.tolist()
    return [d[o[i]:o[i + 1]] for i in range(len(bam))]


@pytest.fixture(scope="module")
def case():
    refs, records, _ = rc.random_case(400, 1, seed=3)
    records.append(rc.rec("long", 1, 1, "70000M"))          # a record larger than a BGZF block
    records.append(rc.rec("tail", 2, 7, "10M"))
    return refs, records, rc.bam_plain(refs, records, b"@HD\tVN:1.6\n")


def check(bam, refs, records, text=b"@HD\tVN:1.6\n"):
    assert len(bam) == len(records)
    assert bam.ref_names == [n for n, _ in refs] and bam.ref_lens.tolist() == [l for _, l in refs]
    assert bam.text == text
    assert records_of(bam) == [rc.record_bytes(r) for r in records]
    assert [bam.name(i) for i in range(len(bam))] == [r["name"] for r in records]
    assert bam.offsets.dtype == np.int64 and int(bam.offsets[-1]) == len(bam.data)


def test_round_trip_plain_and_bgzf(case, tmp_path):
    refs, records, plain = case
    check(regions.read_bam(plain), refs, records)
    z = rc.bgzf(plain)
    assert z.count(b"\x1f\x8b\x08\x04") >= 3
    check(regions.read_bam(z), refs, records)
    p = tmp_path / "a.bam"
    p.write_bytes(z)
    check(regions.read_bam(str(p)), refs, records)
    p.write_bytes(plain)
    check(regions.read_bam(str(p)), refs, records)
    check(regions.read_bam(np.frombuffer(z, np.uint8)), refs, records)


def test_records_straddle_block_boundaries(case):
    refs, records, plain = case
    bam = regions.read_bam(plain)
    o = bam.offsets.tolist()
    # inside the block_size field, the core fields, the name, the CIGAR, the sequence and the qualities
    cuts = [o[5] + 1, o[6] + 3, o[7] + 20, o[8] + 37, o[9] + 45, o[10] + 60, o[11] - 1, o[12], 5, 13]
    check(regions.read_bam(rc.bgzf(plain, cuts)), refs, records)
    check(regions.read_bam(rc.bgzf(plain, range(1, len(plain), 997))), refs, records)      # many small blocks
    check(regions.read_bam(rc.bgzf(plain, [o[-3] + 100], block=4096)), refs, records)


def test_stored_blocks_and_missing_eof(case):
    refs, records, plain = case
    z = rc.bgzf(plain, stored=True)
    assert len(z) > len(plain)
    check(regions.read_bam(z), refs, records)
    assert rc.bgzf(plain, eof=False) + rc.EOF_BLOCK == rc.bgzf(plain)
    check(regions.read_bam(rc.bgzf(plain, eof=False)), refs, records)
    check(regions.read_bam(rc.bgzf(plain, [100, 100000], stored=True, eof=False)), refs, records)


def test_many_references_and_no_records():
    refs = [("contig_%d_%s" % (k, "x" * (k % 40)), 1000 + k) for k in range(300)]
    records = [rc.rec("r%d" % k, (k * 7) % 300, 1 + k, "10M") for k in range(50)]
    check(regions.read_bam(rc.bgzf(rc.bam_plain(refs, records), [30, 2000])), refs, records, b"")
    check(regions.read_bam(rc.bgzf(rc.bam_plain(refs, []))), refs, [], b"")
    check(regions.read_bam(rc.bam_plain([], [])), [], [], b"")


def test_records_from_sam_gives_the_writers_layout():
    refs, records, _ = rc.cigar_edges()
    records += rc.record_filter()[1] + rc.slice_edges()[1][:3]
    lines = [rc.sam_line(r, refs) for r in records]
    assert any(l.endswith("\t*\t*") for l in lines) and any(l.endswith("T\t*") for l in lines)
    for given in (lines, "\n".join(lines) + "\n", [l.encode() + b"\n" for l in lines]):
        check(regions.records_from_sam(given, references=refs), refs, records, b"")
    header = ["@HD\tVN:1.6", "@SQ\tSN:chr1\tLN:100000", "@SQ\tSN:chr2\tLN:100000"]
    check(regions.records_from_sam(header + lines), refs, records, ("\n".join(header) + "\n").encode())
    # without a header the references come from the RNAME column, in order of first appearance
    bam = regions.records_from_sam(lines)
    assert bam.ref_names == ["chr1", "chr2"] and records_of(bam) == [rc.record_bytes(r) for r in records]
    with pytest.raises(ValueError):
        regions.records_from_sam(["r\t0\tchr9\t1\t30\t4M\t*\t0\t0\tACGT\tIIII"], references=refs)
    with pytest.raises(ValueError):
        regions.records_from_sam(["r\t0\tchr1\t1\t30\t4Q\t*\t0\t0\tACGT\tIIII"], references=refs)


def patched(plain, at, fmt, value):
    b = bytearray(plain)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def test_malformed_input_returns_its_error(case, tmp_path):
    refs, records, plain = case
    z = rc.bgzf(plain)
    o = regions.read_bam(plain).offsets.tolist()
    first_block = struct.unpack_from("<H", z, 16)[0] + 1
    bad_crc = bytearray(z)
    bad_crc[first_block - 8] ^= 1
    bad_size = bytearray(z)
    bad_size[first_block - 4] ^= 1
    bad_deflate = bytearray(z)
    bad_deflate[40] ^= 0xFF
    no_bc = bytearray(z)
    no_bc[12:14] = b"XY"
    plain_gzip = zlib.compressobj(6, zlib.DEFLATED, 31)
    plain_gzip = plain_gzip.compress(plain) + plain_gzip.flush()
    r5 = o[5]
    cases = {
        "bad BAM magic": b"BAM\2" + plain[4:],
        "bad BAM magic ": b"",
        "bad BAM magic  ": b"SAM text",
        "bad BAM magic   ": rc.bgzf(b"BAX\1" + plain[4:]),
        "truncated": z[:first_block + 10],
        "truncated ": z[:first_block - 1],
        "truncated  ": z[:7],
        "CRC-32 mismatch": bytes(bad_crc),
        "block's size": bytes(bad_size),
        "BGZF block 0": bytes(bad_deflate),
        "no BC field": bytes(no_bc),
        "not a BGZF block": plain_gzip,
        "passes the end": plain[:-1],
        "passes the end ": rc.bgzf(plain[:-40]),
        "record 5 passes the end": patched(plain, r5, "<i", len(plain)),
        "block_size": patched(plain, r5, "<i", 31),
        "block_size ": patched(plain, r5, "<i", -5),
        "smaller than its fields": patched(plain, r5 + 20, "<i", 100000),       # l_seq
        "smaller than its fields ": patched(plain, r5 + 16, "<H", 60000),      # n_cigar_op
        "l_seq": patched(plain, r5 + 20, "<i", -1),
        "reference": patched(plain, r5 + 4, "<i", len(refs)),
        "reference ": patched(plain, r5 + 4, "<i", -2),
        "truncated (2 bytes left)": plain + b"\0\0",
        "header text": patched(plain, 4, "<i", len(plain)),
        "references": patched(plain, 8 + 11, "<i", -1),
        "name of ": patched(plain, 8 + 11, "<i", 1 << 20),      # (the records read as references)
        "reference 0: name of": patched(plain, 8 + 11 + 4, "<i", 0),
    }
    for want, data in cases.items():
        with pytest.raises(regions.RegionsError) as e:
            regions.read_bam(data)
        assert want.strip() in str(e.value), (want, str(e.value))
        assert "(%d)" % _lib.NW_E_INVALID in str(e.value)
    with pytest.raises(regions.RegionsError, match="cannot open"):
        regions.read_bam(str(tmp_path / "missing.bam"))
    # a damaged record late in the stream, through BGZF: the same error
    with pytest.raises(regions.RegionsError, match="record %d" % (len(records) - 1)):
        regions.read_bam(rc.bgzf(patched(plain, o[-2], "<i", 1 << 20)))
