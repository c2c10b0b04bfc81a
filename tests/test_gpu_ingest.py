"""The FASTQ ingest on the GPU (crispresso_amd/ingest.py, nwi_*, fastq_parse.hip) against its CPU
restatement (tests/ingest_model.py): every field of every record -- flags, the three offset
arrays, the three streams, info -- on the cases of tests/ingest_cases.py; strict mode; gzip files;
repeatability."""
import functools
import gzip

import numpy as np
import pytest

from crispresso_amd import flash, ingest
from tests import ingest_cases as ic
from tests import ingest_model as im

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def model(name: str) -> im.Parsed:
    return im.parse_lines(ic.cases()[name])


def assert_equals_model(rec: ingest.FastqRecords, p: im.Parsed, what=""):
    assert {k: rec.info[k] for k in im.INFO_KEYS} == p.info(), what
    s = p.streams()
    assert rec.flags.dtype == np.uint8 and rec.off.dtype == np.int64 and rec.name_off.dtype == np.int64
    assert np.array_equal(rec.flags, p.flags), (what, np.flatnonzero(rec.flags != p.flags)[:10])
    assert np.array_equal(rec.off, s["off"]), what
    assert np.array_equal(rec.off if rec.qual_off is None else rec.qual_off, s["qual_off"]), what
    assert (rec.qual_off is None) == np.array_equal(s["off"], s["qual_off"]), what
    assert np.array_equal(rec.name_off, s["name_off"]), what
    for key in ("seq", "qual", "names"):
        got = getattr(rec, key)
        assert got.shape == s[key].shape and np.array_equal(got, s[key]), (what, key, np.flatnonzero(got != s[key])[:10])


@pytest.mark.parametrize("name", sorted(ic.cases()))
def test_cases_against_model(name):
    with ingest.parse_fastq_bytes(ic.cases()[name], strict=False) as rec:
        assert_equals_model(rec, model(name), name)
        p = model(name)
        assert rec.lists() == (p.names, p.seqs, p.quals)


def test_random_texts_against_model():
    for k, text in enumerate(ic.random_texts(150, 14) + ic.random_texts(150, 120, seed=7)):
        with ingest.parse_fastq_bytes(text, strict=False) as rec:
            assert_equals_model(rec, im.parse_lines(text), (k, text))


@pytest.mark.parametrize("k", range(len(ic.HAND_FLAGS)))
def test_flags_by_hand_and_strict(k):
    text, flags = ic.HAND_FLAGS[k]
    with ingest.parse_fastq_bytes(text, strict=False) as rec:
        assert rec.flags.tolist() == flags
    bad = [r for r, f in enumerate(flags) if f]
    if not bad:
        ingest.parse_fastq_bytes(text, strict=True).close()
        return
    with pytest.raises(ingest.FastqFormatError) as ei:
        ingest.parse_fastq_bytes(text, strict=True)
    assert ei.value.record == bad[0] and ei.value.flags == flags[bad[0]]
    assert f"record {bad[0]}" in str(ei.value)


@pytest.mark.parametrize("bit", [1, 2, 4, 8])
def test_strict_names_each_flag(bit):
    r = ic.FLAG_EXPECTED.index(bit)
    lines = ic.FLAG_TEXT.split(b"\n")
    text = b"".join(b"\n".join(lines[4 * k:4 * k + 4]) + b"\n" for k in (0, r, 6))   # clean, flagged, clean
    with pytest.raises(ingest.FastqFormatError) as ei:
        ingest.parse_fastq_bytes(text)
    assert ei.value.record == 1 and ei.value.flags == bit
    assert dict(ingest.FLAG_REASONS)[bit] in str(ei.value)


def test_first_bad_with_several_flagged_records():
    with ingest.parse_fastq_bytes(ic.cases()["flags_late"], strict=False, fetch=False) as rec:
        assert rec.info["first_bad"] == 700 and rec.info["len_mismatch"] == 1 and rec.info["bad_header"] == 1
        assert rec.seq is None   # nothing fetched
        assert np.flatnonzero(rec.fetch_flags()).tolist() == [700, 1001]
        rec.fetch()
        assert rec.qual_off is not None and rec.qual_off[-1] == rec.off[-1] - 1


def test_gzip_files(tmp_path):
    text = ic.cases()["crlf"]
    p = model("crlf")
    one, two, tail = tmp_path / "one.fastq.gz", tmp_path / "two.fastq.gz", tmp_path / "tail.fastq.gz"
    one.write_bytes(gzip.compress(text))
    two.write_bytes(ic.gz_members(text[:1234], text[1234:]))
    tail.write_bytes(gzip.compress(text) + b"\x00\x00not a member")
    for path in (one, two, tail):
        with ingest.read_fastq_records(str(path), strict=False) as rec:
            assert_equals_model(rec, p, path.name)
            assert rec.info["inflate_ms"] > 0
    assert ingest.read_fastq(str(two)) == flash.read_fastq(str(two)) == (p.names, p.seqs, p.quals)
    plain = tmp_path / "plain.fastq"
    plain.write_bytes(text)
    assert ingest.read_fastq(str(plain)) == flash.read_fastq(str(plain))
    empty = tmp_path / "empty.fastq"
    empty.write_bytes(b"")
    assert ingest.read_fastq(str(empty)) == ([], [], [])


def test_large_gzip_member(tmp_path):
    path = tmp_path / "many.fastq.gz"
    path.write_bytes(gzip.compress(ic.cases()["many_short_records"], compresslevel=1))
    with ingest.read_fastq_records(str(path), strict=True) as rec:
        assert_equals_model(rec, model("many_short_records"), "many.gz")


def test_damaged_gzip_is_refused(tmp_path):
    blob = gzip.compress(ic.cases()["crlf"])
    cut, second = tmp_path / "cut.fastq.gz", tmp_path / "second.fastq.gz"
    cut.write_bytes(blob[:len(blob) // 2])
    second.write_bytes(blob + blob[:len(blob) // 2])   # the second member is cut
    for path in (cut, second):
        with pytest.raises(ingest.IngestError) as ei:
            ingest.read_fastq_records(str(path))
        assert ei.value.code == -1 and "truncated" in str(ei.value)
    flipped = bytearray(blob)
    flipped[len(blob) // 2] ^= 0xFF
    bad = tmp_path / "bad.fastq.gz"
    bad.write_bytes(bytes(flipped))
    with pytest.raises(ingest.IngestError) as ei:
        ingest.read_fastq_records(str(bad))
    assert ei.value.code == -1
    with pytest.raises(ingest.IngestError):
        ingest.read_fastq_records(str(tmp_path / "absent.fastq"))


@pytest.mark.parametrize("name", ["many_short_records", "flags_late", "long_record"])
def test_three_repeats_byte_for_byte(name):
    text = ic.cases()[name]
    runs = []
    for _ in range(3):
        with ingest.parse_fastq_bytes(text, strict=False) as rec:
            runs.append((rec.flags.tobytes(), rec.off.tobytes(), rec.name_off.tobytes(), rec.seq.tobytes(),
                         rec.qual.tobytes(), rec.names.tobytes(),
                         None if rec.qual_off is None else rec.qual_off.tobytes(),
                         {k: rec.info[k] for k in im.INFO_KEYS}))
    assert runs[0] == runs[1] == runs[2]


def test_closed_records_refuse():
    rec = ingest.parse_fastq_bytes(b"@a\nAC\n+\nII\n", fetch=False)
    rec.close()
    rec.close()
    with pytest.raises(ingest.IngestError):
        rec.fetch()
