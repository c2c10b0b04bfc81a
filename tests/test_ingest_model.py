"""The FASTQ ingest's CPU restatements (tests/ingest_model.py) against flash.read_fastq, the
reader they restate, on every case of tests/ingest_cases.py and on random texts; the flags against
hand-written cases; the refusals the library makes before it touches a device."""
import ctypes
import gzip

import numpy as np
import pytest

from crispresso_amd import _lib
from crispresso_amd.flash import read_fastq
from tests import ingest_cases as ic
from tests import ingest_model as im


def same(a: im.Parsed, b: im.Parsed, what):
    assert a.names == b.names, what
    assert a.seqs == b.seqs, what
    assert a.quals == b.quals, what
    assert a.flags.tolist() == b.flags.tolist(), what
    assert a.info() == b.info(), what


def check_text(text: bytes, path, lanes: bool, what):
    with open(path, "wb") as f:
        f.write(text)
    names, seqs, quals = read_fastq(str(path))
    a, b = im.parse_lines(text), im.parse_positions(text, lanes=lanes)
    assert (a.names, a.seqs, a.quals) == (names, seqs, quals), what
    same(a, b, what)
    return a


@pytest.mark.parametrize("name", sorted(ic.cases()))
def test_models_equal_read_fastq(tmp_path, name):
    text = ic.cases()[name]
    a = check_text(text, tmp_path / "x.fastq", len(text) <= ic.SMALL, name)
    s = a.streams()
    assert len(s["off"]) == a.n + 1 and int(s["off"][-1]) == len(s["seq"])
    if not a.flags.any():
        assert np.array_equal(s["off"], s["qual_off"])


def test_models_equal_read_fastq_on_random_texts(tmp_path):
    path = tmp_path / "r.fastq"
    seen = set()
    for k, text in enumerate(ic.random_texts(20000, 14)):
        if text in seen:
            continue
        seen.add(text)
        check_text(text, path, True, (k, text))
    longer = ic.random_texts(400, 120, seed=7)
    assert max(len(im.parse_lines(t).seqs) for t in longer) >= 8
    for k, text in enumerate(longer):
        check_text(text, path, True, (k, text))


def test_gzip_files_read_the_same(tmp_path):
    text = ic.cases()["crlf"]
    path = tmp_path / "x.fastq.gz"
    path.write_bytes(ic.gz_members(text[:1000], text[1000:]))
    assert gzip.decompress(path.read_bytes()) == text
    a = im.parse_lines(text)
    assert read_fastq(str(path)) == (a.names, a.seqs, a.quals)


@pytest.mark.parametrize("k", range(len(ic.HAND_FLAGS)))
def test_flags_by_hand(k):
    text, flags = ic.HAND_FLAGS[k]
    for p in (im.parse_lines(text), im.parse_positions(text, lanes=True)):
        assert p.flags.tolist() == flags
        bad = [r for r, f in enumerate(flags) if f]
        assert p.info()["first_bad"] == (bad[0] if bad else -1)
        for bit, key in ((1, "bad_header"), (2, "bad_plus"), (4, "len_mismatch"), (8, "bad_qual")):
            assert p.info()[key] == sum(1 for f in flags if f & bit)


def test_cases_cover_what_they_are_for():
    c = ic.cases()
    assert [len(c[f"size_{s}"]) for s in (0, 1, 15, 16, 17, 4095, 4096, 4097)] == [0, 1, 15, 16, 17, 4095, 4096, 4097]
    assert [im.parse_lines(c[f"lines_mod4_{e}"]).info()["trailing_lines"] for e in range(4)] == [0, 1, 2, 3]
    assert [im.parse_lines(c[f"records_{n}"]).n for n in (255, 256, 257)] == [255, 256, 257]
    assert im.parse_lines(c["only_newlines"]).info()["lines"] == 37
    assert im.parse_lines(c["long_record"]).info()["lmax"] == 70000
    p = im.parse_lines(c["header_lengths"])
    assert {len(n) for n in p.names} == set(range(8)) and {len(s) for s in p.seqs} == set(range(10))
    assert im.parse_lines(c["flags_late"]).info()["first_bad"] == 700
    assert im.parse_lines(c["flags_late"]).flags[[700, 1001]].tolist() == [4, 1]
    assert im.parse_lines(c["quality_edges"]).flags.tolist() == [8, 0, 8, 8]
    p = im.parse_lines(c["cr_inside"])
    assert p.names == [b"a\rb", b"c"] and p.seqs == [b"AC\rGT", b"A\r\rC"]
    assert im.parse_lines(c["cr_only_lines"]).seqs == [b"", b""] * 3


def test_refusals_before_any_device_work():
    lib = _lib.load()
    h = ctypes.c_void_p()
    one = np.zeros(16, np.uint8)
    assert lib.nwi_parse_text(0, _lib.ptr(one), (1 << 32) - 16, ctypes.byref(h)) == -3
    msg = lib.nwi_last_error().decode()
    assert "2^32" in msg and "out of scope" in msg and not h.value
    assert lib.nwi_parse_text(0, _lib.ptr(one), (1 << 32) + 5, ctypes.byref(h)) == -3
    assert lib.nwi_parse_text(0, None, 5, ctypes.byref(h)) == -1
    assert lib.nwi_parse_text(0, _lib.ptr(one), -1, ctypes.byref(h)) == -1
    assert lib.nwi_parse_file(0, b"/nonexistent/reads.fastq", ctypes.byref(h)) == -1
    assert "cannot read" in lib.nwi_last_error().decode()
    assert lib.nwi_info(None, None) == -1
    lib.nwi_release(None)


def test_damaged_gzip_is_refused_before_any_device_work(tmp_path):
    """The inflate runs on the host before the device is touched: a cut or damaged member is -1
    with its message whether or not there is a GPU; a sound file gets as far as the device."""
    lib = _lib.load()
    blob = ic.gz_members(ic.cases()["crlf"][:3000], ic.cases()["crlf"][3000:])
    first = len(gzip.compress(ic.cases()["crlf"][:3000], mtime=0))
    flipped = bytearray(blob)
    flipped[first // 2] ^= 0xFF
    files = {"cut_first": blob[:first // 2], "cut_second": blob[:first + (len(blob) - first) // 2],
             "header_only": blob[:7], "flipped": bytes(flipped)}
    for name, data in files.items():
        path = tmp_path / (name + ".fastq.gz")
        path.write_bytes(data)
        h = ctypes.c_void_p()
        assert lib.nwi_parse_file(0, str(path).encode(), ctypes.byref(h)) == -1, name
        msg = lib.nwi_last_error().decode()
        assert not h.value and "gzip member" in msg, (name, msg)
        if name.startswith("cut") or name == "header_only":
            assert "truncated" in msg and ("member 1" in msg) == (name == "cut_second"), (name, msg)
    sound = tmp_path / "sound.fastq.gz"
    sound.write_bytes(blob + b"\0\0 trailing bytes that start no member")
    h = ctypes.c_void_p()
    rc = lib.nwi_parse_file(0, str(sound).encode(), ctypes.byref(h))
    assert rc in (0, -4), lib.nwi_last_error().decode()   # -4: no GPU here
    if rc == 0:
        lib.nwi_release(h)


def test_header_and_binding_agree():
    from tests.test_abi import declared_symbols

    assert declared_symbols("crispr_ingest.h", "nwi_") == set(_lib.INGEST_EXPORTS)
    assert declared_symbols("crispr_front.h", "nwp_") == set(_lib.FRONT_EXPORTS)
    exported = _lib.exported_symbols()
    for name in _lib.INGEST_EXPORTS + _lib.FRONT_EXPORTS:
        assert exported[name], name
