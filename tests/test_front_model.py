"""CPU: the front end's restatement (tests/front_model.py) and the inputs of the GPU tests
(tests/test_gpu_front.py): the generator's families with fixed seeds reach the floors the packer
test needs, so a seed change cannot quietly empty one; the binding's host-side refusals."""
import numpy as np
import pytest

from tests import front_model as fm


def test_packer_input_reaches_the_floors():
    pairs, e = fm.packer_case()
    f = fm.floors(e)
    assert len(pairs) == fm.PACKER_PAIRS
    assert f["combined"] >= 2049          # two full 1024-read length groups and a partial one
    assert f["not_combined"] >= 100
    assert f["trimmed"] >= 50
    assert f["filtered"] >= 50
    assert f["exceptions"] >= 100
    assert f["outies"] >= 1
    assert f["len_mod4"] == [0, 1, 2, 3]
    assert f["starts_mid_dword"] >= 1 and f["ends_mid_dword"] >= 1
    assert sum(e.trim.values()) == len(pairs) - f["filtered"]
    assert all(40 <= len(p[0]) <= 150 and 40 <= len(p[2]) <= 150 for p in pairs)


def test_model_batch_is_consistent():
    pairs, e = fm.packer_case()
    assert len(e.src) == len(e.reads) == len(e.lens) == len(e.offsets) - 1
    assert np.all(np.diff(e.src) > 0)
    assert np.array_equal(np.flatnonzero(e.status >= fm.COMBINED), e.src)
    assert set(np.unique(e.buf)) <= set(b"ACGTN")
    # the exceptions of the merged text are its N, ascending
    assert np.array_equal(e.packed.exc_pos, np.flatnonzero(e.buf == ord("N")))
    assert np.all(e.packed.exc_byte == ord("N"))
    # 2 bits per base, (byte >> 1) & 3, 0 at an exception, unused bits of the last byte 0
    total = int(e.offsets[-1])
    code = np.where(e.buf == ord("N"), 0, (e.buf >> 1) & 3).astype(np.uint8)
    code = np.concatenate([code, np.zeros(-total % 4, np.uint8)]).reshape(-1, 4)
    want = code[:, 0] | code[:, 1] << 2 | code[:, 2] << 4 | code[:, 3] << 6
    assert np.array_equal(e.packed.packed[:(total + 3) // 4], want)


def test_single_end_model_keeps_bytes_as_given():
    pairs = [(b"ACGTacgtRN", b"IIIIIIIIII", b"", b""), (b"", b"", b"", b""), (b"TTTT", b"!!!!", b"", b"")]
    e = fm.expected(pairs, single_end=True)
    assert e.status.tolist() == [fm.COMBINED] * 3
    assert e.reads == [b"ACGTacgtRN", b"", b"TTTT"]
    assert e.packed.exc_byte.tobytes() == b"RN" and e.packed.exc_pos.tolist() == [8, 9]
    e = fm.expected(pairs[::2], single_end=True, min_bp_quality=10)
    assert e.status.tolist() == [fm.COMBINED, fm.FILTERED]


def test_alignment_input():
    amp, pairs = fm.align_case()
    assert len(amp) == 200 and len(pairs) == 3000
    assert all(len(p[0]) == 120 and len(p[2]) == 120 for p in pairs)
    assert set(amp) <= set("ACGT")


def test_frontend_refusals_on_the_host():
    """What prepare_packed refuses before it reaches the library (no GPU needed)."""
    from crispresso_amd import frontend
    from crispresso_amd.trim import UnsupportedTrimStep

    s, q, off = np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"IIII", np.uint8), np.array([0, 4], np.int64)
    with pytest.raises(UnsupportedTrimStep):
        frontend.prepare_packed(None, s, q, off, s, q, off, trim="MAXINFO:40:0.5")
    with pytest.raises(UnsupportedTrimStep):
        frontend.prepare_packed(None, s, q, off, s, q, off, trim="LEADING:3 ILLUMINACLIP:x.fa:2:30:10")
    off0 = np.array([0, 4, 4], np.int64)
    with pytest.raises(ValueError):
        frontend.prepare_packed(None, s, q, off0, s, q, off0, min_bp_quality=20)
