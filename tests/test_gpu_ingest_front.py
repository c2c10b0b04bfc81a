"""frontend.prepare_fastq_device (the files parsed on the GPU, nwi_parse_file, and handed to the
front end where they lie, nwp_prepare_records) against frontend.prepare_fastq (the interpreter's
reader and an upload) on files written from tests/front_model.py's pairs: status, src, buf,
offsets, lens, quals, the packed stream with its exceptions, the stats' counts, the names, and
the aligner's ops on the adopted batch; the refusals."""
import gzip

import numpy as np
import pytest

from crispresso_amd import frontend
from crispresso_amd.flash import FlashOptions
from tests import front_model as fm

pytestmark = pytest.mark.gpu
FLASH = FlashOptions(min_overlap=4, max_overlap=100, allow_outies=True)
AMP = "ACGT" * 50


def write_fastq(path, pairs, mate, eol=b"\n", gz=False, names=None):
    s, q = (0, 1) if mate == 1 else (2, 3)
    out = []
    for k, p in enumerate(pairs):
        name = names[k] if names else b"M0:%d:%d 1:N:0:1/%d" % (k, 7 * k, mate) if k % 3 else b"read%d/%d" % (k, mate)
        out.append(b"@" + name + eol + p[s] + eol + b"+" + eol + p[q] + eol)
    data = b"".join(out)
    with open(path, "wb") as f:
        f.write(gzip.compress(data, compresslevel=1) if gz else data)
    return str(path)


def with_reference(factory):
    al = factory()
    al.set_reference(AMP)
    return al


def run_ops(al, m):
    al.run_async()
    al.sync()
    return al.download_ops(m)


def assert_same_batch(got, want, what=""):
    (pb, names), (pe, enames) = got, want
    for key in ("status", "src", "buf", "offsets", "lens", "quals"):
        a, b = getattr(pb, key), getattr(pe, key)
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, key)
    nb = (int(pe.offsets[-1]) + 3) // 4
    assert np.array_equal(pb.packed.packed[:nb], pe.packed.packed[:nb]), what
    assert np.array_equal(pb.packed.exc_pos, pe.packed.exc_pos), what
    assert np.array_equal(pb.packed.exc_byte, pe.packed.exc_byte), what
    counts = [k for k in pe.stats if not k.endswith("_ms")]
    assert {k: pb.stats[k] for k in counts} == {k: pe.stats[k] for k in counts}, what
    assert names == enames, what


def both(factory, r1, r2, **kw):
    """The two paths on two contexts, the batches compared, then the aligner's ops on each."""
    kw.setdefault("flash", FLASH)
    out = []
    for fn in (frontend.prepare_fastq_device, frontend.prepare_fastq):
        al = with_reference(factory)
        out.append((al, fn(al, r1, r2, with_quals=True, with_packed=True, **kw)))
    (al_d, got), (al_h, want) = out
    assert_same_batch(got, want)
    m = len(want[0])
    if m:
        a, b = run_ops(al_d, m), run_ops(al_h, m)
        assert np.array_equal(a.stats, b.stats) and np.array_equal(a.ops_off, b.ops_off) and np.array_equal(a.ops, b.ops)
    return got[0]


def test_paired_filter_clip_steps_merge(gpu_aligner_factory, tmp_path):
    pairs, e = fm.packer_case()
    r1, r2 = write_fastq(tmp_path / "r1.fastq", pairs, 1), write_fastq(tmp_path / "r2.fastq", pairs, 2)
    pb = both(gpu_aligner_factory, r1, r2, trim=fm.PACKER_TRIM, **fm.PACKER_FILTER)
    assert np.array_equal(pb.status, e.status) and np.array_equal(pb.buf, e.buf)   # and the model's
    assert len(set(pb.status.tolist())) == 5


def test_single_end(gpu_aligner_factory, tmp_path):
    pairs, _ = fm.packer_case()
    r1 = write_fastq(tmp_path / "r1.fastq", pairs[:900], 1)
    pb = both(gpu_aligner_factory, r1, None, trim=["SLIDINGWINDOW:4:15", "LEADING:5", "MINLEN:40"], **fm.PACKER_FILTER)
    assert len(set(pb.status.tolist())) == 3
    both(gpu_aligner_factory, r1, None)   # no trim, no filter: every read whole


def test_mates_with_different_record_counts(gpu_aligner_factory, tmp_path):
    pairs, _ = fm.packer_case()
    r1 = write_fastq(tmp_path / "r1.fastq", pairs[:700], 1)
    r2 = write_fastq(tmp_path / "r2.fastq", pairs[:613], 2)
    pb = both(gpu_aligner_factory, r1, r2, trim=fm.PACKER_TRIM)
    assert pb.stats["pairs"] == 613 and len(pb.status) == 613
    pb = both(gpu_aligner_factory, r1, write_fastq(tmp_path / "r2b.fastq", pairs[:701], 2))
    assert pb.stats["pairs"] == 700


def test_crlf_and_gz_files(gpu_aligner_factory, tmp_path):
    pairs, _ = fm.packer_case()
    pairs = pairs[:800]
    plain = both(gpu_aligner_factory, write_fastq(tmp_path / "a1.fastq", pairs, 1),
                 write_fastq(tmp_path / "a2.fastq", pairs, 2), **fm.PACKER_FILTER)
    crlf = both(gpu_aligner_factory, write_fastq(tmp_path / "c1.fastq", pairs, 1, eol=b"\r\n"),
                write_fastq(tmp_path / "c2.fastq", pairs, 2, eol=b"\r\n"), **fm.PACKER_FILTER)
    gz = both(gpu_aligner_factory, write_fastq(tmp_path / "g1.fastq.gz", pairs, 1, gz=True),
              write_fastq(tmp_path / "g2.fastq.gz", pairs, 2, gz=True), **fm.PACKER_FILTER)
    for pb in (crlf, gz):
        assert np.array_equal(pb.buf, plain.buf) and np.array_equal(pb.status, plain.status)


def test_no_record_and_no_survivor(gpu_aligner_factory, tmp_path):
    empty = tmp_path / "e.fastq"
    empty.write_bytes(b"")
    pb = both(gpu_aligner_factory, str(empty), str(empty))
    assert len(pb) == 0 and pb.offsets.tolist() == [0]
    unrelated = [(b"ACGTTGCAAC" * 5, b"I" * 50, b"GATTACAGGA" * 5, b"I" * 50)] * 3
    pb = both(gpu_aligner_factory, write_fastq(tmp_path / "u1.fastq", unrelated, 1),
              write_fastq(tmp_path / "u2.fastq", unrelated, 2))
    assert pb.status.tolist() == [fm.NOT_COMBINED] * 3


def test_flagged_record_is_refused_and_the_batch_stays(gpu_aligner_factory, tmp_path):
    pairs, _ = fm.packer_case()
    good = pairs[:300]
    r1, r2 = write_fastq(tmp_path / "r1.fastq", good, 1), write_fastq(tmp_path / "r2.fastq", good, 2)
    al = with_reference(gpu_aligner_factory)
    pb, _ = frontend.prepare_fastq_device(al, r1, r2, flash=FLASH)
    before = run_ops(al, len(pb))
    off_before = al._off
    reasons = {
        "length": (lambda p: (p[0], p[1], p[2], p[3][:-1]), 2, "differ in length"),
        "quality": (lambda p: (p[0], b" " + p[1][1:], p[2], p[3]), 1, "33..126"),
    }
    for what, (spoil, mate, text) in reasons.items():
        bad = list(good)
        bad[41] = spoil(bad[41])
        bad[77] = spoil(bad[77])
        b1, b2 = write_fastq(tmp_path / f"{what}1.fastq", bad, 1), write_fastq(tmp_path / f"{what}2.fastq", bad, 2)
        with pytest.raises(frontend.FrontError) as ei:
            frontend.prepare_fastq_device(al, b1, b2, flash=FLASH)
        assert ei.value.code == -1 and f"record 41 of R{mate}" in str(ei.value) and text in str(ei.value), str(ei.value)
        with pytest.raises(frontend.FrontError) as ei:
            frontend.prepare_fastq(al, b1, b2, flash=FLASH)
        assert ei.value.code == -1
    # a header without '@' (the interpreter's reader does not look)
    raw = open(r1, "rb").read().replace(b"@read3/1", b"read3/1 ", 1)
    (tmp_path / "h1.fastq").write_bytes(raw)
    with pytest.raises(frontend.FrontError) as ei:
        frontend.prepare_fastq_device(al, str(tmp_path / "h1.fastq"), r2, flash=FLASH)
    assert ei.value.code == -1 and "record 3 of R1" in str(ei.value) and "'@'" in str(ei.value)
    # a flagged record past the pairs the call uses does not refuse it
    short2 = write_fastq(tmp_path / "s2.fastq", good[:40], 2)
    bad = list(good)
    bad[41] = (bad[41][0], bad[41][1][:-1], bad[41][2], bad[41][3])
    pb2, _ = frontend.prepare_fastq_device(with_reference(gpu_aligner_factory),
                                           write_fastq(tmp_path / "p1.fastq", bad, 1), short2, flash=FLASH)
    assert pb2.stats["pairs"] == 40
    # the context still holds the first batch
    assert al._off is off_before
    after = run_ops(al, len(pb))
    assert np.array_equal(after.stats, before.stats) and np.array_equal(after.ops, before.ops)


def test_long_record_is_refused(gpu_aligner_factory, tmp_path):
    pairs = [(b"A" * 4097, b"I" * 4097, b"T" * 50, b"I" * 50)] + fm.packer_case()[0][:5]
    r1, r2 = write_fastq(tmp_path / "r1.fastq", pairs, 1), write_fastq(tmp_path / "r2.fastq", pairs, 2)
    al = with_reference(gpu_aligner_factory)
    for fn in (frontend.prepare_fastq_device, frontend.prepare_fastq):
        with pytest.raises(frontend.FrontError) as ei:
            fn(al, r1, r2, flash=FLASH)
        assert ei.value.code == -3, fn.__name__


def test_empty_read_with_the_filter_on(gpu_aligner_factory, tmp_path):
    pairs = [(b"", b"", b"ACGT", b"IIII")] + fm.packer_case()[0][:5]
    r1, r2 = write_fastq(tmp_path / "r1.fastq", pairs, 1), write_fastq(tmp_path / "r2.fastq", pairs, 2)
    al = with_reference(gpu_aligner_factory)
    for fn in (frontend.prepare_fastq_device, frontend.prepare_fastq):
        with pytest.raises(ValueError):
            fn(al, r1, r2, flash=FLASH, min_bp_quality=20)
    both(gpu_aligner_factory, r1, r2)
