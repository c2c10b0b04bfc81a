"""The around-cut windows on the device (crispresso_amd/csrc/nw_windows.hip, nwa_windows_device
of include/crispr_alleles.h) against a plain Python expansion, slice and dict over hand-built
runs (tests/around_cut_cases.py), and alleles.around_cut_tables on the aligner's resident batch
against around_cut_from_alleles(allele_table(...)), the host path it replaces."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from crispresso_amd import _lib, alleles, quantify, synth
from tests import alleles_cases as ac
from tests import around_cut_cases as cc
from tests.test_around_cut_host import assert_around_equal, assert_form

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = {b.name: b for b in cc.batches()}


@pytest.fixture(scope="module")
def nwa():
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    assert lib.nwa_create(0, ctypes.byref(ctx)) == 0
    yield lib, ctx
    lib.nwa_destroy(ctx)


def check(nwa, batch, cuts, offset, keep=None, tag=None, lead=0, bias=0, calls=2):
    lib, ctx = nwa
    want = [cc.expected(batch, c, offset, keep, tag) for c in cuts]
    assert all(w is not None for w in want)
    for _ in range(calls):     # the second call reuses the context's buffers
        rc, bad, first_bad, got, ng = cc.device_windows(lib, ctx, batch, cuts, offset, keep, tag, lead, bias)
        assert rc == 0, lib.nwa_last_error(ctx)
        assert (bad, first_bad) == (0, -1)
        assert ng == [len(w[0]) for w in want]
        for g, w in zip(got, want):
            assert g == w
            assert all(a < b for a, b in zip(g[0], g[0][1:]))
        assert lib.nwa_windows_collided(ctx) == 0
    rc, bad, _, got, _ = cc.device_windows(lib, ctx, batch, cuts, offset, keep, tag, lead, bias, want_gor=False)
    assert rc == 0 and bad == 0
    assert [g[:2] + g[3:] for g in got] == [w[:2] + w[3:] for w in want]


def good_cuts(batch, offset):
    """The cut points of the recorded cases the device path takes and every read has a column for."""
    cuts = [c for b, c, o in cc.combos() if b.name == batch.name and o == offset and 0 <= c < len(batch.amp)]
    return [c for c in cuts if cc.expected(batch, c, offset) is not None]


@pytest.mark.parametrize("offset", cc.OFFSETS)
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_windows_equal_expansion(nwa, name, offset):
    """Every hand-built case at every cut point of the host list: all cut points in one call
    (more than one launch takes), and K = 1, 2, 3."""
    b = BATCHES[name]
    cuts = good_cuts(b, offset)
    assert cuts
    check(nwa, b, cuts, offset)
    for k in (1, 2, 3):
        check(nwa, b, (cuts * 3)[1:1 + k], offset, calls=1)
    wins = [w for c in cuts for w in cc.expected(b, c, offset)[4]]
    if name == "plain" and offset == 20:
        assert ("", "") in wins                                           # win_len 0
        assert any(len(a) < 2 * offset for a, _ in wins)                  # a clipped stop or a wrapped start


def test_run_edges(nwa):
    """The cut base in the first and the last column of a run, X runs directly before and after
    the cut column, offsets between 1 and the largest the device takes."""
    b = BATCHES["plain"]
    check(nwa, b, [18, 19, 21, 22], 3, calls=1)       # M19 Y3 M..: last of M, first / last of Y, first of M
    check(nwa, b, [29, 30, 31], 2, calls=1)           # M31 X3 / M30 X2 / M30 Y1
    check(nwa, b, [30, 59], 64, calls=1)
    check(nwa, b, [0, 30], 33, calls=1)


def test_no_cut_column(nwa):
    """aln_len > awidth with the cut column on either side of awidth: the pairs without a column
    and the first such read are reported, and nothing is kept to fetch."""
    lib, ctx = nwa
    b = BATCHES["cut_rows"]
    check(nwa, b, [25, 29], 20, calls=1)
    for cuts, keep in (([30], None), ([25, 34, 40], None), ([29, 30], [0, 1, 1]), ([34], [0, 1, 1]), ([35], [1, 0, 0])):
        rc, bad, first_bad, got, ng = cc.device_windows(lib, ctx, b, cuts, 20, keep=keep)
        assert rc == 0, lib.nwa_last_error(ctx)
        assert (bad, first_bad) == cc.expected_no_cut(b, cuts, 20, keep)
        if bad:
            assert ng == [0] * len(cuts) and got == []
            assert lib.nwa_windows_fetch(ctx, 0, None, None, None, None, None, None) == _lib.NW_E_INVALID
        else:
            assert got == [cc.expected(b, c, 20, keep) for c in cuts]
    assert cc.expected_no_cut(b, [30], 20)[0] == 1 and cc.expected_no_cut(b, [34], 20, [0, 1, 1])[0] == 0


def test_empty_and_keep(nwa):
    b = BATCHES["plain"]
    empty = cc.Batch("empty", b.amp, 5000, [])
    check(nwa, empty, [30], 20)
    n = len(b.reads)
    check(nwa, b, [30, 40], 20, keep=np.zeros(n, np.uint8))
    check(nwa, b, [30, 40], 20, keep=(np.arange(n) % 3 == 0).astype(np.uint8))
    check(nwa, b, [30], 20, keep=(np.arange(n) % 2 == 1).astype(np.uint8), tag=np.arange(n, dtype=np.int32) % 2)
    # the same window under two tags is two groups
    tag = np.arange(n, dtype=np.int32) % 2
    assert len(cc.expected(b, 30, 20, None, tag)[0]) > len(cc.expected(b, 30, 20)[0])
    check(nwa, b, [30], 20, tag=tag, calls=1)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_every_start_alignment_and_bias(nwa, lead):
    b = BATCHES["plain"]
    check(nwa, b, [19, 30], 20, lead=lead, calls=1)
    check(nwa, BATCHES["n_ref"], [30], 20, lead=lead, bias=1000003, calls=1)


def test_limits_are_refused(nwa):
    lib, ctx = nwa
    b = BATCHES["plain"]
    for cuts, offset in (([30], 0), ([30], 65), ([-1], 20), ([len(b.amp)], 20)):
        rc, _, _, got, _ = cc.device_windows(lib, ctx, b, cuts, offset)
        assert rc == _lib.NW_E_UNSUPPORTED and got == []
    iupac = cc.Batch("iupac", b.amp[:10] + "R" + b.amp[11:], 5000, b.distinct)
    assert cc.device_windows(lib, ctx, iupac, [30], 20)[0] == _lib.NW_E_UNSUPPORTED
    lower = cc.Batch("lower", b.amp[:10].lower() + b.amp[10:], 5000, b.distinct)
    assert cc.device_windows(lib, ctx, lower, [30], 20)[0] == _lib.NW_E_UNSUPPORTED


def test_one_window_20000_reads(nwa):
    b = cc.repeated_batch(20000, distinct=False)
    assert len(cc.expected(b, 30, 20)[0]) == 1 and cc.expected(b, 30, 20)[3] == [1]
    check(nwa, b, [30], 20, calls=1)
    check(nwa, b, [30, 3], 20, keep=(np.arange(20000) % 7 != 0).astype(np.uint8), lead=3, calls=1)


def test_distinct_windows_20000_reads(nwa):
    b = cc.repeated_batch(20000, distinct=True)
    assert len(cc.expected(b, 30, 20)[0]) == 20000
    check(nwa, b, [30], 20, lead=1, calls=1)


def test_every_wavefront_takes_several_records(nwa):
    lib, ctx = nwa
    n = 2 * int(lib.nwa_reads_per_step(ctx)) + 5
    check(nwa, cc.repeated_batch(n, distinct=False), [30, 6], 20, calls=1)


@pytest.mark.parametrize("bits", [0, 3, 12])
def test_forced_collisions(bits):
    """CRISPR_NWA_HASH_BITS cuts the hash of the records to `bits` bits (a child process each):
    the collided records go through the exact host path and the groups are still the dict's."""
    env = dict(os.environ, CRISPR_NWA_HASH_BITS=str(bits))
    p = subprocess.run([sys.executable, "-m", "tests.around_cut_cases", "forced"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"], out
    assert all(c > 0 for c in out["collided"]), out


# ------------------------------------------------------------------ after the aligner

@pytest.fixture(scope="module")
def gq():
    q = quantify.GpuQuantifier(0)
    yield q
    q.close()


def aligned_resident(al, gq, amp, buf, off, min_identity, packed=True, guide=None, window=1):
    """The batch aligned and quantified resident -> (OpsBatch, keep, nwq_read results)."""
    from crispresso_amd.aligner import pack_2bit
    from crispresso_amd.devmem import DeviceBuffer
    from tests.test_gpu_alleles import kept_reads, quant_args

    n = len(off) - 1
    al.set_reference(amp)
    al.set_output("ops")
    if packed:
        al.upload_packed(pack_2bit(buf, off))
    else:
        al.upload(buf, off)
    al.run_async()
    al.sync()
    dev = al.device_ops()
    ob = al.download_ops(n)
    keep, score = kept_reads(ob.stats, min_identity)
    args = quant_args(amp)
    if guide is not None:
        args.guide_seq, args.window_around_sgrna = guide, window
    gq.set_params(quantify.globals_from_args(args), args)
    with DeviceBuffer.from_array(quantify.pre_flags(score == 100)) as d_pre, DeviceBuffer(16 * n) as d_out:
        gq.run_device_ops(amp, dev, d_pre.ptr, n, d_out.ptr)
        rr = d_out.download(np.zeros((n, 4), np.int32))
    return ob, keep, rr


def host_tables(al, amp, buf, off, ob, rr, keep, cuts, offset, tag=None):
    groups = alleles.group_reads_host(buf, off, keep=keep, tag=tag)
    table = alleles.allele_table(amp, buf, off, ob, rr, groups)
    return table, [alleles.around_cut_from_alleles(table, c, offset) for c in cuts]


def check_resident(al, gq, amp, buf, off, min_identity, packed=True):
    ob, keep, rr = aligned_resident(al, gq, amp, buf, off, min_identity, packed)
    cuts = [len(amp) // 2, 7, len(amp) - 4]            # the middle, and within `offset` of each end
    grouper = alleles.default_grouper(al.device)
    got = alleles.around_cut_tables(al, amp, buf, off, rr, cuts, 20, keep=keep)
    assert grouper.window_times()["extract"] > 0       # the device path ran
    table, want = host_tables(al, amp, buf, off, ob, rr, keep, cuts, 20)
    for g, w in zip(got, want):
        assert_form(g)
        assert_around_equal(g, w)
        assert int(g["#Reads"].sum()) == int(keep.sum())
    assert 0 < len(got[0]) < len(table)
    return got, keep


def test_after_aligner_c2(gpu_aligner_factory, gq):
    amp = synth.random_amplicon(250, 31)
    buf, off = synth.reads_from(amp, 12000, 32)
    check_resident(gpu_aligner_factory(), gq, amp, buf, off, 60.0)


def test_after_aligner_parity_mix(gpu_aligner_factory, gq):
    """N bytes and reverse-complemented reads, which the identity filter drops."""
    amp = synth.random_amplicon(250, 33)
    buf, off = synth.reads_from(amp, 12000, 34, synth.PARITY_MIX)
    _, keep = check_resident(gpu_aligner_factory(), gq, amp, buf, off, 60.0)
    assert 0 < int(keep.sum()) < len(keep)


def test_after_aligner_short_reads(gpu_aligner_factory, gq):
    """151-bp reads on a 280-bp amplicon, min_identity 30: most windows near an end are end gaps."""
    amp = synth.random_amplicon(280, 35)
    buf, off = synth.window_reads(amp, 12000, 36, 151)
    check_resident(gpu_aligner_factory(), gq, amp, buf, off, 30.0, packed=False)


def hand_results(buf, off, amp):
    """nwq_read results without a quantifier: class 0 for the amplicon's own bytes, else 1."""
    rr = np.zeros((len(off) - 1, 4), np.int32)
    a = amp.upper().encode()
    rr[:, 0] = [bytes(buf[off[r]:off[r + 1]]).upper() != a for r in range(len(off) - 1)]
    return rr


def test_pooled_tags(gpu_aligner_factory):
    """3 amplicons x 2,000 reads in one pooled pass (align_multi_ops), tag = ref_of_read, one cut
    point per amplicon: the pass leaves no resident batch, so its arrays are uploaded here."""
    from crispresso_amd.devmem import DeviceBuffer
    from tests.test_gpu_alleles import kept_reads

    al = gpu_aligner_factory()
    amps = [synth.random_amplicon(250, 40 + a) for a in range(3)]
    reads, tag = [], []
    for a, amp in enumerate(amps):
        b, o = synth.reads_from(amp, 2000, 50 + a)
        reads += [bytes(b[o[r]:o[r + 1]]) for r in range(2000)]
        tag += [a] * 2000
    tag = np.array(tag, np.int32)
    buf, off = ac.pack(reads)
    ob = al.align_multi_ops(amps, buf, off, tag)
    keep, _ = kept_reads(ob.stats, 30.0)
    ops = np.append(np.ascontiguousarray(ob.ops, np.uint32), np.uint32(0))
    with DeviceBuffer.from_array(buf) as d_buf, DeviceBuffer.from_array(off + 7) as d_off, \
            DeviceBuffer.from_array(ops) as d_ops, DeviceBuffer.from_array(ob.ops_off) as d_ops_off, \
            DeviceBuffer.from_array(ob.stats) as d_stats:
        dev = {"ops": d_ops.ptr, "ops_off": d_ops_off.ptr, "stats": d_stats.ptr, "reads": d_buf.ptr,
               "offsets": d_off.ptr, "reads_bias": 7}
        for a, amp in enumerate(amps):
            rr = hand_results(buf, off, amp)
            mine = keep & (tag == a)
            cut = 100 + 20 * a
            got = alleles.around_cut_tables(None, amp, buf, off, rr, [cut], 20, keep=mine, tag=tag, ops_batch=ob,
                                            dev=dev)
            assert alleles.default_grouper(0).window_times()["extract"] > 0
            _, want = host_tables(al, amp, buf, off, ob, rr, mine, [cut], 20, tag=tag)
            assert_form(got[0])
            assert_around_equal(got[0], want[0])
            assert int(got[0]["#Reads"].sum()) == int(mine.sum())


def test_reference_pin(tmp_path, gpu_aligner_factory, gq):
    """The reference's `test` run from the raw pairs: the table around its guide's cut point
    equals the host path's, and its top row is the unedited window."""
    import gzip

    from crispresso_amd import fastq
    from crispresso_amd.flash import FlashOptions, run_flash
    from tests.test_e2e_pin import CASES, HERE, restated_merge

    case = dict(CASES["test"], name="test")
    with gzip.open(os.path.join(HERE, case["fixture"]), "rt") as f:
        fx = json.load(f)
    r1, r2 = restated_merge(case, tmp_path)
    st = run_flash(r1, r2, str(tmp_path), options=FlashOptions(min_overlap=4, max_overlap=100, allow_outies=True))
    assert st["combined"] == case["merged"]
    names, buf, off = fastq.read_fastq_as_fasta(str(tmp_path / "out.extendedFrags.fastq.gz"))
    amp = fx["amplicon_seq"].upper()
    al = gpu_aligner_factory()
    ob, keep, rr = aligned_resident(al, gq, amp, buf, off, case["min_identity"], packed=False, guide=fx["guide_seq"],
                                    window=case["window"])
    cuts = [int(c) for c in quantify.compute_cut_points(amp, fx["guide_seq"])]
    assert cuts and all(19 <= c < len(amp) - 20 for c in cuts)      # (the guide also matches on the other strand)
    got = alleles.around_cut_tables(al, amp, buf, off, rr, cuts, 20, keep=keep)
    assert alleles.default_grouper(al.device).window_times()["extract"] > 0
    _, want = host_tables(al, amp, buf, off, ob, rr, keep, cuts, 20)
    for c, g, w in zip(cuts, got, want):
        assert_form(g)
        assert_around_equal(g, w)
        assert int(g["#Reads"].sum()) == 7058
        window = amp[c - 19: c + 21]
        top = g.iloc[0]
        assert g.index[0] == window and top["Reference_Sequence"] == window and bool(top["Unedited"])


def test_routing(gpu_aligner_factory, monkeypatch):
    """A lower-case read byte, an IUPAC amplicon and offset 65 each take the host path (the
    device entry point is not called) and give the host path's frames."""
    amp = synth.random_amplicon(250, 61)
    buf, off = synth.reads_from(amp, 2000, 62)
    n = len(off) - 1
    lower = buf.copy()
    lower[off[5] + 40] |= 0x20
    iupac = amp[:60] + "R" + amp[61:]
    al = gpu_aligner_factory()

    def refuse(*a, **k):
        raise AssertionError("the device path was taken")

    for amp_k, buf_k, offset in ((amp, lower, 20), (iupac, buf, 20), (amp, buf, 65)):
        al.set_reference(amp_k)
        al.set_output("ops")
        al.upload(buf_k, off)
        al.run_async()
        al.sync()
        ob = al.download_ops(n)
        rr = hand_results(buf_k, off, amp_k)
        monkeypatch.setattr(alleles.GpuAlleleGrouper, "windows", refuse)
        got = alleles.around_cut_tables(al, amp_k, buf_k, off, rr, [125, 240], offset)
        monkeypatch.undo()
        _, want = host_tables(al, amp_k, buf_k, off, ob, rr, None, [125, 240], offset)
        for g, w in zip(got, want):
            assert_form(g)
            assert_around_equal(g, w)
    # and the same batch with nothing in the way goes through the device
    rr = hand_results(buf, off, amp)
    got = alleles.around_cut_tables(al, amp, buf, off, rr, [125, 240], 20)
    assert alleles.default_grouper(al.device).window_times()["extract"] > 0
    _, want = host_tables(al, amp, buf, off, ob, rr, None, [125, 240], 20)
    for g, w in zip(got, want):
        assert_around_equal(g, w)
