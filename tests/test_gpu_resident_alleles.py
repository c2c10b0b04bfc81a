"""The allele tables of a resident summary (crispresso_amd/csrc/nw_allele_rows.hip, nwa_table_device
/ nwa_table_fetch / nwa_windows_resident of include/crispr_alleles.h, the ``alleles`` keyword of
demux.summarize_pooled and regions.summarize_regions, the command lines' --alleles).

The kernels on hand-built device arrays (tests/resident_alleles_cases.py) against the host path on
the same reads, alleles.group_reads_host + nw_expand_ops_subset; the whole calls against the host
path they replace: the rows of every group on the host, the reference's filter on the printed
identity, quantify.quantify_alignments and quantify.run_summary on the kept rows, and
alleles.around_cut_from_alleles of that table.  Everything exact."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
from pandas.testing import assert_frame_equal

from crispresso_amd import _lib, alleles, demux, quantify, regions, report
from crispresso_amd.pooled import align_pooled
from tests import alleles_cases as ac
from tests import around_cut_cases as cc
from tests import hdr_summary_model as hm
from tests import regions_summary_cases as sc
from tests import resident_alleles_cases as rc_
from tests.alleles_cases import pack
from tests.resident_alleles_cases import M, X, Y
from tests.test_around_cut_host import assert_form
from tests.test_gpu_reports import host_frames, quant_args
from tests.test_gpu_summary import OPTS, SCORE, panel_rows, write_fastq

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nwa():
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    assert lib.nwa_create(0, ctypes.byref(ctx)) == 0
    yield lib, ctx
    lib.nwa_destroy(ctx)


@pytest.fixture(scope="module")
def d():
    with demux.GpuDemultiplexer(0) as x:
        yield x


@pytest.fixture(scope="module")
def gq():
    with quantify.GpuQuantifier(0) as q:
        yield q


def keep_flags(reads, pattern):
    """uint8 flags in 0, 1, 2 by `pattern` (a function of the read's index); 0 for the reads
    that must never be kept."""
    return np.array([0 if rd.get("drop") else pattern(j) for j, rd in enumerate(reads)], np.uint8)


# ---- nwa_table_device: the kernel against the host path ------------------------------------------

@pytest.mark.parametrize("la", [1, 63, 64, 65, 255, 256, 257])
def test_alignment_lengths_and_awidth(nwa, la):
    """Single-run alignments of la columns with awidth below, at and above la: the rows are cut
    to min(la, awidth) columns and row_stride follows the cut."""
    lib, ctx = nwa
    amp = rc_.amplicon(la)
    a = rc_.Arrays(amp, rc_.single_run_reads(amp), lead=la % 4)
    for awidth in sorted({max(la - 1, 1), la, la + 7}):
        rc, g, w, rows, cols, first, count, res = rc_.same_as_host(lib, ctx, a, None, awidth)
        assert set(cols) == {min(la, awidth)} and w == max(16, (min(la, awidth) + 15) & ~15)
        assert sum(count) == a.n and count[0] == 3 and first[0] == 0
    # cut to one column the groups stay (the reads' bytes differ) while their rows show the first base only
    if la >= 63:
        rc, g, w, rows, cols, first, count, res = rc_.same_as_host(lib, ctx, a, None, 1)
        assert w == 16 and len({bytes(rows[q, 0, :1]) for q in range(g)}) == 2      # the first base, and its substitution


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_read_counts_and_run_shapes(nwa, n):
    """The run shapes (a single M run, a leading Y and a trailing X run, 64 / 65 / 130 alternating
    runs, N / IUPAC / '-' bytes, a read of no byte that is not kept) cycled to n reads, with the
    keep flags 0, 1 and 2 in turn and with NULL; awidth below, at and above the longest
    alignment; every start alignment of the text and a bias."""
    lib, ctx = nwa
    amp = rc_.amplicon(257)
    distinct = rc_.shape_reads(amp)
    reads = rc_.cycled(distinct, n)
    a = rc_.Arrays(amp, reads, lead=n % 4, bias=1000003 if n % 2 else 0)
    longest = max((sum(l for _, l in rd["runs"]) for rd in reads), default=0)
    for awidth in sorted({100, max(longest, 1), longest + 9}):
        keep = keep_flags(reads, lambda j: (j // 5) % 3)
        got = rc_.same_as_host(lib, ctx, a, keep, awidth)
        if n >= 65:
            assert 0 < sum(got[6]) == int((keep != 0).sum()) < n and max(got[6]) > 1
            assert {1, 2} <= set(keep.tolist())
    # NULL keeps every read: the batch without the read that must not be kept
    kept_all = [rd for rd in reads if not rd.get("drop")]
    b = rc_.Arrays(amp, kept_all, lead=1)
    got = rc_.same_as_host(lib, ctx, b, None, 5000)
    assert sum(got[6]) == len(kept_all)
    if n == 257:
        assert got[1] == len(distinct) - 3                      # two repeats, and the read that is never kept
        rows, cols = got[3], got[4]
        texts = [bytes(rows[q, 0, :c]) for q, c in enumerate(cols)]
        assert any(b"N" in t and b"R" in t and b"-" in t for t in texts)
        assert any(t == b"-" * 257 for t in texts)              # the kept read of no byte
        assert max(cols) == 257 + 70 and got[2] == 336            # M40 X70 M217, rounded up to 16
        # all dropped: no group
        none = rc_.device_table(lib, ctx, b, np.zeros(b.n, np.uint8), 5000)
        assert none[:3] == (0, 0, 0)


def test_kept_read_of_no_byte_and_no_run(nwa):
    """nw_expand_ops_subset leaves such a read's row empty: zero columns, no error."""
    lib, ctx = nwa
    amp = rc_.amplicon(64)
    reads = [rc_.read_of(amp, [(M, 64)], cls=0), {"runs": [], "seq": b"", "cls": 0}, rc_.read_of(amp, [(M, 64)], cls=0)]
    got = rc_.same_as_host(lib, ctx, rc_.Arrays(amp, reads), None, 5000)
    assert got[4] == [64, 0] and got[6] == [2, 1]


def test_padding_over_a_used_buffer_and_two_runs_give_equal_bytes(nwa):
    """A wide table first, then a narrow one on the same context: the narrow rows are zero past
    their columns although the device buffer held the wide rows; the same call twice gives the
    same bytes."""
    lib, ctx = nwa
    amp = rc_.amplicon(257)
    wide = rc_.Arrays(amp, rc_.cycled(rc_.shape_reads(amp)[:11], 300))
    first = rc_.same_as_host(lib, ctx, wide, None, 5000)
    short = rc_.amplicon(20)
    narrow = rc_.Arrays(short, rc_.single_run_reads(short) + [rc_.read_of(short, [(M, 9), (Y, 11)])])
    got = rc_.same_as_host(lib, ctx, narrow, None, 5000)
    assert got[2] == 32 and 9 < min(got[4]) and not got[3][:, :, 20:].any()
    again = rc_.same_as_host(lib, ctx, wide, None, 5000)
    assert again[1:3] == first[1:3] and np.array_equal(again[3], first[3]) and again[4:] == first[4:]
    keep = keep_flags(wide.reads, lambda j: j % 3)
    one, two = rc_.device_table(lib, ctx, wide, keep, 120), rc_.device_table(lib, ctx, wide, keep, 120)
    assert one[:3] == two[:3] and np.array_equal(one[3], two[3]) and one[4:] == two[4:]


def test_runs_that_overrun_the_read_or_the_amplicon_are_refused(nwa):
    """NW_E_INVALID, nothing to fetch, and the context works afterwards.  The bytes past the end
    are never loaded: the kernel writes 0 for them."""
    lib, ctx = nwa
    amp = rc_.amplicon(70)
    good = rc_.read_of(amp, [(M, 70)], cls=0)
    other = (b"C" if good["seq"][:1] == b"A" else b"A") + good["seq"][1:]           # (other bytes: a group of its own)
    short_read = {"runs": [(M, 70)], "seq": good["seq"][:67], "cls": 1}                 # the run overruns the read
    long_runs = {"runs": [(M, 70), (Y, 5)], "seq": other, "cls": 1}                # ... the amplicon
    insertion = {"runs": [(M, 30), (X, 9), (M, 40)], "seq": good["seq"] + b"ACG", "cls": 1}   # 6 bytes short
    unknown = {"runs": [(M, 30), (5, 4), (M, 40)], "seq": other, "cls": 1}         # a run type that is none of M X Y
    uncovered = {"runs": [(M, 60)], "seq": good["seq"][:60], "cls": 1}                   # ends before the amplicon does
    for bad in (short_read, long_runs, insertion, unknown, uncovered):
        a = rc_.Arrays(amp, [good, bad, good])
        got = rc_.device_table(lib, ctx, a, None, 5000)
        assert got[:3] == (_lib.NW_E_INVALID, 0, 0), bad["runs"]
        assert b"do not match" in lib.nwa_last_error(ctx)
        assert lib.nwa_table_fetch(ctx, None, None, None, None, None) == 0
        # not kept: not looked at
        assert rc_.same_as_host(lib, ctx, a, np.array([1, 0, 2], np.uint8), 5000)[6] == [2]
    # fewer columns in the runs than the record counts
    a = rc_.Arrays(amp, [good], aln_len=[75])
    assert rc_.device_table(lib, ctx, a, None, 5000)[0] == _lib.NW_E_INVALID
    assert rc_.device_table(lib, ctx, a, None, 70)[0] == 0         # (cut to 70 columns the runs hold them)


def test_refusals(nwa):
    lib, ctx = nwa
    amp = rc_.amplicon(64)
    a = rc_.Arrays(amp, rc_.single_run_reads(amp))
    ng, stride = ctypes.c_int64(), ctypes.c_int32()
    args = (None, None, None, None, None, 0)
    assert lib.nwa_table_device(ctx, *args, 3, 5000, amp.encode(), 64, None, None, ctypes.byref(ng),
                                ctypes.byref(stride)) == _lib.NW_E_INVALID
    assert lib.nwa_table_device(ctx, *args, -1, 5000, amp.encode(), 64, None, None, ctypes.byref(ng),
                                ctypes.byref(stride)) == _lib.NW_E_INVALID
    assert lib.nwa_table_device(ctx, *args, 0, 0, amp.encode(), 64, None, None, ctypes.byref(ng),
                                ctypes.byref(stride)) == _lib.NW_E_INVALID
    assert lib.nwa_table_device(ctx, *args, 0, 5000, amp.encode(), 64, None, None, ctypes.byref(ng),
                                ctypes.byref(stride)) == 0 and ng.value == 0 and stride.value == 0
    assert rc_.same_as_host(lib, ctx, a, None, 5000)[1] == 4


def test_forced_collisions():
    """A grouper created under CRISPR_NWA_HASH_BITS=3 (a child process): the collided reads go
    through the exact host path, the merged first list is uploaded, and the rows are still the
    host path's."""
    env = dict(os.environ, CRISPR_NWA_HASH_BITS="3")
    p = subprocess.run([sys.executable, "-m", "tests.resident_alleles_cases", "forced"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"], out
    assert all(c > 0 for c in out["collided"]), out


def test_group_device_is_unchanged_and_agrees(nwa):
    """nwa_group_device's results on one of these inputs are what they were (the dict's), and
    the table's groups are the same groups."""
    lib, ctx = nwa
    amp = rc_.amplicon(257)
    reads = rc_.cycled(rc_.shape_reads(amp), 257)
    keep = keep_flags(reads, lambda j: (j // 5) % 3)
    texts = [rd["seq"] for rd in reads]
    for k in (keep, None if not any(rd.get("drop") for rd in reads) else keep_flags(reads, lambda j: 1)):
        want = ac.expected_groups(texts, k)
        rc, first, count, gor, ng = ac.device_group(lib, ctx, texts, keep=k, lead=3, bias=77)
        assert rc == 0 and (first, count, gor) == want and ng == len(want[0])
        got = rc_.device_table(lib, ctx, rc_.Arrays(amp, reads, lead=3, bias=77), k, 5000)
        assert got[5] == first and got[6] == count
    assert lib.nwa_last_collided(ctx) == 0


# ---- nwa_windows_resident ----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["plain", "n_ref"])
def test_windows_resident_equals_windows_device(nwa, name):
    lib, ctx = nwa
    b = {x.name: x for x in cc.batches()}[name]
    n = len(b.reads)
    cuts = [0, 18, 19, 30, 40, 59]                # more than one launch takes
    tag = np.arange(n, dtype=np.int32) % 2
    for keep, t in ((None, None), ((np.arange(n) % 3).astype(np.uint8), None), ((np.arange(n) % 2 * 2).astype(np.uint8), tag),
                    (np.zeros(n, np.uint8), None)):
        for offset in (1, 20, 64):
            want = cc.device_windows(lib, ctx, b, cuts, offset, keep=keep, tag=t)
            got = rc_.device_windows_resident(lib, ctx, b, cuts, offset, keep=keep, tag=t)
            assert want[0] == 0 and got == want
            assert got[3] == [cc.expected(b, c, offset, keep, t) for c in cuts]
    empty = cc.Batch("empty", b.amp, 5000, [])
    assert rc_.device_windows_resident(lib, ctx, empty, [30], 20) == cc.device_windows(lib, ctx, empty, [30], 20)
    # the no-cut report and the limits are the same
    cut_rows = {x.name: x for x in cc.batches()}["cut_rows"]
    for c, keep in (([30], None), ([34], [0, 1, 1]), ([35], [1, 0, 0])):
        got = rc_.device_windows_resident(lib, ctx, cut_rows, c, 20, keep=keep)
        assert got == cc.device_windows(lib, ctx, cut_rows, c, 20, keep=keep)
        assert got[1:3] == cc.expected_no_cut(cut_rows, c, 20, keep)
    for c, offset in (([30], 0), ([30], 65), ([-1], 20), ([len(b.amp)], 20)):
        assert rc_.device_windows_resident(lib, ctx, b, c, offset)[0] == _lib.NW_E_UNSUPPORTED


# ---- summarize_pooled(reports=..., alleles=True) -----------------------------------------------

def host_alleles(row, batch, batch_hdr, gq, offset=20):
    """(df_alleles, cut points) of the host path on the kept rows, as check_report of
    tests/test_gpu_reports.py builds them."""
    hdr = row.get("Expected_HDR") if batch_hdr is not None else None
    kept, _ = host_frames(batch, batch_hdr, SCORE)
    args = quant_args(row, hdr)
    out = quantify.quantify_alignments(kept.copy(), args, quantifier=gq, globals_=quantify.globals_from_args(args))
    cuts = quantify.compute_cut_points(row["Amplicon_Sequence"], args.guide_seq, args.cleavage_offset)
    return quantify.run_summary(out[0], len(row["Amplicon_Sequence"]), cuts)["df_alleles"], cuts, len(kept)


def check_tables(rep, row, batch, batch_hdr, gq, offset=20):
    want, cuts, n_kept = host_alleles(row, batch, batch_hdr, gq)
    assert_frame_equal(rep.alleles, want)
    assert int(rep.alleles["#Reads"].sum()) == rep.n_total == n_kept
    pairs = report.guide_cut_pairs(row["sgRNA"] or None, cuts)
    assert [(sg, c) for sg, c, _ in rep.around_cut] == pairs
    for sg, c, frame in rep.around_cut:
        assert_form(frame)
        assert_frame_equal(frame, alleles.around_cut_from_alleles(rep.alleles, c, offset))
        assert int(frame["#Reads"].sum()) == rep.n_total
    return len(pairs)


def same_reports(a, b):
    """Every field of two GroupReports but the two tables."""
    assert a.slots.tolist() == b.slots.tolist() and (a.name, a.amplicon, a.n_reads) == (b.name, b.amplicon, b.n_reads)
    assert list(a.cut_points) == list(b.cut_points) and (a.has_coding_seq, a.has_expected_hdr) == (b.has_coding_seq, b.has_expected_hdr)
    for f in ("hist_ins", "hist_del", "hist_mut", "hist_indel"):
        assert np.array_equal(getattr(a, f), getattr(b, f))
    for name in quantify.VECTOR_NAMES:
        assert np.array_equal(a.totals["vectors"][name], b.totals["vectors"][name])
    assert a.totals["counters"] == b.totals["counters"]
    assert a.totals["hist_inframe"] == b.totals["hist_inframe"] and a.totals["hist_frameshift"] == b.totals["hist_frameshift"]


def test_pooled_alleles_equal_the_host_path_on_the_kept_rows(d, gq, gpu_aligner_factory, monkeypatch):
    rows, amps, reads = panel_rows()
    al = gpu_aligner_factory()
    res = demux.demultiplex(amps, pack(reads), demultiplexer=d)
    counts = res.counts.tolist()
    keep = [g for g in range(8) if g != 6]
    groups = res.reads_per_amplicon()
    batches = dict(zip(keep, align_pooled([amps[g] for g in keep], [groups[g] for g in keep], al)))
    got, plain = {}, {}
    kw = dict(min_reads=counts[6], min_identity_score=SCORE, demultiplexer=d, **OPTS)
    ps = demux.summarize_pooled(rows, pack(reads), al, reports=lambda g, rep: got.__setitem__(g, rep), alleles=True, **kw)
    ps0 = demux.summarize_pooled(rows, pack(reads), al, reports=lambda g, rep: plain.__setitem__(g, rep), **kw)
    assert np.array_equal(ps.counts, ps0.counts) and ps.skipped == ps0.skipped == [6] and al.output_mode == "rows"
    assert set(ps.kernel_ms) == set(ps0.kernel_ms) | {"alleles", "around_cut", "alleles_wall", "around_cut_wall"}
    assert ps.kernel_ms["alleles"] > 0 and ps.kernel_ms["around_cut"] > 0
    assert sorted(got) == sorted(plain) == keep
    n_around = 0
    for g in keep:
        same_reports(got[g], plain[g])
        assert plain[g].alleles is None and plain[g].around_cut is None
        n_around += check_tables(got[g], rows[g], batches[g], None, gq)
    assert n_around > 0
    # amplicon 0: the ten reads the filter drops are in no allele
    assert counts[0] == 50 and int(got[0].alleles["#Reads"].sum()) == 40
    assert len(got[0].alleles) > 1 and int(got[0].alleles["#Reads"][got[0].alleles["UNMODIFIED"]].sum()) == 19
    # offset 65 is beyond the device path: the tables come from the resident allele table, in the same form
    def refuse(*a, **k):
        raise AssertionError("the device path was taken")

    monkeypatch.setattr(alleles.GpuAlleleGrouper, "windows_resident", refuse)
    wide = {}
    pw = demux.summarize_pooled(rows, pack(reads), al, reports=lambda g, rep: wide.__setitem__(g, rep), alleles=True,
                                offset_around_cut=65, **kw)
    monkeypatch.undo()
    assert pw.kernel_ms["around_cut"] == 0 and pw.kernel_ms["around_cut_wall"] > 0 and pw.kernel_ms["alleles"] > 0
    assert sum(check_tables(wide[g], rows[g], batches[g], None, gq, offset=65) for g in keep) == n_around
    g2 = next(g for g in keep if wide[g].around_cut)
    assert max(len(s) for s in wide[g2].around_cut[0][2].index) > 40


def test_pooled_alleles_with_expected_hdr(d, gq, gpu_aligner_factory):
    rows, reads, origin = hm.panel()
    amps = [r["Amplicon_Sequence"] for r in rows]
    al = gpu_aligner_factory()
    res = demux.demultiplex(amps, pack(reads), demultiplexer=d)
    assert res.which.tolist() == origin
    groups = res.reads_per_amplicon()
    batches = align_pooled(amps, groups, al)
    hdr_batches = dict(zip(range(3), align_pooled([rows[g]["Expected_HDR"] for g in range(3)], groups[:3], al)))
    got, plain = {}, {}
    kw = dict(min_reads=5, min_identity_score=SCORE, demultiplexer=d, allow_hdr=True, **OPTS)
    ps = demux.summarize_pooled(rows, pack(reads), al, reports=lambda g, rep: got.__setitem__(g, rep), alleles=True, **kw)
    ps0 = demux.summarize_pooled(rows, pack(reads), al, reports=lambda g, rep: plain.__setitem__(g, rep), **kw)
    assert np.array_equal(ps.counts, ps0.counts) and sorted(got) == [0, 1, 2, 3]
    for g in range(4):
        same_reports(got[g], plain[g])
        n = check_tables(got[g], rows[g], batches[g], hdr_batches.get(g), gq)
        assert n == (1 if g == 2 else 0)
        assert bool(got[g].alleles["HDR"].any()) == (g < 3)
        assert int(got[g].alleles["#Reads"][got[g].alleles["HDR"]].sum()) == int(ps.counts[g, 4])


# ---- summarize_regions and the command lines ---------------------------------------------------

def read_back(folder, rep):
    """The two kinds of file of a folder read with pd.read_csv(sep="\\t") against the report's frames."""
    got = pd.read_csv(os.path.join(folder, "Alleles_frequency_table.txt"), sep="\t", float_precision="round_trip")
    assert_frame_equal(got, rep.alleles.loc[:, :"%Reads"].reset_index(drop=True))
    names = []
    for sg, c, frame in rep.around_cut:
        name = "Alleles_frequency_table_around_cut_site_for_%s.txt" % sg
        back = pd.read_csv(os.path.join(folder, name), sep="\t", float_precision="round_trip").set_index("Aligned_Sequence")
        assert_frame_equal(back, frame)
        names.append(name)
    assert sorted(f for f in os.listdir(folder) if f.startswith("Alleles_")) == sorted(["Alleles_frequency_table.txt"] + names)
    return len(names)


def test_region_alleles_and_the_command_line(gq, gpu_aligner_factory, tmp_path):
    bam_path, table, fasta = sc.write_inputs(tmp_path)
    rows = regions.wgs_rows(regions.read_wgs_region_file(table), fasta)
    amps = [r["Amplicon_Sequence"] for r in rows]
    bam = regions.read_bam(bam_path)
    targets = [(r["chr_id"], r["bpstart"], r["bpend"], r["Name"]) for r in rows]
    host = regions.extract_regions(bam, targets)
    al = gpu_aligner_factory()
    batches = align_pooled(amps[:3], [host.reads(g) for g in range(3)], al)
    got, plain = {}, {}
    with regions.extract_regions_resident(bam, targets) as res:
        rs = regions.summarize_regions(rows, res, al, min_reads=sc.MIN_READS, min_identity_score=SCORE,
                                       reports=lambda g, rep: got.__setitem__(g, rep), alleles=True, **OPTS)
        rs0 = regions.summarize_regions(rows, res, al, min_reads=sc.MIN_READS, min_identity_score=SCORE,
                                        reports=lambda g, rep: plain.__setitem__(g, rep), **OPTS)
    assert np.array_equal(rs.counts, rs0.counts) and sorted(got) == [0, 1, 2]
    assert "alleles" not in rs0.kernel_ms and rs.kernel_ms["alleles"] > 0
    n_around = 0
    for g in range(3):
        same_reports(got[g], plain[g])
        n_around += check_tables(got[g], rows[g], batches[g], None, gq)
        assert rs.counts[g, 0] > rs.counts[g, 1] == int(got[g].alleles["#Reads"].sum())
    assert n_around > 0
    out = str(tmp_path / "cli")
    assert regions.main(["--bam", bam_path, "--regions", table, "--genome", fasta, "--summary", "--reports", "--alleles",
                         "--out", out]) == 0
    assert sum(read_back(os.path.join(out, "CRISPResso_on_region_%d" % g), got[g]) for g in range(3)) == n_around
    with pytest.raises(SystemExit) as exc:
        regions.main(["--bam", bam_path, "--regions", table, "--genome", fasta, "--summary", "--alleles", "--out",
                      str(tmp_path / "no")])
    assert exc.value.code == 2 and not os.path.exists(tmp_path / "no")


def test_pooled_command_line_writes_the_tables(d, gpu_aligner_factory, tmp_path, capsys):
    rows, amps, reads = panel_rows()
    table = tmp_path / "amplicons.txt"
    table.write_text("".join("%s\t%s\t%s\t\t%s\n" % (r["Name"], r["Amplicon_Sequence"], r["sgRNA"], r["Coding_sequence"])
                             for r in rows))
    fq = str(tmp_path / "reads.fq")
    write_fastq(fq, [b"read%d" % j for j in range(len(reads))], reads)
    n6 = sum(1 for j in range(400) if j % 8 == 6 and j <= 200)
    got = {}
    demux.summarize_pooled(rows, pack(reads), gpu_aligner_factory(), min_reads=n6, demultiplexer=d,
                           reports=lambda g, rep: got.__setitem__(g, rep), alleles=True, offset_around_cut=12)
    out = str(tmp_path / "out")
    assert demux.main(["-f", str(table), "-r1", fq, "-o", out, "--summary", "--reports", "--alleles",
                       "--offset_around_cut_to_plot", "12", "--min_reads_to_use_region", str(n6)]) == 0
    assert "7 result folders" in capsys.readouterr().out
    n_around = 0
    for g in sorted(got):
        folder = os.path.join(out, "CRISPResso_on_" + demux.clean_filename(rows[g]["Name"]))
        n_around += read_back(folder, got[g])
        for sg, c, frame in got[g].around_cut:
            assert max(len(s) for s in frame.index) == 24
    assert sorted(got) == [g for g in range(8) if g != 6] and n_around > 0
    with pytest.raises(SystemExit) as exc:
        demux.main(["-f", str(table), "-r1", fq, "-o", str(tmp_path / "no"), "--summary", "--alleles"])
    assert exc.value.code == 2 and "--reports" in capsys.readouterr().err and not os.path.exists(tmp_path / "no")
