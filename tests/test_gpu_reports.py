"""Per-group reports from HBM (nws_mask_pre and nws_histograms of include/crispr_summary.h, the
``reports`` keyword of demux.summarize_pooled and regions.summarize_regions, the command line's
--reports): the two kernels against numpy on hand-made records, and the reports of whole calls
against the host path they replace -- the rows of every group on the host, the reference's filter
on the printed identity, oracle.quant_oracle.process_rows and quantify.run_summary on the kept
rows.  Everything exact."""
import ctypes
import os
import types

import numpy as np
import pandas as pd
import pytest
from pandas.testing import assert_frame_equal

from crispresso_amd import _lib, demux, quantify, regions, report
from crispresso_amd.aligner import printed_percent
from crispresso_amd.devmem import DeviceBuffer
from crispresso_amd.pooled import align_pooled
from oracle import quant_oracle as qo
from tests import hdr_summary_model as hm
from tests import regions_summary_cases as sc
from tests import report_model as rm
from tests.alleles_cases import pack
from tests.test_gpu_summary import OPTS, SCORE, panel_rows, write_fastq

pytestmark = pytest.mark.gpu
THRESHOLD = 98.0
LOW = 128           # the sizes below it are counted in LDS, the others straight in HBM
TABLES = ("df_indels", "df_insertion", "df_deletion", "df_substitution")


@pytest.fixture(scope="module")
def d():
    with demux.GpuDemultiplexer(0) as x:
        yield x


@pytest.fixture(scope="module")
def s():
    with demux.GpuSummarizer(0) as x:
        yield x


# ---- nws_mask_pre ------------------------------------------------------------------------------

def pre_and_keep(n):
    """Every pre value 0 .. 7 with every keep in 0, 1, 2, in turn."""
    j = np.arange(n)
    return (j % 8).astype(np.uint8), ((j // 8) % 3).astype(np.uint8)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_mask_pre(s, n):
    pre, keep = pre_and_keep(n)
    want = rm.mask_pre(pre, keep)
    assert np.array_equal(want, np.where(keep > 0, pre, _lib.NWQ_PRE_UNMODIFIED))
    got, aliased = np.full(n, 0xAA, np.uint8), np.full(n, 0xAA, np.uint8)
    ms = ctypes.c_float(-1.0)
    with DeviceBuffer.from_array(pre) as d_pre, DeviceBuffer.from_array(keep) as d_keep, DeviceBuffer(n) as d_q:
        assert s._lib.nws_mask_pre(s._ctx, d_pre.ptr, d_keep.ptr, n, d_q.ptr, ctypes.byref(ms)) == 0
        assert s._lib.nws_mask_pre(s._ctx, d_pre.ptr, d_keep.ptr, n, d_q.ptr, None) == 0
        if n:
            d_q.download(got)
            before = np.zeros(n, np.uint8)
            d_pre.download(before)
            assert np.array_equal(before, pre)              # the input is left alone
        s.mask_pre(d_pre.ptr, d_keep.ptr, n, d_pre.ptr)    # the aliased call
        if n:
            d_pre.download(aliased)
    if n:
        assert np.array_equal(got, want) and np.array_equal(aliased, want) and ms.value > 0
    else:
        assert ms.value == 0.0
    if n >= 257:
        assert {(int(p), int(k)) for p, k in zip(pre, keep)} == {(p, k) for p in range(8) for k in range(3)}
        # a dropped read loses its HDR and MIXED bits; a kept one keeps every bit
        assert set(want[keep == 0].tolist()) == {_lib.NWQ_PRE_UNMODIFIED} and set(want[keep > 0].tolist()) == set(range(8))


def test_mask_pre_refusals(s):
    with DeviceBuffer(8) as buf:
        assert s._lib.nws_mask_pre(s._ctx, None, buf.ptr, 4, buf.ptr, None) == _lib.NW_E_INVALID
        assert s._lib.nws_mask_pre(s._ctx, buf.ptr, buf.ptr, -1, buf.ptr, None) == _lib.NW_E_INVALID
        assert s._lib.nws_mask_pre(s._ctx, None, None, 0, None, None) == 0


# ---- nws_histograms ----------------------------------------------------------------------------

def size_records(n, bins, seed=2):
    """nwq_read records whose sizes hit 0, the last low bin, the first value beyond it and
    bins - 1 (each clipped to bins - 1), in every pairing of n_inserted and n_deleted; classes -1
    to 3 and keep 0, 1, 2 in turn."""
    rng = np.random.Generator(np.random.PCG64(seed))
    marks = np.minimum(np.array([0, 1, LOW - 1, LOW, LOW + 1, bins - 1, 0, 5]), bins - 1)
    j = np.arange(n)
    rr = np.zeros(n, _lib.NWQ_READ_DTYPE)
    rr["cls"] = j % 5 - 1
    rr["n_inserted"] = marks[j % 8]
    rr["n_deleted"] = marks[(j // 8) % 8]
    rr["n_mutated"] = marks[(j // 64) % 8]
    some = rng.random(n) < 0.3
    for f in ("n_inserted", "n_deleted", "n_mutated"):
        rr[f][some] = rng.integers(0, bins, int(some.sum()))
    keep = ((j // 3) % 3).astype(np.uint8)
    return rr, keep


def run_histograms(s, rr, keep, bins, fill=0x55):
    n = len(rr)
    out = np.full(max(5 * bins - 1, 1), fill, np.int64)
    bad, ms = ctypes.c_int64(-1), ctypes.c_float(-1.0)
    with DeviceBuffer.from_array(rr) as d_rr, DeviceBuffer.from_array(keep) as d_keep:
        rc = s._lib.nws_histograms(s._ctx, d_rr.ptr, d_keep.ptr, n, bins, _lib.ptr(out), ctypes.byref(bad),
                                   ctypes.byref(ms))
    return rc, out, int(bad.value), float(ms.value)


def model_histograms(rr, keep, bins):
    (hi, hd, hm_, hx), bad = rm.histograms(rr["cls"], rr["n_mutated"], rr["n_inserted"], rr["n_deleted"], keep, bins)
    return np.concatenate([hi, hd, hm_, hx]), bad


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 2048 * 256 + 77])
def test_histograms(s, n):
    bins = 300
    rr, keep = size_records(n, bins)
    want, bad = model_histograms(rr, keep, bins)
    assert bad == 0
    rc, got, got_bad, ms = run_histograms(s, rr, keep, bins)
    rc2, again, _, _ = run_histograms(s, rr, keep, bins, fill=-1)
    assert rc == 0 and rc2 == 0 and got_bad == 0
    assert got.tolist() == want.tolist() and again.tolist() == want.tolist()
    counted = (keep != 0) & (rr["cls"] >= 0)
    assert got[:bins].sum() == got[bins:2 * bins].sum() == got[2 * bins:3 * bins].sum() == got[3 * bins:].sum() == counted.sum()
    if n == 0:
        assert ms == 0.0 and not got.any()
    if n >= 257:
        ins = got[:bins]
        assert ins[0] > 0 and ins[LOW - 1] > 0 and ins[LOW] > 0 and ins[bins - 1] > 0
        indel = got[3 * bins:]
        assert indel[0] > 0 and indel[-1] > 0 and indel[bins - 1] > 0          # -(bins - 1), bins - 1 and 0
        assert indel[bins - 1 - LOW] > 0 and indel[bins - 1 + LOW] > 0           # the first beyond the low bins, both sides
        assert (~counted).sum() > n // 3                                         # the skipped reads were there
    # through the binding
    with DeviceBuffer.from_array(rr) as d_rr, DeviceBuffer.from_array(keep) as d_keep:
        parts = s.histograms(d_rr.ptr, d_keep.ptr, n, bins)
    assert [len(p) for p in parts] == [bins, bins, bins, 2 * bins - 1] and np.concatenate(parts).tolist() == want.tolist()


def test_histograms_all_reads_in_one_bin(s):
    for sizes in ((3, 1, 2), (LOW + 7, 0, LOW), (0, 0, 0)):
        n = 100000
        rr = np.zeros(n, _lib.NWQ_READ_DTYPE)
        rr["cls"], rr["n_inserted"], rr["n_deleted"], rr["n_mutated"] = 1, sizes[0], sizes[1], sizes[2]
        keep = np.ones(n, np.uint8)
        rc, got, bad, _ = run_histograms(s, rr, keep, 200)
        want, _ = model_histograms(rr, keep, 200)
        assert rc == 0 and bad == 0 and got.tolist() == want.tolist()
        assert got[sizes[0]] == n and got[200 + sizes[1]] == n and got[400 + sizes[2]] == n
        assert got[600 + sizes[0] - sizes[1] + 199] == n and got.sum() == 4 * n


def test_histograms_out_of_range(s):
    bins = 200
    rr, keep = size_records(1000, bins)
    rr["cls"][[10, 11, 12, 13, 14]] = 1
    keep[[10, 11, 12, 13, 14]] = 1
    rr["n_inserted"][10] = bins          # one past the last bin
    rr["n_deleted"][11] = -1
    rr["n_mutated"][12] = bins + 5
    rr["n_inserted"][13] = -(2 ** 31)
    rr["n_deleted"][14] = 2 ** 31 - 1
    keep[15], rr["n_inserted"][15] = 0, bins       # not counted: not out of range either
    rr["cls"][16], rr["n_deleted"][16] = -1, -7
    want, bad = model_histograms(rr, keep, bins)
    assert bad == 5
    rc, got, got_bad, _ = run_histograms(s, rr, keep, bins)
    assert rc == _lib.NW_E_INVALID and got_bad == 5 and got.tolist() == want.tolist()
    assert b"outside" in s._lib.nws_last_error(s._ctx)
    with pytest.raises(demux.SummaryError) as exc, DeviceBuffer.from_array(rr) as d_rr, \
            DeviceBuffer.from_array(keep) as d_keep:
        s.histograms(d_rr.ptr, d_keep.ptr, len(rr), bins)
    assert exc.value.code == _lib.NW_E_INVALID and exc.value.n_out_of_range == 5
    # the context still works
    rr, keep = size_records(64, bins)
    assert run_histograms(s, rr, keep, bins)[0] == 0


def test_histograms_bins_limits(s):
    rr, keep = size_records(500, 1)
    assert not rr["n_inserted"].any() and not rr["n_mutated"].any()
    rc, got, bad, _ = run_histograms(s, rr, keep, 1)
    want, _ = model_histograms(rr, keep, 1)
    assert rc == 0 and bad == 0 and got.tolist() == want.tolist() and len(want) == 4 and want[0] > 0
    top = _lib.NWS_MAX_BINS
    rr, keep = size_records(5000, top)
    want, _ = model_histograms(rr, keep, top)
    rc, got, bad, _ = run_histograms(s, rr, keep, top)
    assert rc == 0 and bad == 0 and np.array_equal(got, want) and got[top - 1] > 0 and got[3 * top] > 0 and got[-1] > 0
    for bins in (0, top + 1, -3):
        out = np.zeros(8, np.int64)
        with DeviceBuffer(64) as buf:
            assert s._lib.nws_histograms(s._ctx, buf.ptr, buf.ptr, 1, bins, _lib.ptr(out), None, None) == _lib.NW_E_UNSUPPORTED
    with DeviceBuffer(64) as buf:
        out = np.zeros(9, np.int64)
        assert s._lib.nws_histograms(s._ctx, buf.ptr + 8, buf.ptr, 1, 2, _lib.ptr(out), None, None) == _lib.NW_E_INVALID
        assert s._lib.nws_histograms(s._ctx, buf.ptr, buf.ptr, 1, 2, None, None, None) == _lib.NW_E_INVALID


# ---- the host path the reports replace ---------------------------------------------------------

def quant_args(row, hdr):
    return types.SimpleNamespace(
        amplicon_seq=row["Amplicon_Sequence"], guide_seq=row["sgRNA"] or None, coding_seq=row["Coding_sequence"] or None,
        ignore_substitutions=False, ignore_insertions=False, ignore_deletions=False,
        hide_mutations_outside_window_NHEJ=False, expected_hdr_amplicon_seq=hdr or None,
        hdr_perfect_alignment_threshold=THRESHOLD, **OPTS)


def host_frames(batch, batch_hdr, score_min=SCORE):
    """(the DataFrame the reference would quantify, the same without its filter): the rows on the
    host, both printed identities, kept iff either is > score_min (CORE:1849-1856)."""
    recs, kept = [], []
    for i in range(len(batch)):
        if batch.empty(i):
            continue
        sr = printed_percent(int(batch.stats["n_ident"][i]), int(batch.stats["aln_len"][i]))
        sp = float("nan") if batch_hdr is None else \
            printed_percent(int(batch_hdr.stats["n_ident"][i]), int(batch_hdr.stats["aln_len"][i]))
        recs.append((batch.ref_seq(i), batch.align_str(i), batch.align_seq(i), sr, sp, sr - sp))
        kept.append(sr > score_min or sp > score_min)
    df = pd.DataFrame(recs, columns=["ref_seq", "align_str", "align_seq", "score_ref", "score_repaired", "score_diff"])
    return df[np.array(kept, bool)].reset_index(drop=True), df


def oracle_totals(df, row, hdr):
    """oracle.quant_oracle.process_rows over the rows of df."""
    amp = row["Amplicon_Sequence"]
    cuts = qo.cut_points(amp, row["sgRNA"] or None, OPTS["cleavage_offset"])
    exon, spl = qo.exon_splicing_positions(amp, row["Coding_sequence"] or None)
    prm = qo.QuantParams(len(amp), qo.include_idxs(len(amp), cuts, OPTS["window_around_sgrna"],
                                                   OPTS["exclude_bp_from_left"], OPTS["exclude_bp_from_right"]),
                         exon, spl, window_around_sgrna=OPTS["window_around_sgrna"], expected_hdr=bool(hdr),
                         hdr_perfect_alignment_threshold=THRESHOLD)
    return qo.process_rows(df["ref_seq"].tolist(), df["align_str"].tolist(), df["align_seq"].tolist(),
                           (df["score_ref"] == 100).to_numpy(), df["score_diff"].to_numpy() if hdr else None,
                           df["score_repaired"].to_numpy() if hdr else None, prm)


def same_totals(totals, ref):
    """The report's 15 vectors, 4 counters and 2 frameshift histograms against the oracle's."""
    for name in quantify.VECTOR_NAMES:
        if not np.array_equal(totals["vectors"][name], ref["vectors"][name]):
            return name
    for name in quantify.COUNTER_NAMES:
        if totals["counters"][name] != ref["counters"][name]:
            return name
    if totals["hist_inframe"] != ref["hist_inframe"] or totals["hist_frameshift"] != ref["hist_frameshift"]:
        return "frameshift histograms"
    return None


def check_report(rep, row, n_reads, batch, batch_hdr, slots, gq, score_min=SCORE):
    """One GroupReport against the host path on the kept rows; returns (kept, all) oracle totals."""
    hdr = row.get("Expected_HDR") if batch_hdr is not None else None
    kept, everything = host_frames(batch, batch_hdr, score_min)
    ref = oracle_totals(kept, row, hdr)
    assert same_totals(rep.totals, ref) is None, (row["Name"], same_totals(rep.totals, ref))
    args = quant_args(row, hdr)
    out = quantify.quantify_alignments(kept.copy(), args, quantifier=gq, globals_=quantify.globals_from_args(args))
    cuts = quantify.compute_cut_points(row["Amplicon_Sequence"], args.guide_seq, args.cleavage_offset)
    summary = quantify.run_summary(out[0], len(row["Amplicon_Sequence"]), cuts)
    got = report.tables(rep)
    for key in TABLES:
        assert_frame_equal(got[key], summary[key])
    # the histograms themselves against the oracle's per-read sizes
    bins = len(rep.hist_ins)
    (hi, hd, hm_, hx), bad = rm.histograms(ref["cls"], ref["n_mutated"], ref["n_inserted"], ref["n_deleted"],
                                           np.ones(len(kept), np.uint8), bins)
    assert bad == 0 and np.array_equal(rep.hist_ins, hi) and np.array_equal(rep.hist_del, hd)
    assert np.array_equal(rep.hist_mut, hm_) and np.array_equal(rep.hist_indel, hx)
    assert rep.slots.tolist() == list(slots) and rep.n_total == len(kept) == summary["n_total"]
    assert rep.slots[2:6].tolist() == [summary[k] for k in ("n_unmodified", "n_modified", "n_repaired", "n_mixed_hdr_nhej")]
    assert rep.n_reads == n_reads and rep.name == row["Name"] and rep.amplicon == row["Amplicon_Sequence"]
    assert list(rep.cut_points) == cuts and rep.has_coding_seq == bool(row["Coding_sequence"])
    assert rep.has_expected_hdr == bool(hdr)
    return ref, oracle_totals(everything, row, hdr)


# ---- summarize_pooled(reports=...) -------------------------------------------------------------

def test_pooled_reports_equal_the_host_path_on_the_kept_rows(d, gpu_aligner_factory):
    rows, amps, reads = panel_rows()
    al = gpu_aligner_factory()
    res = demux.demultiplex(amps, pack(reads), demultiplexer=d)
    counts = res.counts.tolist()
    assert counts[6] < 50 and [counts[g] for g in range(8) if g != 6] == [50] * 7
    keep = [g for g in range(8) if g != 6]
    groups = res.reads_per_amplicon()
    batches = dict(zip(keep, align_pooled([amps[g] for g in keep], [groups[g] for g in keep], al)))
    # the masked totals differ from the unmasked ones: the cut reads the filter drops carry long deletions
    kept0, all0 = host_frames(batches[0], None)
    assert len(all0) == 50 and len(kept0) == 40
    masked, unmasked = oracle_totals(kept0, rows[0], None), oracle_totals(all0, rows[0], None)
    assert same_totals(masked, unmasked) is not None
    assert unmasked["vectors"]["effect_vector_deletion"].sum() > masked["vectors"]["effect_vector_deletion"].sum()

    got, seen = {}, []
    ps = demux.summarize_pooled(rows, pack(reads), al, min_reads=counts[6], min_identity_score=SCORE, demultiplexer=d,
                                reports=lambda g, rep: got.__setitem__(g, rep),
                                on_group=lambda g, a, n: seen.append((g, n, sorted(got))), **OPTS)
    plain = demux.summarize_pooled(rows, pack(reads), al, min_reads=counts[6], min_identity_score=SCORE, demultiplexer=d,
                                   **OPTS)
    assert np.array_equal(ps.counts, plain.counts) and ps.skipped == plain.skipped == [6] and al.output_mode == "rows"
    assert_frame_equal(ps.frame, plain.frame)
    assert set(plain.kernel_ms) == {"flags", "summary", "quantify", "printed", "hdr_pass"}
    assert set(ps.kernel_ms) == set(plain.kernel_ms) | {"mask", "histograms"}
    assert ps.kernel_ms["mask"] > 0 and ps.kernel_ms["histograms"] > 0
    assert sorted(got) == keep and [(g, n) for g, n, _ in seen] == [(g, counts[g]) for g in keep]
    assert all(g not in before for g, _, before in seen)      # a group's report follows its on_group
    with quantify.GpuQuantifier(0) as gq:
        for g in keep:
            ref, everything = check_report(got[g], rows[g], counts[g], batches[g], None, ps.counts[g].tolist(), gq)
            if g == 0:
                assert same_totals(got[g].totals, everything) is not None
    assert ps.counts[0, :3].tolist() == [50, 40, 19]
    assert got[5].has_coding_seq and sum(got[5].totals["counters"].values()) > 0 and got[2].cut_points
    assert got[0].hist_del[1:].sum() > 0 and got[0].hist_indel.sum() == 40
    # the same reports again on the same contexts
    again = {}
    demux.summarize_pooled(rows, pack(reads), al, min_reads=counts[6], min_identity_score=SCORE, demultiplexer=d,
                           reports=lambda g, rep: again.__setitem__(g, rep), **OPTS)
    for g in keep:
        assert same_totals(again[g].totals, got[g].totals) is None and np.array_equal(again[g].hist_indel, got[g].hist_indel)


def test_reports_with_a_coding_sequence_and_with_expected_hdr(d, gpu_aligner_factory, tmp_path):
    rows, reads, origin = hm.panel()
    amps = [r["Amplicon_Sequence"] for r in rows]
    rows[3] = dict(rows[3], Coding_sequence=amps[3][80:140])          # the 3-base deletion at 100 lies in it
    rows[0] = dict(rows[0], Coding_sequence=amps[0][60:120])          # and one row with both
    al = gpu_aligner_factory()
    res = demux.demultiplex(amps, pack(reads), demultiplexer=d)
    assert res.which.tolist() == origin
    groups, counts = res.reads_per_amplicon(), res.counts.tolist()
    batches = align_pooled(amps, groups, al)
    hdr_batches = dict(zip(range(3), align_pooled([rows[g]["Expected_HDR"] for g in range(3)], groups[:3], al)))
    got = {}
    ps = demux.summarize_pooled(rows, pack(reads), al, min_reads=5, min_identity_score=SCORE, demultiplexer=d,
                                allow_hdr=True, reports=lambda g, rep: got.__setitem__(g, rep), **OPTS)
    plain = demux.summarize_pooled(rows, pack(reads), al, min_reads=5, min_identity_score=SCORE, demultiplexer=d,
                                   allow_hdr=True, **OPTS)
    assert np.array_equal(ps.counts, plain.counts) and sorted(got) == [0, 1, 2, 3]
    assert (ps.counts[:3, 4] > 0).all() and (ps.counts[:3, 5] > 0).all() and (ps.counts[:3, 0] > ps.counts[:3, 1]).all()
    with quantify.GpuQuantifier(0) as gq:
        for g in range(4):
            ref, _ = check_report(got[g], rows[g], counts[g], batches[g], hdr_batches.get(g), ps.counts[g].tolist(), gq)
            v = ref["vectors"]
            if g < 3:       # a test that passes with zeros in the HDR and mixed vectors shows nothing
                assert v["effect_vector_mutation_hdr"].sum() > 0 and v["effect_vector_mutation_mixed"].sum() > 0
            else:
                assert not v["effect_vector_mutation_hdr"].any() and not v["effect_vector_insertion_mixed"].any()
            if g in (0, 3):
                assert sum(ref["counters"].values()) > 0 and ref["hist_inframe"]
            if g == 3:
                assert v["effect_vector_mutation_noncoding"].sum() > 0
    hdr_files = {"effect_vector_%s_%s.txt" % (k, tag) for k in ("insertion", "deletion", "substitution")
                 for tag in ("HDR", "mixed_hdr_nhej")}
    coding_files = {"Frameshift_analysis.txt", "Splice_sites_analysis.txt"} | {
        "effect_vector_%s_noncoding.txt" % k for k in ("insertion", "deletion", "substitution")}
    for g in range(4):
        folder = str(tmp_path / report.folder_name(rows[g]["Name"]))
        names = set(report.write_report(folder, got[g]))
        assert names == set(os.listdir(folder))
        assert (names & hdr_files) == (hdr_files if g < 3 else set())
        assert (names & coding_files) == (coding_files if g in (0, 3) else set())
        assert rm.read_quantification(os.path.join(folder, "Quantification_of_editing_frequency.txt")) == \
            ps.counts[g, 1:6].tolist()
        frames = report.tables(got[g])
        want = rm.expected_files(got[g], frames)
        assert set(want) == names
        for name, body in want.items():
            with open(os.path.join(folder, name), "rb") as f:
                assert f.read() == body, (g, name)


# ---- summarize_regions(reports=...) ------------------------------------------------------------

def test_region_reports_equal_the_host_path_on_the_kept_rows(gpu_aligner_factory, tmp_path):
    bam_path, table, fasta = sc.write_inputs(tmp_path)
    rows = regions.wgs_rows(regions.read_wgs_region_file(table), fasta)
    amps = [r["Amplicon_Sequence"] for r in rows]
    bam = regions.read_bam(bam_path)
    targets = [(r["chr_id"], r["bpstart"], r["bpend"], r["Name"]) for r in rows]
    plain = regions.extract_regions(bam, targets)
    al = gpu_aligner_factory()
    batches = align_pooled(amps[:3], [plain.reads(g) for g in range(3)], al)
    got = {}
    with regions.extract_regions_resident(bam, targets) as res:
        rs = regions.summarize_regions(rows, res, al, min_reads=sc.MIN_READS, min_identity_score=SCORE,
                                       reports=lambda g, rep: got.__setitem__(g, rep), **OPTS)
        without = regions.summarize_regions(rows, res, al, min_reads=sc.MIN_READS, min_identity_score=SCORE, **OPTS)
    assert np.array_equal(rs.counts, without.counts) and rs.skipped == without.skipped == [3] and sorted(got) == [0, 1, 2]
    assert_frame_equal(rs.frame, without.frame)
    assert "mask" not in without.kernel_ms and rs.kernel_ms["histograms"] > 0
    with quantify.GpuQuantifier(0) as gq:
        for g in range(3):
            ref, everything = check_report(got[g], rows[g], sc.N_RECORDS[g], batches[g], None, rs.counts[g].tolist(), gq)
            assert rs.counts[g, 0] > rs.counts[g, 1]            # the junk the filter drops
    assert got[0].cut_points and got[2].has_coding_seq and got[1].hist_ins[2] > 0 and got[1].hist_del[3:7].sum() > 0
    # the command line: the same table, and a folder per analysed region
    out = str(tmp_path / "cli")
    assert regions.main(["--bam", bam_path, "--regions", table, "--genome", fasta, "--summary", "--reports",
                         "--out", out]) == 0
    want = str(tmp_path / "want.txt")
    demux.write_summary(want, rs.frame)
    with open(os.path.join(out, "SAMPLES_QUANTIFICATION_SUMMARY.txt"), "rb") as f, open(want, "rb") as w:
        assert f.read() == w.read()
    assert sorted(os.listdir(out)) == ["CRISPResso_on_region_%d" % g for g in range(3)] + ["SAMPLES_QUANTIFICATION_SUMMARY.txt"]
    for g in range(3):
        folder = os.path.join(out, "CRISPResso_on_region_%d" % g)
        files = rm.expected_files(got[g], report.tables(got[g]))
        assert sorted(os.listdir(folder)) == sorted(files)
        for name, body in files.items():
            with open(os.path.join(folder, name), "rb") as f:
                assert f.read() == body, (g, name)
    with pytest.raises(SystemExit) as exc:
        regions.main(["--bam", bam_path, "--regions", table, "--out", str(tmp_path / "no"), "--reports"])
    assert exc.value.code == 2 and not os.path.exists(tmp_path / "no")


# ---- the command line --------------------------------------------------------------------------

def test_command_line_writes_a_folder_per_summarized_amplicon(tmp_path, capsys):
    rows, amps, reads = panel_rows()
    rows[4]["Name"] = "AMP 4/x"            # a name the folder's name is cleaned of
    table = tmp_path / "amplicons.txt"
    table.write_text("".join("%s\t%s\t%s\t\t%s\n" % (r["Name"], r["Amplicon_Sequence"], r["sgRNA"], r["Coding_sequence"])
                             for r in rows))
    fq = str(tmp_path / "reads.fq")
    write_fastq(fq, [b"read%d" % j for j in range(len(reads))], reads)
    out = str(tmp_path / "out")
    n6 = sum(1 for j in range(400) if j % 8 == 6 and j <= 200)
    assert demux.main(["-f", str(table), "-r1", fq, "-o", out, "--summary", "--reports", "--min_reads_to_use_region",
                       str(n6)]) == 0
    printed = capsys.readouterr().out
    assert "7 result folders" in printed
    names = [r["Name"].replace(" ", "_") for r in rows]            # (read_amplicons_file's rule for blanks)
    folders = sorted(f for f in os.listdir(out) if f.startswith("CRISPResso_on_"))
    assert folders == sorted("CRISPResso_on_" + demux.clean_filename(nm) for g, nm in enumerate(names) if g != 6)
    assert "CRISPResso_on_AMP_4x" in folders and "CRISPResso_on_AMP_6" not in folders
    summary = pd.read_csv(os.path.join(out, "SAMPLES_QUANTIFICATION_SUMMARY.txt"), sep="\t")
    assert summary["Name"].tolist() == names and np.isnan(summary["Reads_aligned"][6])
    for g, nm in enumerate(names):
        if g == 6:
            continue
        folder = os.path.join(out, "CRISPResso_on_" + demux.clean_filename(nm))
        total, unmod, nhej, hdr, mixed = rm.read_quantification(os.path.join(folder, "Quantification_of_editing_frequency.txt"))
        line = summary.iloc[g]
        assert line["Reads_aligned"] == float(total) and line["Reads_total"] == 50
        assert line[["Unmodified%", "NHEJ%", "HDR%", "Mixed_HDR-NHEJ%"]].tolist() == \
            [float(x) / float(total) * 100. for x in (unmod, nhej, hdr, mixed)]
        combined = np.loadtxt(os.path.join(folder, "effect_vector_combined.txt"), skiprows=1)
        assert combined.shape == (len(amps[g]), 2)
        with open(os.path.join(folder, "Mapping_statistics.txt")) as f:
            assert f.read() == "READS IN INPUTS:50\nREADS AFTER PREPROCESSING:50\nREADS ALIGNED:%d" % total
        assert os.path.exists(os.path.join(folder, "Frameshift_analysis.txt")) == (g == 5)
        assert not os.path.exists(os.path.join(folder, "effect_vector_insertion_HDR.txt"))
    assert rm.read_quantification(os.path.join(out, "CRISPResso_on_AMP_0", "Quantification_of_editing_frequency.txt"))[:2] \
        == [40, 19]
    # --reports alone is a usage error
    with pytest.raises(SystemExit) as exc:
        demux.main(["-f", str(table), "-r1", fq, "-o", str(tmp_path / "no"), "--reports"])
    assert exc.value.code == 2 and "--summary" in capsys.readouterr().err and not os.path.exists(tmp_path / "no")


def test_a_group_without_a_kept_read_gets_no_folder(d, tmp_path, gpu_aligner_factory):
    """With the score at 100 no read is kept (the filter is strict): zero slots, a report whose
    writing is refused, no folder and the group noted."""
    rows, amps, reads = panel_rows()
    rows, amps = rows[:2], amps[:2]
    sel = [r for j, r in enumerate(reads[:160]) if j % 8 < 2]
    al = gpu_aligner_factory()
    folders, refused = {}, []
    ps = demux.summarize_pooled(rows, pack(sel), al, min_reads=5, min_identity_score=100.0, demultiplexer=d,
                                reports=demux._folder_writer(str(tmp_path), folders, refused), **OPTS)
    assert ps.counts[:, 0].tolist() == [20, 20] and not ps.counts[:, 1:].any()
    assert refused == [0, 1] and folders == {} and os.listdir(tmp_path) == []
