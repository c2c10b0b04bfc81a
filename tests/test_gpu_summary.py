"""Raw reads to the per-amplicon summary in HBM (include/crispr_summary.h, nwd_assign_prepared,
crispresso_amd.demux.summarize_pooled): the two kernels against tests/pooled_summary_model.py on
hand-made records, the demultiplexer on the front end's resident reads against the same call on
their host copy, and the whole call against the host path (download, printed identity, filter,
quantify_alignments, run_summary) and against the CPU oracles.  Everything exact."""
import ctypes
import gzip
import json
import os
import subprocess
import sys
import types

import numpy as np
import pandas as pd
import pytest

from crispresso_amd import _lib, demux, frontend, quantify, synth
from crispresso_amd.aligner import printed_percent
from crispresso_amd.devmem import DeviceBuffer
from oracle import quant_oracle as qo
from tests import demux_cases as dc
from tests import demux_model as dm
from tests import pooled_summary_cases as cases
from tests import pooled_summary_model as psm
from tests.alleles_cases import pack
from tests.helpers import oracle_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_COLS = 2000
SCORE = 60.0


@pytest.fixture(scope="module")
def d():
    with demux.GpuDemultiplexer(0) as x:
        yield x


@pytest.fixture(scope="module")
def tables():
    return demux.identity_thresholds(SCORE, MAX_COLS)


@pytest.fixture(scope="module")
def summarizer(tables):
    with demux.GpuSummarizer(0) as s:
        s.set_identity(*tables)
        yield s


# ---- nws_flags ---------------------------------------------------------------------------------

SPECIAL = [(6, 10, 0), (7, 10, 0), (150, 250, 0), (151, 250, 0), (1999, 2000, 0), (1998, 2000, 0), (0, 0, 1),
           (250, 250, 1), (1200, MAX_COLS, 0), (1201, MAX_COLS, 0), (MAX_COLS, MAX_COLS, 0), (0, 1, 0), (1, 1, 0),
           (0, 0, 0)]           # (n_ident, aln_len, flags)


def stat_records(n, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    st = np.zeros(n, _lib.STAT_DTYPE)
    st["aln_len"] = rng.integers(1, MAX_COLS + 1, n)
    st["n_ident"] = (st["aln_len"] * rng.uniform(0.5, 1.0, n)).astype(np.int32)
    exact = rng.random(n) < 0.2
    st["n_ident"][exact] = st["aln_len"][exact]
    st["flags"] = (rng.random(n) < 0.05).astype(np.int32)
    for f in ("n_sim", "n_gaps", "score", "end_i", "end_j"):
        st[f] = rng.integers(-5, 5000, n)
    for j, (i, L, f) in enumerate(SPECIAL[:n]):
        st["n_ident"][j], st["aln_len"][j], st["flags"][j] = i, L, f
    return st


def run_flags(summarizer, st):
    n = len(st)
    pre, keep = np.full(n, 0xAA, np.uint8), np.full(n, 0xAA, np.uint8)
    bad, ms = ctypes.c_int64(-1), ctypes.c_float(-1.0)
    with DeviceBuffer.from_array(st) as d_st, DeviceBuffer(n) as d_pre, DeviceBuffer(n) as d_keep:
        rc = summarizer._lib.nws_flags(summarizer._ctx, d_st.ptr, n, d_pre.ptr, d_keep.ptr, ctypes.byref(bad),
                                       ctypes.byref(ms))
        if n:
            d_pre.download(pre)
            d_keep.download(keep)
    return rc, pre, keep, int(bad.value), float(ms.value)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_flags(summarizer, tables, n):
    st = stat_records(n)
    rc, pre, keep, bad, ms = run_flags(summarizer, st)
    assert rc == 0 and bad == 0
    want_pre, want_keep, _ = psm.flags(st["aln_len"], st["n_ident"], st["flags"], *tables)
    assert np.array_equal(pre, want_pre) and np.array_equal(keep, want_keep)
    # and numpy on the tables
    L = st["aln_len"]
    assert np.array_equal(keep.astype(bool), ((st["flags"] & 1) == 0) & (st["n_ident"] >= tables[0][L]))
    assert np.array_equal(pre, (st["n_ident"] >= tables[1][L]).astype(np.uint8) * _lib.NWQ_PRE_UNMODIFIED)
    if n == 0:
        assert ms == 0.0
    if n >= len(SPECIAL):
        # 6/10 and 150/250 print 60.0 and are dropped; 1999/2000 prints 100.0; an EMPTY record is never kept
        assert keep[:8].tolist() == [0, 1, 0, 1, 1, 1, 0, 0] and pre[:8].tolist() == [0, 0, 0, 0, 1, 0, 0, 1]
        assert keep[8] == 0 and keep[10] == 1 and pre[10] == 1          # aln_len == max_cols is inside the tables


def test_flags_outside_the_tables(summarizer, tables):
    st = stat_records(65)
    st["aln_len"][64] = MAX_COLS + 1
    st["n_ident"][64] = MAX_COLS + 1
    rc, pre, keep, bad, _ = run_flags(summarizer, st)
    assert rc == _lib.NW_E_INVALID and bad == 1 and b"outside" in summarizer._lib.nws_last_error(summarizer._ctx)
    want_pre, want_keep, want_bad = psm.flags(st["aln_len"], st["n_ident"], st["flags"], *tables)
    assert want_bad == 1 and keep[64] == 0 and pre[64] == 0
    assert np.array_equal(pre, want_pre) and np.array_equal(keep, want_keep)
    with pytest.raises(demux.SummaryError) as exc, DeviceBuffer.from_array(st) as d_st, DeviceBuffer(65) as a, \
            DeviceBuffer(65) as b:
        summarizer.flags(d_st.ptr, 65, a.ptr, b.ptr)
    assert exc.value.code == _lib.NW_E_INVALID and exc.value.n_out_of_range == 1
    # the context still works
    assert run_flags(summarizer, stat_records(64))[0] == 0


def test_flags_before_the_tables():
    with demux.GpuSummarizer(0) as fresh, DeviceBuffer(64) as buf:
        rc = fresh._lib.nws_flags(fresh._ctx, buf.ptr, 2, buf.ptr, buf.ptr, None, None)
        assert rc == _lib.NW_E_STATE


# ---- nws_summary -------------------------------------------------------------------------------

def read_records(n):
    """Every class (-1 included) x every n_* > 0 pattern x pre, in turn; keep alternates in runs
    of one and of three."""
    j = np.arange(n)
    rr = np.zeros(n, _lib.NWQ_READ_DTYPE)
    rr["cls"] = j % 5 - 1
    pat = (j // 5) % 8
    rr["n_mutated"] = (pat & 1) * (1 + j % 3)
    rr["n_inserted"] = ((pat >> 1) & 1) * (1 + j % 4)
    rr["n_deleted"] = ((pat >> 2) & 1) * (1 + j % 2)
    pre = (((j // 40) % 2) * _lib.NWQ_PRE_UNMODIFIED).astype(np.uint8)
    keep = np.where(j < n // 2, j % 2, (j % 4 != 0)).astype(np.uint8)
    return rr, pre, keep


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 1000, 2048 * 256 + 77])
def test_summary(summarizer, n):
    rr, pre, keep = read_records(n)
    with DeviceBuffer.from_array(rr) as d_rr, DeviceBuffer.from_array(pre) as d_pre, \
            DeviceBuffer.from_array(keep) as d_keep:
        got = summarizer.summary(d_rr.ptr, d_pre.ptr, d_keep.ptr, n)
        again = summarizer.summary(d_rr.ptr, d_pre.ptr, d_keep.ptr, n)
    want = psm.slots(rr["cls"], rr["n_mutated"], rr["n_inserted"], rr["n_deleted"], pre, keep)
    assert got.dtype == np.int64 and got.tolist() == want and again.tolist() == want
    if n >= 1000:
        assert min(want) > 0
    if n == 0:
        assert summarizer.summary_ms == 0.0 and not got.any()


# ---- nwd_assign_prepared -----------------------------------------------------------------------

def test_assign_prepared_equals_assign_of_the_merged_text(d, gpu_aligner_factory):
    al = gpu_aligner_factory()
    for name, (amps, packed_reads) in sorted(cases.cases().items()):
        mine, theirs, fallback, m = cases.both_ways(d, al, amps, packed_reads)
        assert mine == theirs, name
        assert m > 0 and fallback == 0          # (which pairs merge is the front end's business)
    # and array by array on the panel, against the model of the same merged text
    amps, packed_reads = cases.cases()["panel_pairs"]
    al.set_reference(amps[0].decode())
    d.set_amplicons(*demux.pack_amplicons([a.decode() for a in amps]), cases.K)
    with frontend.prepare_packed_resident(al, *packed_reads) as rr:
        assert rr.stats["combined"] == len(rr) > 0 and rr.status.dtype == np.uint8 and len(rr.status) == 400
        text, off = rr.fetch_text(), rr.offsets
        assert np.array_equal(rr.lens, np.diff(off)) and len(rr.src) == len(rr)
        with pytest.raises(frontend.FrontError):
            rr.fetch_quals()
        got = d.assign_prepared(rr, **cases.KW)
    merged = [text[off[j]:off[j + 1]].tobytes() for j in range(len(off) - 1)]
    want = dm.demultiplex(amps, merged, k=cases.K, **cases.KW)
    assert got[0].tolist() == want["which"] and got[1].tolist() == want["strand"]
    assert got[2].tolist() == want["votes"] and got[3].tolist() == want["rival"] and got[4].tolist() == want["counts"]
    pk = d.pack(got[5])
    assert pk.group_offsets.tolist() == want["group_offsets"] and pk.order.tolist() == want["order"]
    goff, order, gtext, toff = d.gather(got[5], int(pk.text_offsets[-1]))
    flat = [r for grp in want["groups"] for r in grp]
    assert [gtext[toff[j]:toff[j + 1]].tobytes() for j in range(len(flat))] == flat


@pytest.mark.parametrize("env", [{"CRISPR_NWD_CHUNK": "1"}, {"CRISPR_NWD_CHUNK": "7"}, {"CRISPR_NWD_TALLY_SLOTS": "1"}],
                         ids=lambda e: "-".join(e.values()))
def test_assign_prepared_under_the_settings(d, gpu_aligner_factory, env):
    """Chunks of one and seven reads and a tally of one entry (settings read at nwd_create: a
    child process) leave every array as it is here."""
    al = gpu_aligner_factory()
    here = [cases.both_ways(d, al, *case)[0] for _, case in sorted(cases.cases().items())]
    p = subprocess.run([sys.executable, "-m", "tests.pooled_summary_cases"], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["mine"] == here and out["theirs"] == here
    if "CRISPR_NWD_TALLY_SLOTS" in env:
        assert sum(out["fallback"]) > 0


def test_assign_prepared_refusals(d, gpu_aligner_factory):
    amps, packed_reads = cases.cases()["panel_pairs"]
    al = gpu_aligner_factory()
    al.set_reference(amps[0].decode())
    rr = frontend.prepare_packed_resident(al, *packed_reads)
    rr.close()
    assert rr.closed
    d.set_amplicons(*demux.pack_amplicons([a.decode() for a in amps]), cases.K)
    with pytest.raises(demux.DemuxError, match=r"\(-1\)"):
        d.assign_prepared(rr, **cases.KW)
    with pytest.raises(frontend.FrontError):
        rr.fetch_text()
    assert d._lib.nwd_assign_prepared(d._ctx, None, 2, 1, *[None] * 9) == _lib.NW_E_INVALID
    # pairs that do not overlap: no merged read, zeros, no kernel
    lone = cases.pairs_of([dc.bases(260, 5), dc.bases(260, 6)], n1=60)
    with frontend.prepare_packed_resident(al, *lone) as none:
        assert len(none) == 0 and none.stats["not_combined"] == 2
        got = d.assign_prepared(none, **cases.KW)
    assert [len(x) for x in got[:4]] == [0] * 4 and not got[4].any() and got[5:] == (0, 0, 0, 0.0)
    with demux.GpuDemultiplexer(0) as fresh, frontend.prepare_packed_resident(al, *packed_reads) as live:
        with pytest.raises(demux.DemuxError, match=r"\(-6\)"):
            fresh.assign_prepared(live, **cases.KW)


# ---- summarize_pooled --------------------------------------------------------------------------

OPTS = dict(window_around_sgrna=1, cleavage_offset=-3, exclude_bp_from_left=15, exclude_bp_from_right=15)


def panel_rows():
    """dc.pooled_panel() with amplicon 0's first ten reads cut to 55 % and its next ten to 65 % of
    their length (in the amplicon's orientation), an N in one read, fewer reads of amplicon 6; an
    sgRNA on row 2 and a coding sequence on row 5."""
    amps, reads = dc.pooled_panel()
    for i in range(20):
        j = 8 * i
        r = dm.revcomp(reads[j]) if j % 2 else reads[j]
        r = r[:int(len(r) * (0.55 if i < 10 else 0.65))]
        reads[j] = dm.revcomp(r) if j % 2 else r
    j = 8 * 9 + 3
    reads[j] = reads[j][:70] + b"N" + reads[j][71:]
    reads = [r for j, r in enumerate(reads) if not (j % 8 == 6 and j > 200)]
    rows = [{"Name": "AMP_%d" % g, "Amplicon_Sequence": a, "sgRNA": "", "Expected_HDR": "", "Coding_sequence": ""}
            for g, a in enumerate(amps)]
    mid = len(amps[2]) // 2
    rows[2]["sgRNA"] = amps[2][mid - 10:mid + 10]
    rows[5]["Coding_sequence"] = amps[5][40:130]
    return rows, amps, reads


def quant_args(row):
    return types.SimpleNamespace(
        amplicon_seq=row["Amplicon_Sequence"], guide_seq=row["sgRNA"] or None, coding_seq=row["Coding_sequence"] or None,
        ignore_substitutions=False, ignore_insertions=False, ignore_deletions=False,
        hide_mutations_outside_window_NHEJ=False, expected_hdr_amplicon_seq=None, **OPTS)


def kept_frame(batch, score_min=SCORE):
    """The DataFrame the reference would quantify: the rows whose printed identity is > score_min."""
    recs = []
    for i in range(len(batch)):
        if batch.empty(i):
            continue
        score = printed_percent(int(batch.stats["n_ident"][i]), int(batch.stats["aln_len"][i]))
        if score > score_min:
            recs.append((batch.ref_seq(i), batch.align_str(i), batch.align_seq(i), score))
    return pd.DataFrame(recs, columns=["ref_seq", "align_str", "align_seq", "score_ref"])


def host_slots(batch, row, gq, score_min=SCORE):
    """The 16 slots by the path summarize_pooled replaces: rows on the host, the printed
    identity, the filter, quantify_alignments, run_summary."""
    df = kept_frame(batch, score_min)
    args = quant_args(row)
    g = quantify.globals_from_args(args)
    out = quantify.quantify_alignments(df, args, quantifier=gq, globals_=g)
    cuts = quantify.compute_cut_points(row["Amplicon_Sequence"], args.guide_seq, args.cleavage_offset)
    return psm.slots_of_summary(quantify.run_summary(out[0], len(row["Amplicon_Sequence"]), cuts), len(batch))


def oracle_slots(row, group_reads, score_min=SCORE):
    """The same from the CPU oracles alone: needle, the filter, quant_oracle, the model."""
    amp = row["Amplicon_Sequence"]
    buf, off = pack(group_reads)
    df = kept_frame(oracle_batch(amp, buf, off), score_min)
    cuts = qo.cut_points(amp, row["sgRNA"] or None, OPTS["cleavage_offset"])
    exon, spl = qo.exon_splicing_positions(amp, row["Coding_sequence"] or None)
    prm = qo.QuantParams(len(amp), qo.include_idxs(len(amp), cuts, OPTS["window_around_sgrna"],
                                                   OPTS["exclude_bp_from_left"], OPTS["exclude_bp_from_right"]),
                         exon, spl, window_around_sgrna=OPTS["window_around_sgrna"])
    um = (df["score_ref"] == 100).to_numpy()
    res = qo.process_rows(df["ref_seq"].tolist(), df["align_str"].tolist(), df["align_seq"].tolist(), um, None, None, prm)
    k = len(df)
    got = psm.slots(res["cls"], res["n_mutated"], res["n_inserted"], res["n_deleted"],
                    um.astype(np.uint8) * _lib.NWQ_PRE_UNMODIFIED, np.ones(k, np.uint8))
    return [len(group_reads)] + got[1:]


@pytest.fixture(scope="module")
def panel_reference(d, gpu_aligner_factory):
    """(rows, amps, reads, min_reads, {g: slots}) of the host path, computed once."""
    rows, amps, reads = panel_rows()
    want = dm.demultiplex([a.encode() for a in amps], reads)
    counts = want["counts"]
    assert counts[6] < 50 and [counts[g] for g in range(8) if g != 6] == [50] * 7
    al = gpu_aligner_factory()
    batches, res, skipped = demux.align_demultiplexed(amps, pack(reads), al, min_reads=counts[6], demultiplexer=d)
    assert skipped == [6] and not dc.mismatches(res, want)
    with quantify.GpuQuantifier(0) as gq:
        slots = {g: host_slots(batches[g], rows[g], gq) for g in range(8) if g != 6}
    return rows, amps, reads, counts, slots, want


def check_frame(ps, rows, counts, slots):
    f = ps.frame
    assert list(f.columns) == list(demux.SUMMARY_COLUMNS) and f["Name"].tolist() == [r["Name"] for r in rows]
    assert f["Reads_total"].tolist() == counts
    for g in range(8):
        if g == 6:
            assert f.iloc[g][1:6].isna().all() and not ps.counts[g].any()
            continue
        s = slots[g]
        total = float(s[1])
        assert f.iloc[g][1:6].tolist() == [s[2] / total * 100., s[3] / total * 100., s[4] / total * 100.,
                                          s[5] / total * 100., total]


def test_summarize_pooled_equals_the_host_path_and_the_oracles(d, gpu_aligner_factory, panel_reference):
    rows, amps, reads, counts, slots, want = panel_reference
    al = gpu_aligner_factory()
    seen = []
    ps = demux.summarize_pooled(rows, pack(reads), al, min_reads=counts[6], min_identity_score=SCORE, demultiplexer=d,
                                on_group=lambda g, a, n: seen.append((g, n)), **OPTS)
    assert al.output_mode == "rows" and ps.skipped == [6] and ps.counts.dtype == np.int64 and ps.counts.shape == (8, 16)
    assert seen == [(g, counts[g]) for g in range(8) if g != 6]
    assert ps.result.counts.tolist() == counts and ps.result.which.tolist() == want["which"]
    for g in range(8):
        if g != 6:
            assert ps.counts[g].tolist() == slots[g], g
            assert ps.counts[g].tolist() == oracle_slots(rows[g], want["groups"][g]), g
    # the numbers of the cut reads: ten print 54.0 .. 54.9 and are dropped, ten print 62.1 .. 64.8
    assert ps.counts[0, :3].tolist() == [50, 40, 19] and ps.counts[:, 15].tolist() == [0] * 8
    assert ps.counts[:, 3].sum() > 0 and ps.kernel_ms["summary"] > 0 and ps.kernel_ms["flags"] > 0
    check_frame(ps, rows, counts, slots)
    # a second call on the same contexts gives the same
    again = demux.summarize_pooled(rows, pack(reads), al, min_reads=counts[6], min_identity_score=SCORE,
                                   demultiplexer=d, **OPTS)
    assert np.array_equal(again.counts, ps.counts)
    pd.testing.assert_frame_equal(again.frame, ps.frame)
    # another filter moves the cut reads
    low = demux.summarize_pooled(rows, pack(reads), al, min_reads=counts[6], min_identity_score=50.0, demultiplexer=d,
                                 **OPTS)
    assert low.counts[0, 1] == 50 and low.counts[1:, :].tolist() == ps.counts[1:, :].tolist()


def test_summarize_pooled_from_pairs(d, gpu_aligner_factory):
    """The panel as pairs through the front end: the resident reads against the same call on
    their host copy, and against the host path on that copy."""
    rows, amps, reads = panel_rows()
    al = gpu_aligner_factory()
    al.set_reference(amps[0])
    with frontend.prepare_packed_resident(al, *cases.pairs_of(reads, n1=150)) as rr:
        assert len(rr) > 0
        text, off = np.ascontiguousarray(rr.fetch_text()), rr.offsets.copy()
        ps = demux.summarize_pooled(rows, rr, al, min_reads=10, min_identity_score=SCORE, demultiplexer=d, **OPTS)
    host = demux.summarize_pooled(rows, (text, off), al, min_reads=10, min_identity_score=SCORE, demultiplexer=d, **OPTS)
    assert np.array_equal(ps.counts, host.counts) and ps.skipped == host.skipped and len(ps.skipped) < 8
    pd.testing.assert_frame_equal(ps.frame, host.frame)
    assert np.array_equal(ps.result.which, host.result.which) and np.array_equal(ps.result.order, host.result.order)
    batches, res, skipped = demux.align_demultiplexed(amps, (text, off), al, min_reads=10, demultiplexer=d)
    assert skipped == ps.skipped
    with quantify.GpuQuantifier(0) as gq:
        for g in range(8):
            if g not in skipped:
                assert ps.counts[g].tolist() == host_slots(batches[g], rows[g], gq), g
    assert ps.counts[:, 1].sum() > 0
    with pytest.raises(ValueError, match="released"):
        demux.summarize_pooled(rows, rr, al, demultiplexer=d)


def test_a_long_amplicon_prints_100_with_one_mismatch(d, gpu_aligner_factory):
    """One 2,100-base amplicon: exact, one substitution (2099/2100 prints 100.0: UNMODIFIED), two
    substitutions, a 3-base deletion.

    At this length the quantifier's vectors and histograms do not fit in LDS beside the rest: it
    keeps them in each block's slab in HBM (quant_kernel_long), on the resident ops and on host
    rows alike.  The totals of that form are held to the CPU oracle here as well, with a coding
    sequence over the deletion so that the histograms and counters are used."""
    amp = synth.random_amplicon(2100, 77)
    a = amp.encode()
    reads = [a, dc.substitute(a, 1000), dc.substitute(dc.substitute(a, 900), 1200), a[:1050] + a[1053:]]
    rows = [{"Name": "long", "Amplicon_Sequence": amp, "sgRNA": "", "Expected_HDR": "", "Coding_sequence": ""}]
    al = gpu_aligner_factory()
    batches, res, skipped = demux.align_demultiplexed([amp], pack(reads), al, demultiplexer=d)
    assert batches[0].stats["aln_len"].tolist() == [2100] * 4
    assert batches[0].stats["n_ident"].tolist() == [2100, 2099, 2098, 2097]
    assert oracle_slots(rows[0], reads)[:4] == [4, 4, 2, 2]
    ps = demux.summarize_pooled(rows, pack(reads), al, min_reads=0, demultiplexer=d, **OPTS)
    with quantify.GpuQuantifier(0) as gq:
        want = host_slots(batches[0], rows[0], gq)
    assert ps.counts[0].tolist() == want == oracle_slots(rows[0], reads)
    assert want[:4] == [4, 4, 2, 2]          # the read with one substitution is UNMODIFIED to the reference
    assert ps.frame["Unmodified%"][0] == 50.0 and ps.frame["Reads_aligned"][0] == 4.0
    # the totals of the long form against quant_oracle, frameshift analysis on
    coding = dict(rows[0], Coding_sequence=amp[1000:1100])
    args = quant_args(coding)
    df = kept_frame(batches[0])
    with quantify.GpuQuantifier(0) as gq:
        out = quantify.quantify_alignments(df.copy(), args, quantifier=gq, globals_=quantify.globals_from_args(args))
    exon, spl = qo.exon_splicing_positions(amp, coding["Coding_sequence"])
    prm = qo.QuantParams(len(amp), qo.include_idxs(len(amp), [], 1, 15, 15), exon, spl)
    ref = qo.process_rows(df["ref_seq"].tolist(), df["align_str"].tolist(), df["align_seq"].tolist(),
                          (df["score_ref"] == 100).to_numpy(), None, None, prm)
    for k, name in enumerate(quantify.VECTOR_NAMES[:13]):
        assert np.array_equal(out[1 + k], ref["vectors"][name]), name
    assert np.array_equal(out[16], ref["vectors"]["avg_vector_del_all"])
    assert np.array_equal(out[17], ref["vectors"]["avg_vector_ins_all"])
    assert out[14] == ref["hist_inframe"] == {-3: 1} and out[15] == ref["hist_frameshift"] == {}
    assert list(out[18:22]) == [ref["counters"][c] for c in quantify.COUNTER_NAMES]
    assert out[3].sum() == 2 and out[2].sum() == 3 and out[0]["NHEJ"].sum() == 2


# ---- the command line --------------------------------------------------------------------------

def write_fastq(path, names, seqs):
    with open(path, "wb") as f:
        for nm, s in zip(names, seqs):
            f.write(b"@" + nm + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")


def test_command_line_from_pairs_to_the_summary(tmp_path, gpu_aligner_factory):
    amps, reads = dc.pooled_panel()
    amps, reads = amps[:3], [r for j, r in enumerate(reads) if j % 8 < 3][:60]
    table = tmp_path / "amplicons.txt"
    table.write_text("".join("A%d\t%s\n" % (g, a) for g, a in enumerate(amps)))
    r1, r2 = str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq")
    write_fastq(r1, [b"read%d/1" % j for j in range(60)], [r[:150] for r in reads])
    write_fastq(r2, [b"read%d/2" % j for j in range(60)], [dm.revcomp(r[-150:]) for r in reads])
    out = str(tmp_path / "out")
    assert demux.main(["-f", str(table), "-r1", r1, "-r2", r2, "-o", out, "--summary",
                       "--min_reads_to_use_region", "5"]) == 0
    rows = demux.read_amplicons_file(str(table))
    al = gpu_aligner_factory()
    al.set_reference(amps[0])
    rr, names = frontend.prepare_fastq_resident(al, r1, r2, with_quals=True)
    with rr:
        text, qual, off = rr.fetch_text(), rr.fetch_quals(), rr.offsets
        ps = demux.summarize_pooled(rows, rr, al, min_reads=5)
    assert len(names) == len(rr) == len(rr.headers) and rr.headers[0] == b"read%d" % int(rr.src[0])
    assert len(qual) == len(text) == int(off[-1])
    want = str(tmp_path / "want.txt")
    demux.write_summary(want, ps.frame)
    got = open(os.path.join(out, "SAMPLES_QUANTIFICATION_SUMMARY.txt"), "rb").read()
    assert got == open(want, "rb").read() and got.count(b"\n") == 4 and ps.counts[:, 1].sum() > 0
    # the per-amplicon files hold the merged reads under R1's headers
    g = int(np.argmax(ps.result.counts))
    with gzip.open(os.path.join(out, "AMPL_A%d.fastq.gz" % g), "rb") as f:
        lines = f.read().split(b"\n")
    sel = ps.result.order[int(ps.result.group_offsets[g]):int(ps.result.group_offsets[g + 1])]
    assert len(lines) == 4 * len(sel) + 1 and len(sel) > 0
    j = int(sel[0])
    merged = text[off[j]:off[j + 1]].tobytes()
    assert lines[0] == b"@" + rr.headers[j] and not lines[0].endswith(b"/1")
    assert lines[1] == (dm.revcomp(merged) if ps.result.strand[j] else merged) and len(lines[3]) == len(merged)
