"""Expected_HDR rows of the pooled and WGS summaries in HBM (nws_set_printed, nws_printed,
nws_flags_dual of include/crispr_summary.h; summarize_pooled / summarize_regions with allow_hdr):
the two kernels against tests/hdr_summary_model.py, every rounding midpoint included; the whole
calls against a host path built from the earlier API (both reference passes downloaded, the
printed identities, pre_flags, quantify_alignments with expected_hdr_amplicon_seq, run_summary)
and against the CPU oracles; both command lines to the summary file's bytes.  Everything exact."""
import ctypes
import os
import types

import numpy as np
import pandas as pd
import pytest

from crispresso_amd import _lib, demux, frontend, quantify, regions
from crispresso_amd.aligner import printed_percent
from crispresso_amd.devmem import DeviceBuffer
from crispresso_amd.pooled import align_pooled
from tests import demux_model as dm
from tests import hdr_summary_model as hm
from tests import pooled_summary_cases as cases
from tests import pooled_summary_model as psm
from tests.alleles_cases import pack

pytestmark = pytest.mark.gpu
SCORE, THRESHOLD, OPTS = hm.SCORE, hm.THRESHOLD, hm.OPTS
MAX_COLS = 2000
HDR, MIXED = _lib.NWQ_PRE_HDR, _lib.NWQ_PRE_MIXED


@pytest.fixture(scope="module")
def d():
    with demux.GpuDemultiplexer(0) as x:
        yield x


@pytest.fixture(scope="module")
def tables():
    return demux.printed_tables(SCORE, THRESHOLD)


@pytest.fixture(scope="module")
def summarizer(tables):
    with demux.GpuSummarizer(0) as s:
        s.set_printed(*tables)
        s.set_identity(*demux.identity_thresholds(SCORE, MAX_COLS))
        yield s


# ---- nws_printed -------------------------------------------------------------------------------

SPECIAL = [(6, 10, 0), (150, 250, 0), (151, 250, 0), (1999, 2000, 0), (1998, 2000, 0), (0, 0, 1), (250, 250, 1),
           (0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1000, 0), (MAX_COLS, MAX_COLS, 0)]       # (n_ident, aln_len, flags)


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


def records_of(pairs):
    st = np.zeros(len(pairs), _lib.STAT_DTYPE)
    st["n_ident"], st["aln_len"] = [p[0] for p in pairs], [p[1] for p in pairs]
    return st


def run_printed(s, st):
    n = len(st)
    out = np.full(n, 0xAAAA, np.uint16)
    bad, ms = ctypes.c_int64(-1), ctypes.c_float(-1.0)
    with DeviceBuffer.from_array(st) as d_st, DeviceBuffer(2 * n) as d_out:
        rc = s._lib.nws_printed(s._ctx, d_st.ptr, n, d_out.ptr, ctypes.byref(bad), ctypes.byref(ms))
        if n:
            d_out.download(out)
    return rc, out, int(bad.value), float(ms.value)


def run_dual(s, st, rep):
    n = len(st)
    pre, keep = np.full(n, 0xAA, np.uint8), np.full(n, 0xAA, np.uint8)
    bad, ms = ctypes.c_int64(-1), ctypes.c_float(-1.0)
    with DeviceBuffer.from_array(st) as d_st, DeviceBuffer.from_array(np.ascontiguousarray(rep, np.uint16)) as d_rep, \
            DeviceBuffer(n) as d_pre, DeviceBuffer(n) as d_keep:
        rc = s._lib.nws_flags_dual(s._ctx, d_st.ptr, d_rep.ptr, n, d_pre.ptr, d_keep.ptr, ctypes.byref(bad),
                                   ctypes.byref(ms))
        if n:
            d_pre.download(pre)
            d_keep.download(keep)
    return rc, pre, keep, int(bad.value), float(ms.value)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_printed(summarizer, tables, n):
    st = stat_records(n)
    rc, got, bad, ms = run_printed(summarizer, st)
    want, want_bad = hm.printed(st["aln_len"], st["n_ident"], st["flags"], tables[0])
    assert rc == 0 and bad == want_bad == 0 and np.array_equal(got, want)
    live = (st["flags"] & 1) == 0
    assert got[live].tolist() == [round(printed_percent(int(i), int(L)) * 10) for i, L in
                                  zip(st["n_ident"][live], st["aln_len"][live])]
    if n == 0:
        assert ms == 0.0
    if n >= len(SPECIAL):
        assert got[:len(SPECIAL)].tolist() == [600, 600, 604, 1000, 999, 0xFFFF, 0xFFFF, 0, 0, 1000, 1, 1000]


def test_printed_on_every_rounding_midpoint(summarizer, tables):
    """aln_len 2000 with every odd n_ident: one record per table entry, with its two neighbours."""
    tie_up = tables[0]
    pairs = []
    for t in range(1000):
        pairs += [(2 * t + 1, 2000), (t, 1000), (t + 1, 1000)]
    st = records_of(pairs)
    rc, got, bad, _ = run_printed(summarizer, st)
    assert rc == 0 and bad == 0
    assert got.tolist() == [x for t in range(1000) for x in (t + int(tie_up[t]), t, t + 1)]
    assert got.tolist() == [round(printed_percent(i, L) * 10) for i, L in pairs]
    assert np.array_equal(got, hm.printed(st["aln_len"], st["n_ident"], st["flags"], tie_up)[0])
    assert 0 < int(tie_up.sum()) < 1000


def test_printed_out_of_range(summarizer, tables):
    big = _lib_max_cols()
    st = records_of([(5, 10), (0, 0), (1, big + 1), (11, 10), (big, big), (big - 1, big), (big // 2, big)])
    st["flags"][0] = _lib.NW_FLAG_EMPTY
    rc, got, bad, _ = run_printed(summarizer, st)
    assert rc == _lib.NW_E_INVALID and bad == 2 and b"outside" in summarizer._lib.nws_last_error(summarizer._ctx)
    assert got.tolist() == [0xFFFF, 0, 0xFFFF, 0xFFFF, 1000, 1000, 500]
    want, want_bad = hm.printed(st["aln_len"], st["n_ident"], st["flags"], tables[0])
    assert want_bad == 2 and np.array_equal(got, want)
    with pytest.raises(demux.SummaryError) as exc, DeviceBuffer.from_array(st) as d_st, DeviceBuffer(2 * len(st)) as out:
        summarizer.printed(d_st.ptr, len(st), out.ptr)
    assert exc.value.code == _lib.NW_E_INVALID and exc.value.n_out_of_range == 2
    assert run_printed(summarizer, stat_records(64))[0] == 0          # the context still works


def _lib_max_cols():
    text = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "crispr_summary.h")).read()
    assert "#define NWS_MAX_COLS (1 << 20)" in text
    return 1 << 20


# ---- nws_flags_dual ----------------------------------------------------------------------------

# (ref n_ident, ref aln_len, repaired n_ident, repaired aln_len) -> (keep, pre)
STRADDLE = [((60, 100, 601, 1000), (1, MIXED)),        # ref prints 60.0 (not > 60), repaired 60.1: kept by it alone
            ((60, 100, 60, 100), (0, 0)),              # both print 60.0: dropped
            ((59, 100, 150, 250), (0, MIXED)),         # 59.0 and 60.0: dropped, though the repaired is higher
            ((95, 100, 190, 200), (1, 0)),             # equal printed values from different lengths: not HDR
            ((190, 200, 951, 1000), (1, MIXED)),       # 95.0 against 95.1
            ((90, 100, 196, 200), (1, HDR)),           # repaired prints 98.0
            ((90, 100, 979, 1000), (1, MIXED)),        # repaired prints 97.9
            ((1959, 2000, 196, 200), (1, 0)),          # 97.95 is a midpoint that prints 98.0 (or 97.9): see below
            ((100, 100, 100, 100), (1, 1)),            # both 100.0: UNMODIFIED, difference 0
            ((99, 100, 200, 200), (1, HDR)),
            ((61, 100, 50, 100), (1, 0))]


def dual_records(n, tables, seed=3):
    """n ref records and n repaired tenths; the straddling pairs first."""
    st = stat_records(n, seed)
    rep_st = stat_records(n, seed + 1)
    near = np.arange(n) % 3 == 0                       # a repaired identity next to the ref identity
    rep_st["aln_len"][near] = st["aln_len"][near]
    rep_st["n_ident"][near] = np.clip(st["n_ident"][near] + (np.arange(n)[near] % 5 - 2), 0, st["aln_len"][near])
    for j, ((i, L, ih, Lh), _) in enumerate(STRADDLE[:n]):
        st["n_ident"][j], st["aln_len"][j], st["flags"][j] = i, L, 0
        rep_st["n_ident"][j], rep_st["aln_len"][j], rep_st["flags"][j] = ih, Lh, 0
    if n > len(STRADDLE):
        rep_st["flags"][len(STRADDLE)] = _lib.NW_FLAG_EMPTY       # a read without a repaired score
    rep, bad = hm.printed(rep_st["aln_len"], rep_st["n_ident"], rep_st["flags"], tables[0])
    assert bad == 0
    return st, rep


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_flags_dual(summarizer, tables, n):
    tie_up, keep_tenths, hdr_tenths = tables
    st, rep = dual_records(n, tables)
    rc, pre, keep, bad, ms = run_dual(summarizer, st, rep)
    want_pre, want_keep, want_bad = hm.flags_dual(st["aln_len"], st["n_ident"], st["flags"], rep, *tables)
    assert rc == 0 and bad == want_bad == 0
    assert np.array_equal(pre, want_pre) and np.array_equal(keep, want_keep)
    # and the reference's expressions on the printed floats, where there is a repaired score
    has = rep <= 1000
    sr = [printed_percent(int(i), int(L)) for i, L in zip(st["n_ident"][has], st["aln_len"][has])]
    kept, ref_pre = hm.reference_rule(sr, rep[has] / 10.0, SCORE, THRESHOLD)
    assert np.array_equal(pre[has], ref_pre) and np.array_equal(keep[has].astype(bool), kept & ((st["flags"][has] & 1) == 0))
    if n == 0:
        assert ms == 0.0
    if n >= len(STRADDLE):
        for j, (pair, (k, p)) in enumerate(STRADDLE):
            if pair == (1959, 2000, 196, 200):         # the midpoint 97.95 prints what the table says
                p = HDR if tie_up[979] == 0 else 0
            assert (int(keep[j]), int(pre[j])) == (k, p), pair
        assert (pre & HDR).any() and (pre & MIXED).any() and (keep == 0).any() and (rep == 0xFFFF).any()


def test_flags_dual_on_its_own_records_is_nws_flags(summarizer, tables):
    """The repaired tenths taken from the ref records themselves: keep and UNMODIFIED are
    nws_flags' with identity_thresholds at the same score, and nothing is HDR or MIXED."""
    for n in (1, 65, 257, 3000):
        st = stat_records(n, 5) if n < 3000 else records_of([p for t in range(1000) for p in
                                                             ((2 * t + 1, 2000), (t, 1000), (t + 1, 1000))])
        with DeviceBuffer.from_array(st) as d_st, DeviceBuffer(2 * n) as d_rep, DeviceBuffer(n) as d_pre, \
                DeviceBuffer(n) as d_keep, DeviceBuffer(n) as d_pre1, DeviceBuffer(n) as d_keep1:
            summarizer.printed(d_st.ptr, n, d_rep.ptr)
            summarizer.flags_dual(d_st.ptr, d_rep.ptr, n, d_pre.ptr, d_keep.ptr)
            assert summarizer.flags_ms > 0 and summarizer.printed_ms > 0
            summarizer.flags(d_st.ptr, n, d_pre1.ptr, d_keep1.ptr)
            got = [b.download(np.zeros(n, np.uint8)) for b in (d_pre, d_keep, d_pre1, d_keep1)]
        assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3]), n
        assert not (got[0] & (HDR | MIXED)).any()
    assert got[1].any() and got[0].any() and not got[1].all()


def test_flags_dual_out_of_range(summarizer, tables):
    st = records_of([(90, 100), (90, 100), (90, 100), (11, 10), (100, 100)])
    rep = np.array([0xFFFF, 1001, 0xFFFE, 990, 990], np.uint16)
    st["flags"][4] = _lib.NW_FLAG_EMPTY
    rc, pre, keep, bad, _ = run_dual(summarizer, st, rep)
    assert rc == _lib.NW_E_INVALID and bad == 3
    assert keep.tolist() == [1, 0, 0, 0, 0] and pre.tolist() == [0, 0, 0, 0, 1]       # an empty read is never kept
    want = hm.flags_dual(st["aln_len"], st["n_ident"], st["flags"], rep, *tables)
    assert np.array_equal(pre, want[0]) and np.array_equal(keep, want[1]) and want[2] == 3
    assert run_dual(summarizer, *dual_records(64, tables))[0] == 0


def test_before_the_tables():
    with demux.GpuSummarizer(0) as fresh, DeviceBuffer(64) as buf:
        assert fresh._lib.nws_flags_dual(fresh._ctx, buf.ptr, buf.ptr, 2, buf.ptr, buf.ptr, None, None) == _lib.NW_E_STATE
        assert fresh._lib.nws_printed(fresh._ctx, buf.ptr, 2, buf.ptr, None, None) == _lib.NW_E_STATE
        assert fresh._lib.nws_set_printed(fresh._ctx, None, 601, 980) == _lib.NW_E_INVALID
        tie_up = demux.printed_tables(SCORE, THRESHOLD)[0]
        assert fresh._lib.nws_set_printed(fresh._ctx, _lib.ptr(tie_up), 1002, 980) == _lib.NW_E_INVALID
        assert fresh._lib.nws_flags_dual(fresh._ctx, buf.ptr, buf.ptr, 2, buf.ptr, buf.ptr, None, None) == _lib.NW_E_STATE


# ---- the host path the calls replace -----------------------------------------------------------

def quant_args(row, hdr, threshold):
    return types.SimpleNamespace(
        amplicon_seq=row["Amplicon_Sequence"], guide_seq=row["sgRNA"] or None, coding_seq=row["Coding_sequence"] or None,
        ignore_substitutions=False, ignore_insertions=False, ignore_deletions=False,
        hide_mutations_outside_window_NHEJ=False, expected_hdr_amplicon_seq=hdr or None,
        hdr_perfect_alignment_threshold=threshold, **OPTS)


def host_slots(batch, batch_hdr, row, gq, score=SCORE, threshold=THRESHOLD):
    """The 16 slots by the earlier API: the rows of both passes on the host, the two printed
    identities, the reference's filter, quantify_alignments (pre_flags inside), run_summary."""
    recs = []
    for i in range(len(batch)):
        if batch.empty(i):
            continue
        sr = printed_percent(int(batch.stats["n_ident"][i]), int(batch.stats["aln_len"][i]))
        sp = float("nan") if batch_hdr is None else \
            printed_percent(int(batch_hdr.stats["n_ident"][i]), int(batch_hdr.stats["aln_len"][i]))
        if sr > score or sp > score:
            recs.append((batch.ref_seq(i), batch.align_str(i), batch.align_seq(i), sr, sp, sr - sp))
    df = pd.DataFrame(recs, columns=["ref_seq", "align_str", "align_seq", "score_ref", "score_repaired", "score_diff"])
    args = quant_args(row, row["Expected_HDR"] if batch_hdr is not None else None, threshold)
    out = quantify.quantify_alignments(df, args, quantifier=gq, globals_=quantify.globals_from_args(args))
    cuts = quantify.compute_cut_points(row["Amplicon_Sequence"], args.guide_seq, args.cleavage_offset)
    return psm.slots_of_summary(quantify.run_summary(out[0], len(row["Amplicon_Sequence"]), cuts), len(batch))


def host_counts(rows, groups, al, keep, score=SCORE, threshold=THRESHOLD):
    """{g: slots} of the groups (packed (buf, offsets) pairs) in keep."""
    amps = [r["Amplicon_Sequence"] for r in rows]
    batches = dict(zip(keep, align_pooled([amps[g] for g in keep], [groups[g] for g in keep], al)))
    with_hdr = [g for g in keep if rows[g]["Expected_HDR"]]
    hdr_batches = dict(zip(with_hdr, align_pooled([rows[g]["Expected_HDR"] for g in with_hdr],
                                                  [groups[g] for g in with_hdr], al)))
    with quantify.GpuQuantifier(0) as gq:
        return {g: host_slots(batches[g], hdr_batches.get(g), rows[g], gq, score, threshold) for g in keep}, batches


def check_frame(frame, rows, n_reads, counts, skipped):
    assert list(frame.columns) == list(demux.SUMMARY_COLUMNS) and frame["Name"].tolist() == [r["Name"] for r in rows]
    assert frame["Reads_total"].tolist() == list(n_reads)
    for g in range(len(rows)):
        if g in skipped:
            assert frame.iloc[g][1:6].isna().all()
            continue
        s, total = counts[g], float(counts[g][1])
        assert frame.iloc[g][1:6].tolist() == [s[2] / total * 100., s[3] / total * 100., s[4] / total * 100.,
                                              s[5] / total * 100., total]


# ---- summarize_pooled(allow_hdr=True) ----------------------------------------------------------

@pytest.fixture(scope="module")
def panel(d, gpu_aligner_factory):
    """(rows, reads, the model's assignment, {g: host slots}, the amplicon pass's batches)."""
    rows, reads, origin = hm.panel()
    want = dm.demultiplex([r["Amplicon_Sequence"].encode() for r in rows], reads)
    assert want["which"] == origin
    al = gpu_aligner_factory()
    res = demux.demultiplex([r["Amplicon_Sequence"] for r in rows], pack(reads), demultiplexer=d)
    assert res.which.tolist() == origin
    host, batches = host_counts(rows, res.reads_per_amplicon(), al, range(4))
    return rows, reads, want, host, batches


def test_summarize_pooled_with_expected_hdr(d, gpu_aligner_factory, panel):
    rows, reads, want, host, batches = panel
    al = gpu_aligner_factory()
    seen = []

    def on_group(g, a, n):
        ob = a.download_ops(n)
        seen.append((g, n, a.reference, ob.stats["aln_len"].tolist(), ob.stats["n_ident"].tolist()))

    ps = demux.summarize_pooled(rows, pack(reads), al, min_reads=5, min_identity_score=SCORE, demultiplexer=d,
                                allow_hdr=True, on_group=on_group, **OPTS)
    assert ps.result.n_tie == 0 and ps.result.n_no_hit == 0 and ps.skipped == [] and al.output_mode == "rows"
    assert ps.result.counts.tolist() == want["counts"] and ps.result.which.tolist() == want["which"]
    for g in range(4):
        assert ps.counts[g].tolist() == host[g], g
        assert ps.counts[g].tolist() == hm.oracle_slots(rows[g], want["groups"][g])[0], g
    # a test that passes with zeros in HDR and Mixed shows nothing
    assert (ps.counts[:3, 4] > 0).all() and (ps.counts[:3, 5] > 0).all() and ps.counts[3, 4] == ps.counts[3, 5] == 0
    assert ps.counts[0, :6].tolist() == [30, 28, 8, 6, 9, 5] and not ps.counts[:, 15].any()
    check_frame(ps.frame, rows, want["counts"], ps.counts, [])
    assert (ps.frame["HDR%"][:3] > 0).all() and (ps.frame["Mixed_HDR-NHEJ%"][:3] > 0).all()
    # on_group saw the pass against the amplicon, not the one against Expected_HDR
    assert [(g, n, ref) for g, n, ref, _, _ in seen] == [(g, want["counts"][g], rows[g]["Amplicon_Sequence"]) for g in range(4)]
    for g, _, _, aln_len, n_ident in seen:
        assert aln_len == batches[g].stats["aln_len"].tolist() and n_ident == batches[g].stats["n_ident"].tolist(), g
    assert set(ps.kernel_ms) == {"flags", "summary", "quantify", "printed", "hdr_pass"}
    assert min(ps.kernel_ms.values()) > 0
    # again on the same contexts; and the rows without Expected_HDR are what the plain call gives
    again = demux.summarize_pooled(rows, pack(reads), al, min_reads=5, min_identity_score=SCORE, demultiplexer=d,
                                   allow_hdr=True, **OPTS)
    assert np.array_equal(again.counts, ps.counts)
    pd.testing.assert_frame_equal(again.frame, ps.frame)
    plain_rows = [dict(r, Expected_HDR="") for r in rows]
    plain = demux.summarize_pooled(plain_rows, pack(reads), al, min_reads=5, min_identity_score=SCORE, demultiplexer=d, **OPTS)
    allowed = demux.summarize_pooled(plain_rows, pack(reads), al, min_reads=5, min_identity_score=SCORE, demultiplexer=d,
                                     allow_hdr=True, **OPTS)
    assert np.array_equal(plain.counts, allowed.counts) and np.array_equal(plain.counts[3], ps.counts[3])
    assert not plain.counts[:, 4:6].any() and plain.kernel_ms["printed"] == 0.0 and plain.kernel_ms["hdr_pass"] == 0.0
    assert (plain.counts[:3, 1] < ps.counts[:3, 1]).all()          # the reads kept by the repaired score alone
    with pytest.raises(ValueError, match="AMP_0: Expected_HDR is given, and dual alignment per amplicon is not built"):
        demux.summarize_pooled(rows, pack(reads), al, min_reads=5, demultiplexer=d, **OPTS)


def test_summarize_pooled_other_score_and_threshold(d, gpu_aligner_factory, panel):
    """A threshold of 98.1 turns the reads that print 98.0 from HDR to MIXED; a score of 60.5
    drops the reads the repaired score kept at 60."""
    rows, reads, want, host, _ = panel
    al = gpu_aligner_factory()
    for score, threshold in ((SCORE, 98.1), (60.5, THRESHOLD)):
        ps = demux.summarize_pooled(rows, pack(reads), al, min_reads=5, min_identity_score=score, demultiplexer=d,
                                    allow_hdr=True, hdr_perfect_alignment_threshold=threshold, **OPTS)
        for g in range(4):
            assert ps.counts[g].tolist() == hm.oracle_slots(rows[g], want["groups"][g], score, threshold)[0], (g, score)
        if threshold != THRESHOLD:
            assert ps.counts[0, 4] == host[0][4] - 3 and ps.counts[0, 5] == host[0][5] + 3
        else:
            assert ps.counts[0, 1] == host[0][1] - 2 and ps.counts[0, 5] == host[0][5] - 2


def test_summarize_pooled_with_expected_hdr_from_pairs(d, gpu_aligner_factory, panel):
    """The panel as pairs through the front end: the resident reads against the same call on
    their host copy, and against the host path on that copy."""
    rows, reads, _, _, _ = panel
    al = gpu_aligner_factory()
    al.set_reference(rows[0]["Amplicon_Sequence"])
    kw = dict(min_reads=5, min_identity_score=SCORE, demultiplexer=d, allow_hdr=True, **OPTS)
    with frontend.prepare_packed_resident(al, *cases.pairs_of(reads, n1=110)) as rr:
        assert len(rr) > 0
        text, off = np.ascontiguousarray(rr.fetch_text()), rr.offsets.copy()
        ps = demux.summarize_pooled(rows, rr, al, **kw)
    host = demux.summarize_pooled(rows, (text, off), al, **kw)
    assert np.array_equal(ps.counts, host.counts) and ps.skipped == host.skipped == []
    pd.testing.assert_frame_equal(ps.frame, host.frame)
    res = demux.demultiplex([r["Amplicon_Sequence"] for r in rows], (text, off), demultiplexer=d)
    assert res.counts.tolist() == ps.result.counts.tolist()
    want, _ = host_counts(rows, res.reads_per_amplicon(), al, range(4))
    for g in range(4):
        assert ps.counts[g].tolist() == want[g], g
    assert (ps.counts[:3, 4] > 0).all() and (ps.counts[:3, 5] > 0).all()


# ---- summarize_regions(allow_hdr=True) ---------------------------------------------------------

@pytest.fixture(scope="module")
def wgs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hdr_wgs")
    bam_path, table, fasta = hm.write_region_inputs(tmp)
    rows = regions.wgs_rows(regions.read_wgs_region_file(table), fasta)
    return tmp, bam_path, table, fasta, rows


def test_summarize_regions_with_expected_hdr(gpu_aligner_factory, wgs):
    tmp, bam_path, table, fasta, rows = wgs
    assert rows[0]["Expected_HDR"] and not rows[1]["Expected_HDR"]
    bam = regions.read_bam(bam_path)
    targets = [(r["chr_id"], r["bpstart"], r["bpend"], r["Name"]) for r in rows]
    al = gpu_aligner_factory()
    seen = []
    with regions.GpuRegionExtractor(0) as x:
        plain = regions.extract_regions(bam, targets, extractor=x)
        model = hm.region_model_reads()
        for g in range(2):
            buf, off = plain.reads(g)
            assert [buf[off[k]:off[k + 1]].tobytes() for k in range(len(off) - 1)] == model[g]
        host, _ = host_counts(rows, [plain.reads(g) for g in range(2)], al, range(2))
        with regions.extract_regions_resident(bam, targets, extractor=x) as res:
            rs = regions.summarize_regions(rows, res, al, min_identity_score=SCORE, allow_hdr=True,
                                           on_group=lambda g, a, n: seen.append((g, n, a.reference)), **OPTS)
            other = regions.summarize_regions(rows, res, al, min_identity_score=SCORE, allow_hdr=True,
                                              hdr_perfect_alignment_threshold=98.2, **OPTS)
            with pytest.raises(ValueError, match="hdr_region_0: Expected_HDR is given, and dual alignment per region"):
                regions.summarize_regions(rows, res, al, **OPTS)
            with pytest.raises(ValueError, match="region hdr_region_0.*cannot be the same"):
                regions.summarize_regions([dict(rows[0], Expected_HDR=rows[0]["Amplicon_Sequence"]), rows[1]], res, al,
                                          allow_hdr=True)
    assert rs.skipped == [] and al.output_mode == "rows"
    assert seen == [(g, hm.REGION_RECORDS[g], rows[g]["Amplicon_Sequence"]) for g in range(2)]
    for g in range(2):
        assert rs.counts[g].tolist() == host[g], g
        assert rs.counts[g].tolist() == hm.oracle_slots(rows[g], model[g])[0], g
    assert rs.counts[0, :6].tolist() == [24, 20, 4, 4, 8, 4] and rs.counts[1, 4] == rs.counts[1, 5] == 0
    check_frame(rs.frame, rows, hm.REGION_RECORDS, rs.counts, [])
    assert rs.kernel_ms["printed"] > 0 and rs.kernel_ms["hdr_pass"] > 0
    assert other.counts[0, 4:6].tolist() == [4, 8] and np.array_equal(other.counts[1], rs.counts[1])    # 98.1 is MIXED at 98.2
    # the command line writes the same table
    out = str(tmp / "cli")
    assert regions.main(["--bam", bam_path, "--regions", table, "--genome", fasta, "--summary", "--hdr",
                         "--out", out]) == 0
    want = str(tmp / "want.txt")
    demux.write_summary(want, rs.frame)
    got = open(os.path.join(out, "SAMPLES_QUANTIFICATION_SUMMARY.txt"), "rb").read()
    assert got == open(want, "rb").read() and got.count(b"\n") == 3
    assert got.split(b"\n")[1].split(b"\t")[3:5] == [b"40.0", b"20.0"]
    with pytest.raises(ValueError, match="dual alignment per region is not built"):      # without --hdr: refused as before
        regions.main(["--bam", bam_path, "--regions", table, "--genome", fasta, "--summary", "--out", str(tmp / "no")])


# ---- the pooled command line -------------------------------------------------------------------

def write_fastq(path, names, seqs):
    with open(path, "wb") as f:
        for nm, s in zip(names, seqs):
            f.write(b"@" + nm + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")


def test_command_line_from_pairs_to_the_summary_with_hdr(tmp_path, gpu_aligner_factory):
    rows, reads, _ = hm.panel()
    table = tmp_path / "amplicons.txt"
    table.write_text("".join("%s\t%s\t%s\t%s\n" % (r["Name"], r["Amplicon_Sequence"], r["sgRNA"], r["Expected_HDR"].lower())
                             for r in rows))
    r1, r2 = str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq")
    write_fastq(r1, [b"read%d/1" % j for j in range(len(reads))], [r[:110] for r in reads])
    write_fastq(r2, [b"read%d/2" % j for j in range(len(reads))], [dm.revcomp(r[-110:]) for r in reads])
    out = str(tmp_path / "out")
    assert demux.main(["-f", str(table), "-r1", r1, "-r2", r2, "-o", out, "--summary", "--hdr",
                       "--min_reads_to_use_region", "5"]) == 0
    assert demux.read_amplicons_file(str(table)) == rows
    al = gpu_aligner_factory()
    al.set_reference(rows[0]["Amplicon_Sequence"])
    rr, _ = frontend.prepare_fastq_resident(al, r1, r2, with_quals=True)
    with rr:
        ps = demux.summarize_pooled(rows, rr, al, min_reads=5, allow_hdr=True)
        strict = demux.summarize_pooled(rows, rr, al, min_reads=5, allow_hdr=True, hdr_perfect_alignment_threshold=99.0)
    want = str(tmp_path / "want.txt")
    demux.write_summary(want, ps.frame)
    got = open(os.path.join(out, "SAMPLES_QUANTIFICATION_SUMMARY.txt"), "rb").read()
    assert got == open(want, "rb").read() and got.count(b"\n") == 5
    assert (ps.counts[:3, 4] > 0).all() and (ps.counts[:3, 5] > 0).all()
    out2 = str(tmp_path / "out2")
    assert demux.main(["-f", str(table), "-r1", r1, "-r2", r2, "-o", out2, "--summary", "--hdr",
                       "--hdr_perfect_alignment_threshold", "99.0", "--min_reads_to_use_region", "5"]) == 0
    demux.write_summary(want, strict.frame)
    got2 = open(os.path.join(out2, "SAMPLES_QUANTIFICATION_SUMMARY.txt"), "rb").read()
    assert got2 == open(want, "rb").read() and got2 != got
    with pytest.raises(SystemExit):          # the same table without --hdr is refused as before
        demux.main(["-f", str(table), "-r1", r1, "-r2", r2, "-o", str(tmp_path / "no"), "--summary"])
    assert not os.path.exists(tmp_path / "no")
