"""The host side of the pooled summary (crispresso_amd.demux.summarize_pooled): the identity
threshold tables against a brute force of the printed identity, the 16-slot model
(tests/pooled_summary_model.py) against quantify.run_summary on frames quantified by the CPU
oracle, the summary file byte for byte, the command line's argument sets, and the ABI."""
import os

import numpy as np
import pandas as pd
import pytest

from crispresso_amd import _lib, demux, quantify
from crispresso_amd.aligner import printed_percent
from oracle import quant_oracle as qo
from tests import pooled_summary_model as psm
from tests.test_abi import declared_symbols

LONG = (1999, 2000, 2001, 4000, 12288)


# ---- identity thresholds -----------------------------------------------------------------------

@pytest.mark.parametrize("score", [60.0, 0.0, 99.95, 100.0, -1.0])
def test_identity_thresholds_equal_a_brute_force(score):
    keep_min, unmod_min = demux.identity_thresholds(score, 600)
    assert keep_min.dtype == unmod_min.dtype == np.int32 and len(keep_min) == len(unmod_min) == 601
    for L in range(601):
        assert (int(keep_min[L]), int(unmod_min[L])) == psm.brute_thresholds(score, L), L
    for L in LONG:
        k, u = demux.identity_thresholds(score, L, start=L)
        assert (int(k[L]), int(u[L])) == psm.brute_thresholds(score, L), L
        assert not k[:L].any() and not u[:L].any()


def test_printed_identity_does_not_decrease():
    for L in list(range(1, 300)) + [2000, 4001]:
        vals = [printed_percent(i, L) for i in range(L + 1)]
        assert all(a <= b for a, b in zip(vals, vals[1:])), L


def test_the_quoted_values():
    assert printed_percent(150, 250) == 60.0 and printed_percent(151, 250) == 60.4
    assert printed_percent(1999, 2000) == 100.0 and printed_percent(1998, 2000) == 99.9
    keep_min, unmod_min = demux.identity_thresholds(60.0, 2000)
    assert keep_min[250] == 151           # 150/250 prints 60.0 and is dropped; 151/250 is kept
    assert keep_min[10] == 7              # 6/10 likewise
    assert unmod_min[2000] == 1999        # one mismatch in 2000 columns prints 100.0
    assert unmod_min[1999] == 1999 and unmod_min[250] == 250
    assert keep_min[0] == 1 and unmod_min[0] == 1      # no columns: nothing printed is > 60 or 100.0
    with pytest.raises(ValueError):
        demux.identity_thresholds(60.0, -1)


# ---- the 16 slots against run_summary ----------------------------------------------------------

AMP = "ACGTTGCAAGGCTTACGATCGGATCCTAGACTGAAGTCCA"        # 40 bases
EDITS = [dict(), dict(sub=(12,)), dict(dele=(20, 3)), dict(ins=(25, "GG")),
         dict(sub=(8, 30), dele=(15, 2)), dict(sub=(9,), ins=(22, "T")), dict(dele=(10, 1), ins=(28, "ACG")),
         dict(sub=(5, 6, 33), dele=(18, 4), ins=(31, "C"))]       # every n_mutated/n_deleted/n_inserted > 0 pattern


def quantified_frame():
    """Every edit pattern as NHEJ (no HDR scores), as HDR and as MIXED (score_diff < 0, repaired
    above / below the threshold), the unedited row thrice among them, plus two rows UNMODIFIED on
    entry (one of them with edits, which the quantification then does not look at)."""
    rows, um, sd, sr = [], [], [], []
    for diff, repaired in ((1.0, 50.0), (-1.0, 99.0), (-1.0, 90.0)):
        for e in EDITS:
            rows.append(psm.aligned_rows(AMP, **e))
            um.append(False)
            sd.append(diff)
            sr.append(repaired)
    for e in (EDITS[0], EDITS[4]):
        rows.append(psm.aligned_rows(AMP, **e))
        um.append(True)
        sd.append(1.0)
        sr.append(50.0)
    prm = qo.QuantParams(len(AMP), frozenset(range(len(AMP))), expected_hdr=True)
    R, M, S = ([r[k] for r in rows] for k in range(3))
    res = qo.process_rows(R, M, S, um, sd, sr, prm)
    df = pd.DataFrame({"ref_seq": R, "align_str": M, "align_seq": S, "n_mutated": res["n_mutated"],
                       "n_inserted": res["n_inserted"], "n_deleted": res["n_deleted"],
                       **qo.class_flags(res["cls"], um)})
    return df, res, np.array(um, bool)


def test_the_frame_covers_every_class_and_pattern():
    df, res, um = quantified_frame()
    assert sorted(set(res["cls"].tolist())) == [0, 1, 2, 3]
    for c in (1, 2, 3):
        seen = {(m > 0, i > 0, d > 0) for k, m, i, d in zip(res["cls"], res["n_mutated"], res["n_inserted"],
                                                            res["n_deleted"]) if k == c}
        want = {(bool(a & 1), bool(a & 2), bool(a & 4)) for a in range(0 if c > 1 else 1, 8)}
        assert seen == want, c
    assert (res["cls"][um] == 0).all()


def test_slots_equal_run_summary():
    df, res, um = quantified_frame()
    pre = um.astype(np.uint8) * _lib.NWQ_PRE_UNMODIFIED
    n = len(df)
    masks = [np.ones(n, bool), np.arange(n) % 2 == 0, np.arange(n) % 3 != 1, np.zeros(n, bool)]
    for keep in masks:
        got = psm.slots(res["cls"], res["n_mutated"], res["n_inserted"], res["n_deleted"], pre, keep)
        want = quantify.run_summary(df[keep], len(AMP), [])
        assert got == psm.slots_of_summary(want, n)
    got = psm.slots(res["cls"], res["n_mutated"], res["n_inserted"], res["n_deleted"], pre, masks[0])
    assert got[1] == n and got[2] + got[3] + got[4] + got[5] == n and min(got[2:15]) > 0


def test_slot_15_counts_kept_rows_that_are_no_alignment():
    cls = np.array([-1, -1, 0, 1, -1])
    z = np.zeros(5, np.int64)
    got = psm.slots(cls, z, z + 1, z, np.zeros(5, np.uint8), np.array([1, 0, 1, 1, 1]))
    assert got[0] == 5 and got[1] == 4 and got[15] == 2 and got[2] == 1 and got[3] == 1 and got[6] == 1
    assert _lib.NWS_SLOT_NAMES[15] == "not_aligned" and len(_lib.NWS_SLOT_NAMES) == _lib.NWS_SLOTS == 16


# ---- the summary table and its file -------------------------------------------------------------

def test_summary_file_bytes(tmp_path):
    counts = np.zeros((3, 16), np.int64)
    counts[0, :6] = [1300, 1234, 617, 600, 10, 7]
    counts[2, :6] = [40, 3, 1, 2, 0, 0]
    frame = demux.summary_frame(["FANCF", "HEK3 site", "EMX1"], counts, [1300, 12, 40], skipped=[1])
    assert list(frame.columns) == list(demux.SUMMARY_COLUMNS)
    assert frame["Reads_aligned"].tolist()[0] == 1234.0 and np.isnan(frame["NHEJ%"][1])
    assert frame["Unmodified%"][0] == 617.0 / 1234.0 * 100. and frame["NHEJ%"][2] == 2.0 / 3.0 * 100.
    path = str(tmp_path / "SAMPLES_QUANTIFICATION_SUMMARY.txt")
    demux.write_summary(path, frame)
    want = ("Name\tUnmodified%\tNHEJ%\tHDR%\tMixed_HDR-NHEJ%\tReads_aligned\tReads_total\n"
            "FANCF\t50.0\t48.62236628849271\t0.8103727714748784\t0.5672609400324149\t1234.0\t1300\n"
            "HEK3 site\tNA\tNA\tNA\tNA\tNA\t12\n"
            "EMX1\t33.33333333333333\t66.66666666666666\t0.0\t0.0\t3.0\t40\n")
    assert open(path, "rb").read() == want.encode()


def test_no_read_aligned_is_a_row_of_na():
    counts = np.zeros((1, 16), np.int64)
    counts[0, 0] = 25
    frame = demux.summary_frame(["a"], counts, [25], skipped=[])
    assert frame.iloc[0].isna().sum() == 5 and frame["Reads_total"][0] == 25


# ---- the command line --------------------------------------------------------------------------

def parse(*argv):
    p = demux.build_parser()
    return demux.options_from_args(p, p.parse_args(["-f", "a.txt", "-r1", "r1.fq", "-o", "out", *argv]))


def test_the_old_arguments_give_the_old_call():
    assert parse() == dict(k=16, min_hits=2, both_strands=True, min_reads_to_use_region=1000)
    assert parse("--k", "12", "--min_hits", "3", "--forward_only", "--min_reads_to_use_region", "10") == \
        dict(k=12, min_hits=3, both_strands=False, min_reads_to_use_region=10)


def test_the_new_arguments():
    kw = parse("-r2", "r2.fq", "--summary")
    assert kw["fastq_r2"] == "r2.fq" and "front" not in kw
    assert kw["summary"] == dict(min_identity_score=60.0, window_around_sgrna=1, cleavage_offset=-3)
    kw = parse("-r2", "r2.fq", "-q", "20", "-s", "5", "--trim_sequences", "--trimmomatic_options_string", "MINLEN:40",
               "--min_paired_end_reads_overlap", "10", "--max_paired_end_reads_overlap", "65", "--summary",
               "--min_identity_score", "70", "--window_around_sgrna", "3", "--cleavage_offset", "-4")
    assert kw["front"]["min_bp_quality"] == 20 and kw["front"]["min_single_bp_quality"] == 5
    assert kw["front"]["trim"] == "MINLEN:40"
    assert (kw["front"]["flash"].min_overlap, kw["front"]["flash"].max_overlap) == (10, 65)
    assert kw["summary"] == dict(min_identity_score=70.0, window_around_sgrna=3, cleavage_offset=-4)
    assert parse("-q", "20") == dict(k=16, min_hits=2, both_strands=True, min_reads_to_use_region=1000,
                                     front={"min_bp_quality": 20})
    for bad in (["--trim_sequences"], ["--trimmomatic_options_string", "MINLEN:40"], ["--min_identity_score", "70"],
                ["--max_paired_end_reads_overlap", "65"]):
        with pytest.raises(SystemExit):
            parse(*bad)


def test_refusals_before_the_gpu(tmp_path, capsys):
    rows = [{"Name": "a", "Amplicon_Sequence": "ACGT" * 30, "sgRNA": "", "Expected_HDR": "", "Coding_sequence": ""},
            {"Name": "with_hdr", "Amplicon_Sequence": "TTGCA" * 30, "sgRNA": "", "Expected_HDR": "TTGCA" * 29 + "TTGCC",
             "Coding_sequence": ""}]
    with pytest.raises(ValueError, match="with_hdr.*dual alignment per amplicon is not built"):
        demux.summarize_pooled(rows, ([], []), aligner=None)
    long_row = [dict(rows[0], Name="long", Amplicon_Sequence="ACGT" * 8192)]
    with pytest.raises(ValueError, match="long has 32768 bases"):
        demux.summarize_pooled(long_row, ([], []), aligner=None)
    assert demux.check_summary_rows(rows[:1]) == ["ACGT" * 30]
    # the command line refuses the same table before it opens a read
    table, fq = tmp_path / "amplicons.txt", tmp_path / "r1.fq"
    table.write_text("a\t%s\nwith_hdr\t%s\t\t%s\n" % (rows[0]["Amplicon_Sequence"], rows[1]["Amplicon_Sequence"],
                                                       rows[1]["Expected_HDR"]))
    fq.write_text("")
    with pytest.raises(SystemExit):
        demux.main(["-f", str(table), "-r1", str(fq), "-o", str(tmp_path / "out"), "--summary"])
    assert "dual alignment per amplicon is not built" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "out")


# ---- the ABI -----------------------------------------------------------------------------------

def test_headers_bindings_and_library_agree():
    assert declared_symbols("crispr_summary.h", "nws_") == set(_lib.SUMMARY_EXPORTS)
    assert declared_symbols("crispr_demux.h", "nwd_") == set(_lib.DEMUX_EXPORTS)
    assert declared_symbols("crispr_front.h", "nwp_") == set(_lib.FRONT_EXPORTS)
    assert "nwd_assign_prepared" in _lib.DEMUX_EXPORTS
    exported = _lib.exported_symbols()
    for name in _lib.SUMMARY_EXPORTS + _lib.DEMUX_EXPORTS + _lib.FRONT_EXPORTS:
        assert exported[name], name
    lib = _lib.load()
    assert lib.nws_flags.argtypes is not None and lib.nwd_assign_prepared.argtypes is not None


def test_slot_names_follow_the_header():
    text = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "crispr_summary.h")).read()
    order = [name for name in ("NWS_N", "NWS_TOTAL", "NWS_UNMODIFIED", "NWS_MODIFIED", "NWS_REPAIRED", "NWS_MIXED",
                               "NWS_NHEJ_INSERTED", "NWS_NHEJ_DELETED", "NWS_NHEJ_MUTATED", "NWS_HDR_INSERTED",
                               "NWS_HDR_DELETED", "NWS_HDR_MUTATED", "NWS_MIXED_INSERTED", "NWS_MIXED_DELETED",
                               "NWS_MIXED_MUTATED", "NWS_NOT_ALIGNED", "NWS_SLOTS")]
    for k, name in enumerate(order):
        assert "%s = %d" % (name, k) in text, name
