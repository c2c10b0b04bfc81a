"""crispresso_amd/report.py without a GPU: the four histogram tables from the histograms against
quantify.run_summary on the DataFrame of the same reads, every file of write_report byte for byte
against the restatement in tests/report_model.py, the files read back the way CRISPRessoCompare and
CRISPRessoPooled read them, and the refusal of a report without a kept read."""
import os

import numpy as np
import pytest
from pandas.testing import assert_frame_equal

from crispresso_amd import demux, quantify, report
from tests import report_model as rm

AMP = ("ACGTTGCA" * 30)[:201]          # 201 bases: odd
TABLES = ("df_indels", "df_insertion", "df_deletion", "df_substitution")


def reads(n_ins, n_del=None, n_mut=None, cls=None):
    """(cls, n_mutated, n_inserted, n_deleted) of len(n_ins) kept reads; NHEJ where a size is > 0."""
    n_ins = np.asarray(n_ins, np.int64)
    n_del = np.zeros_like(n_ins) if n_del is None else np.asarray(n_del, np.int64)
    n_mut = np.zeros_like(n_ins) if n_mut is None else np.asarray(n_mut, np.int64)
    if cls is None:
        cls = ((n_ins > 0) | (n_del > 0) | (n_mut > 0)).astype(np.int32)
    return np.asarray(cls), n_mut, n_ins, n_del


def both(amp, cuts, rd, bins=None):
    """(tables(report), run_summary) of the same kept reads."""
    rep = rm.report_of("x", amp, cuts, *rd, totals=rm.synthetic_totals(len(amp), 1), bins=bins)
    want = quantify.run_summary(rm.kept_frame(*rd), len(amp), cuts)
    return report.tables(rep), want


def check(got, want):
    assert sorted(got) == sorted(TABLES)
    for key in TABLES:
        assert_frame_equal(got[key], want[key])


def test_no_non_zero_value_gives_the_range_15():
    got, want = both(AMP, [100], reads(np.zeros(40, np.int64)))
    check(got, want)
    for key in TABLES[1:]:
        assert len(got[key]) == 14 and got[key]["fq"].tolist() == [40] + [0] * 13
    assert got["df_indels"]["fq"].sum() == 40


def test_the_last_bin_is_closed_and_the_value_beyond_it_is_dropped():
    """Range 15: bins 0 .. 14, the last row is labelled 13 and also counts the 14s; a 15 is in no row."""
    sizes = np.array([1] * 296 + [13, 14, 14, 15])
    for rd in (reads(sizes), reads(np.zeros(300, np.int64), sizes), reads(np.zeros(300, np.int64), None, sizes)):
        got, want = both(AMP, [100], rd)
        check(got, want)
    got, _ = both(AMP, [100], reads(sizes))
    assert got["df_insertion"]["ins_size"].tolist() == list(range(14))
    assert got["df_insertion"]["fq"].tolist() == [0, 296] + [0] * 11 + [3]
    got, _ = both(AMP, [100], reads(np.zeros(300, np.int64), sizes))
    assert got["df_deletion"]["del_size"].tolist() == [-k for k in range(14)] and got["df_deletion"]["fq"].iloc[-1] == 3


@pytest.mark.parametrize("top", [(20, 30), (20, 70), (21, 71), (40, 41)])
def test_the_99th_percentile_is_interpolated_between_two_integers(top):
    """200 non-zero values: the 99th percentile lies at position 197.01 of the sorted values,
    between top[0] and top[1]; 20 .. 70 and 21 .. 71 land within 1e-12 of x.5."""
    sizes = np.array([0] * 25 + [2] * 197 + [top[0], top[1], 90])
    assert (sizes > 0).sum() == 200
    p = np.percentile(sizes[sizes > 0], 99)
    assert top[0] < p < top[1]
    for rd in (reads(sizes), reads(np.zeros_like(sizes), sizes), reads(np.zeros_like(sizes), None, sizes)):
        got, want = both(AMP, [], rd)
        check(got, want)
    got, _ = both(AMP, [], reads(sizes))
    assert len(got["df_insertion"]) == max(15, int(np.round(p))) - 1 > 14


@pytest.mark.parametrize("low, rows", [(20, 19), (21, 21)])
def test_a_percentile_of_exactly_one_half_rounds_to_even(low, rows):
    """51 non-zero values: position 49.5, halfway between low and low + 1; 20.5 rounds to 20, 21.5 to 22."""
    sizes = np.array([3] * 49 + [low, low + 1] + [0] * 9)
    assert np.percentile(sizes[sizes > 0], 99) == low + 0.5
    got, want = both(AMP, [], reads(sizes, sizes[::-1].copy(), sizes))
    check(got, want)
    assert [len(got[k]) for k in TABLES[1:]] == [rows] * 3


@pytest.mark.parametrize("cuts", [[0], [len(AMP) - 1], [0, 100], [100, len(AMP) - 1], [37, 150]])
def test_cut_points_at_the_ends(cuts):
    rng = np.random.Generator(np.random.PCG64(5))
    n = 400
    rd = reads(rng.integers(0, 60, n) * (rng.random(n) < 0.5), rng.integers(0, 200, n) * (rng.random(n) < 0.5),
               rng.integers(0, 9, n))
    got, want = both(AMP, cuts, rd)
    check(got, want)
    assert got["df_indels"]["indel_size"].tolist() == list(range(-min(cuts), len(AMP) - max(cuts) - 1))


@pytest.mark.parametrize("L", [201, 200, 31])
def test_without_a_guide_the_indel_table_spans_half_the_amplicon_each_side(L):
    rng = np.random.Generator(np.random.PCG64(L))
    n = 300
    rd = reads(rng.integers(0, L, n) * (rng.random(n) < 0.4), rng.integers(0, L, n) * (rng.random(n) < 0.4),
               rng.integers(0, 5, n))
    got, want = both(AMP[:L], [], rd)
    check(got, want)
    assert got["df_indels"]["indel_size"].tolist() == list(range(-(L // 2), L // 2 - 1))
    # more bins than the sizes need change nothing
    wide, _ = both(AMP[:L], [], rd, bins=2 * L + 7)
    check(wide, want)


# ---- write_report ------------------------------------------------------------------------------

def panel(kind):
    rng = np.random.Generator(np.random.PCG64(11))
    n = 500
    cls = rng.integers(0, 4 if kind == "hdr" else 2, n).astype(np.int32)
    mod = cls > 0
    rd = (cls, rng.integers(0, 6, n) * mod, rng.integers(0, 40, n) * mod * (rng.random(n) < 0.5),
          rng.integers(0, 80, n) * mod * (rng.random(n) < 0.5))
    totals = rm.synthetic_totals(len(AMP), 3, coding=kind == "coding", hdr=kind == "hdr")
    cuts = [] if kind == "plain" else [96]
    rep = rm.report_of("AMP (%s)/1" % kind, AMP, cuts, *rd, totals=totals, n_reads=n + 17, coding=kind == "coding",
                       hdr=kind == "hdr")
    return rep, quantify.run_summary(rm.kept_frame(*rd), len(AMP), cuts)


@pytest.mark.parametrize("kind", ["plain", "coding", "hdr"])
def test_write_report_byte_for_byte(tmp_path, kind):
    rep, summary = panel(kind)
    folder = str(tmp_path / report.folder_name(rep.name))
    written = report.write_report(folder, rep)
    want = rm.expected_files(rep, summary)
    assert sorted(os.listdir(folder)) == sorted(want) == sorted(written)
    for name, body in want.items():
        with open(os.path.join(folder, name), "rb") as f:
            assert f.read() == body, name
    assert ("effect_vector_insertion_HDR.txt" in want) == (kind == "hdr")
    assert ("Frameshift_analysis.txt" in want) == ("effect_vector_substitution_noncoding.txt" in want) == (kind == "coding")
    assert len(want) == {"plain": 12, "coding": 17, "hdr": 18}[kind]
    # the folder's name is what the reference derives from the amplicon's name
    assert os.path.basename(folder) == "CRISPResso_on_" + demux.clean_filename(rep.name) == "CRISPResso_on_AMP (%s)1" % kind
    # the averages met both 0 / 0 and x / 0
    v = rep.totals["vectors"]
    den = v["effect_vector_insertion"] + v["effect_vector_insertion_hdr"] + v["effect_vector_insertion_mixed"]
    assert (den == 0).any() and ((den == 0) & (v["avg_vector_ins_all"] > 0)).any()
    avg = np.loadtxt(os.path.join(folder, "position_dependent_vector_avg_insertion_size.txt"), skiprows=1)[:, 1]
    assert np.isfinite(avg).all() and (avg[den == 0] == 0).all() and (avg[den > 0] == (v["avg_vector_ins_all"] / np.maximum(den, 1))[den > 0]).all()


@pytest.mark.parametrize("kind", ["plain", "hdr"])
def test_the_files_as_their_readers_read_them(tmp_path, kind):
    rep, _ = panel(kind)
    folder = str(tmp_path / "out")
    report.write_report(folder, rep)
    # CRISPRessoCompare: np.loadtxt(..., skiprows=1) of the combined vector
    combined = np.loadtxt(os.path.join(folder, "effect_vector_combined.txt"), skiprows=1)
    assert combined.shape == (len(AMP), 2) and combined[:, 0].tolist() == list(range(1, len(AMP) + 1))
    assert np.array_equal(combined[:, 1], 100.0 * rep.totals["vectors"]["effect_vector_any"] / float(rep.n_total))
    # CRISPRessoPooled's summary: the integers after the labels, line by line
    got = rm.read_quantification(os.path.join(folder, "Quantification_of_editing_frequency.txt"))
    assert got == rep.slots[1:6].tolist() and got[0] == 500
    if kind == "hdr":
        assert got[3] > 0 and got[4] > 0


def test_a_report_without_a_kept_read_is_refused(tmp_path):
    rep, _ = panel("plain")
    rep.slots = np.zeros(16, np.int64)
    rep.slots[0] = 40
    folder = str(tmp_path / "none")
    with pytest.raises(report.ReportError, match="zero sequences aligned"):
        report.write_report(folder, rep)
    assert not os.path.exists(folder)


def test_reports_without_the_summary_is_a_usage_error(tmp_path, capsys):
    table, fq = tmp_path / "a.txt", tmp_path / "r.fq"
    table.write_text("A\tACGTACGTACGTACGTACGT\n")
    fq.write_text("@r\nACGT\n+\nIIII\n")
    with pytest.raises(SystemExit) as exc:
        demux.main(["-f", str(table), "-r1", str(fq), "-o", str(tmp_path / "o"), "--reports"])
    assert exc.value.code == 2 and "--reports is used only with --summary" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "o")
