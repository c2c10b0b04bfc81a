"""The host side of the Expected_HDR rows of the pooled and WGS summaries: the printed identity in
tenths by integers (crispresso_amd.demux.printed_tables, tests/hdr_summary_model.py) against
aligner.printed_percent, the integer thresholds, the dual-flag model against quantify.pre_flags
and the reference's keep expression on printed floats, the row checks, both command lines'
options, the ABI, and the choice of the GPU tests' panel held on the CPU oracles."""
import os

import numpy as np
import pytest

from crispresso_amd import _lib, demux, regions
from crispresso_amd.aligner import printed_percent
from tests import demux_model as dm
from tests import hdr_summary_model as hm
from tests.test_abi import declared_symbols

LONG = (1999, 2000, 2001, 4000, 12288)


@pytest.fixture(scope="module")
def tie_up():
    return demux.printed_tables(60.0, 98.0)[0]


# ---- the printed identity in tenths ------------------------------------------------------------

def test_tenths_equal_the_printed_identity(tie_up):
    assert tie_up.dtype == np.uint8 and tie_up.shape == (1000,) and int(tie_up.sum()) == 500
    ties = 0
    for L in list(range(601)) + list(LONG):
        for n in range(L + 1):
            assert hm.tenths(n, L, tie_up) / 10.0 == printed_percent(n, L), (n, L)
            ties += L > 0 and 2 * (1000 * n % L) == L
    assert ties > 1000          # midpoints are met, at many lengths


def test_every_table_entry_is_a_midpoint_of_2000(tie_up):
    for t in range(1000):
        want = printed_percent(2 * t + 1, 2000)
        assert want in (t / 10.0, (t + 1) / 10.0)
        assert hm.tenths(2 * t + 1, 2000, tie_up) == t + int(tie_up[t]) == round(want * 10)
        # the same midpoint from other pairs: the double is the same, and so is what it prints
        for n, L in ((6 * t + 3, 6000), (14 * t + 7, 14000)):
            assert 100.0 * n / L == 100.0 * (2 * t + 1) / 2000 and hm.tenths(n, L, tie_up) == t + int(tie_up[t])


def test_a_printed_value_is_its_tenths_over_ten():
    for t in range(1001):
        assert float("%.1f" % (t / 10.0)) == t / 10.0
        assert "%.1f" % (t / 10.0) == "%d.%d" % divmod(t, 10)


@pytest.mark.parametrize("score", [0, 59.95, 60, 60.05, 98, 99.9, 100, 101])
def test_thresholds_in_tenths(score):
    _, keep_tenths, hdr_tenths = demux.printed_tables(score, score)
    assert 0 <= keep_tenths <= 1001 and 0 <= hdr_tenths <= 1001
    for t in range(1001):
        assert (t >= keep_tenths) == (t / 10.0 > score), t
        assert (t >= hdr_tenths) == (t / 10.0 >= score), t
    want = {0: (1, 0), 59.95: (600, 600), 60: (601, 600), 60.05: (601, 601), 98: (981, 980), 99.9: (1000, 999),
            100: (1001, 1000), 101: (1001, 1001)}[score]
    assert (keep_tenths, hdr_tenths) == want


# ---- the dual flags ----------------------------------------------------------------------------

def test_dual_flags_equal_the_reference_rule_on_printed_floats(tie_up):
    rng = np.random.Generator(np.random.PCG64(11))
    n = 4000
    La, Lh = rng.integers(1, 700, n), rng.integers(1, 700, n)
    na = (La * rng.uniform(0.4, 1.0, n)).astype(np.int64)
    nh = (Lh * rng.uniform(0.4, 1.0, n)).astype(np.int64)
    exact = rng.random(n) < 0.15
    na[exact] = La[exact]
    near = rng.random(n) < 0.3                  # the repaired identity close to the ref identity and to 98
    nh[near] = np.minimum(Lh[near], (Lh[near] * na[near]) // La[near] + rng.integers(-1, 2, near.sum()))
    nh = np.maximum(nh, 0)
    flags = (rng.random(n) < 0.05).astype(np.int32)
    for score, threshold in ((60.0, 98.0), (59.95, 97.95), (0.0, 100.0), (100.0, 60.0)):
        _, keep_tenths, hdr_tenths = demux.printed_tables(score, threshold)
        rep, bad = hm.printed(Lh, nh, np.zeros(n, np.int32), tie_up)
        assert bad == 0
        pre, keep, bad = hm.flags_dual(La, na, flags, rep, tie_up, keep_tenths, hdr_tenths)
        sr = [printed_percent(int(a), int(b)) for a, b in zip(na, La)]
        sp = [printed_percent(int(a), int(b)) for a, b in zip(nh, Lh)]
        kept, want_pre = hm.reference_rule(sr, sp, score, threshold)
        assert bad == 0 and np.array_equal(pre, want_pre)
        assert np.array_equal(keep.astype(bool), kept & (flags == 0))
    assert (pre & _lib.NWQ_PRE_HDR).any() and (pre & _lib.NWQ_PRE_MIXED).any() and (pre & 1).any()
    assert not ((pre & _lib.NWQ_PRE_HDR) != 0)[(pre & _lib.NWQ_PRE_MIXED) != 0].any()


def test_dual_flags_without_a_repaired_score(tie_up):
    """0xFFFF compares false throughout, as the NaN of quantify.pre_flags; other values above
    1000 and records out of range are counted."""
    _, keep_tenths, hdr_tenths = demux.printed_tables(60.0, 98.0)
    L, n, f = [100, 100, 100, 100, -1, 10], [100, 50, 90, 90, 0, 11], [0, 0, 0, 0, 0, 0]
    pre, keep, bad = hm.flags_dual(L, n, f, [0xFFFF, 0xFFFF, 0xFFFF, 1001, 500, 500], tie_up, keep_tenths, hdr_tenths)
    assert pre.tolist() == [1, 0, 0, 0, 0, 0] and keep.tolist() == [1, 0, 1, 0, 0, 0] and bad == 3
    got, bad = hm.printed([0, 10, 10, hm.MAX_COLS + 1, 10], [0, 5, 5, 1, 11], [0, 0, 1, 0, 0], tie_up)
    assert got.tolist() == [0, 500, 0xFFFF, 0xFFFF, 0xFFFF] and bad == 2


# ---- the rows ----------------------------------------------------------------------------------

ROW = {"Name": "a", "Amplicon_Sequence": "ACGT" * 30, "sgRNA": "", "Expected_HDR": "", "Coding_sequence": ""}


def test_row_checks_with_allow_hdr():
    good = dict(ROW, Name="with_hdr", Expected_HDR="  acgt" + "ACGT" * 28 + "ACGA \n")
    assert demux.check_summary_rows([ROW, good], allow_hdr=True) == [ROW["Amplicon_Sequence"]] * 2
    assert demux.checked_expected_hdr(good, good["Amplicon_Sequence"]) == "ACGT" * 29 + "ACGA"
    assert demux.checked_expected_hdr(ROW, ROW["Amplicon_Sequence"]) is None
    for hdr, message in ((ROW["Amplicon_Sequence"].lower(), "with_hdr.*cannot be the same"),
                         ("ACGT" * 29 + "ACGU", "with_hdr.*wrong characters:U"),
                         ("ACGT" * 2048 + "A", "with_hdr.*8193 bases")):
        bad = dict(good, Expected_HDR=hdr)
        with pytest.raises(ValueError, match=message):
            demux.check_summary_rows([ROW, bad], allow_hdr=True)
        with pytest.raises(ValueError, match=message):
            demux.summarize_pooled([ROW, bad], ([], []), aligner=None, allow_hdr=True)
        with pytest.raises(ValueError, match="region " + message):
            demux.checked_expected_hdr(bad, bad["Amplicon_Sequence"], "region")
    # 8192 bases are taken
    assert len(demux.checked_expected_hdr(dict(good, Expected_HDR="ACGT" * 2048), "ACGT")) == 8192
    # and without the switch the refusal is the old one, word for word
    for call in (lambda: demux.check_summary_rows([ROW, good]), lambda: demux.check_summary_rows([ROW, good], False),
                 lambda: demux.summarize_pooled([ROW, good], ([], []), aligner=None)):
        with pytest.raises(ValueError) as exc:
            call()
        assert str(exc.value) == "amplicon with_hdr: Expected_HDR is given, and dual alignment per amplicon is not built"
    long_row = dict(good, Name="long", Amplicon_Sequence="ACGT" * 8192)
    with pytest.raises(ValueError, match="long has 32768 bases"):
        demux.check_summary_rows([long_row], allow_hdr=True)


# ---- the command lines -------------------------------------------------------------------------

def parse(*argv):
    p = demux.build_parser()
    return demux.options_from_args(p, p.parse_args(["-f", "a.txt", "-r1", "r1.fq", "-o", "out", *argv]))


def test_demux_command_line_options():
    old = dict(min_identity_score=60.0, window_around_sgrna=1, cleavage_offset=-3)
    assert parse() == dict(k=16, min_hits=2, both_strands=True, min_reads_to_use_region=1000)
    assert parse("--summary") == dict(k=16, min_hits=2, both_strands=True, min_reads_to_use_region=1000, summary=old)
    assert parse("--summary", "--hdr")["summary"] == dict(old, allow_hdr=True, hdr_perfect_alignment_threshold=98.0)
    kw = parse("-r2", "r2.fq", "--summary", "--min_identity_score", "70", "--hdr", "--hdr_perfect_alignment_threshold", "95.5")
    assert kw["summary"] == dict(min_identity_score=70.0, window_around_sgrna=1, cleavage_offset=-3, allow_hdr=True,
                                 hdr_perfect_alignment_threshold=95.5)
    for bad in (["--hdr"], ["--summary", "--hdr_perfect_alignment_threshold", "98.0"],
                ["--hdr_perfect_alignment_threshold", "97"]):
        with pytest.raises(SystemExit):
            parse(*bad)
    # every key of the summary options is a keyword of summarize_pooled
    import inspect

    assert set(kw["summary"]) <= set(inspect.signature(demux.summarize_pooled).parameters)


def test_demux_command_line_refuses_a_bad_row_before_it_opens_a_read(tmp_path, capsys):
    amp = ROW["Amplicon_Sequence"]
    table, fq = tmp_path / "amplicons.txt", tmp_path / "r1.fq"
    table.write_text("a\t%s\nsame\t%s\t\t%s\n" % (amp, "TTGCA" * 30, "ttgca" * 30))
    fq.write_text("")
    with pytest.raises(SystemExit):
        demux.main(["-f", str(table), "-r1", str(fq), "-o", str(tmp_path / "out"), "--summary", "--hdr"])
    assert "same" in capsys.readouterr().err and not os.path.exists(tmp_path / "out")


def region_options(*argv):
    p = regions.build_parser()
    return regions.summary_options(p, p.parse_args(["--bam", "x.bam", "--regions", "r.txt", "--out", "out", *argv]))


def test_regions_command_line_options():
    import inspect

    assert region_options() == {} and region_options("--summary", "--genome", "g.fa") == {}
    assert region_options("--summary", "--hdr") == dict(allow_hdr=True, hdr_perfect_alignment_threshold=98.0)
    got = region_options("--summary", "--hdr", "--hdr_perfect_alignment_threshold", "90")
    assert got == dict(allow_hdr=True, hdr_perfect_alignment_threshold=90.0)
    assert set(got) <= set(inspect.signature(regions.summarize_regions).parameters)
    for bad in (["--hdr"], ["--summary", "--hdr_perfect_alignment_threshold", "98"]):
        with pytest.raises(SystemExit):
            region_options(*bad)


def test_regions_main_refuses_hdr_without_summary(tmp_path, capsys):
    with pytest.raises(SystemExit):
        regions.main(["--bam", str(tmp_path / "x.bam"), "--by-reference", "--out", str(tmp_path / "o"), "--hdr"])
    assert "--hdr is used only with --summary" in capsys.readouterr().err


# ---- the ABI -----------------------------------------------------------------------------------

def test_the_new_symbols():
    new = {"nws_set_printed", "nws_printed", "nws_flags_dual"}
    assert new <= set(_lib.SUMMARY_EXPORTS) == declared_symbols("crispr_summary.h", "nws_")
    exported = _lib.exported_symbols()
    lib = _lib.load()
    for name in new:
        assert exported[name], name
        assert getattr(lib, name).argtypes is not None
    assert _lib.NWS_NO_TENTHS == hm.NO_TENTHS == 0xFFFF and demux.MAX_ALIGNER_REFERENCE == 8192


# ---- the panel of the GPU tests, held before any GPU call --------------------------------------

def test_the_panel_is_assigned_and_covers_every_class():
    rows, reads, origin = hm.panel()
    want = dm.demultiplex([r["Amplicon_Sequence"].encode() for r in rows], reads)
    assert want["which"] == origin and min(want["counts"]) > 5          # no tie, no read without a hit
    assert sum(1 for s in want["strand"] if s) == len(reads) // 2
    assert len(rows[1]["Expected_HDR"]) == 206 and rows[2]["sgRNA"] in rows[2]["Amplicon_Sequence"]
    for g, row in enumerate(rows):
        s, sr, sp = hm.oracle_slots(row, want["groups"][g])
        pairs = set(zip(sr.tolist(), sp.tolist()))
        if g == 3:
            assert s[4] == s[5] == 0 and s[1] == s[0] and s[2] > 0 and s[3] > 0
            continue
        assert s[4] > 0 and s[5] > 0 and s[2] > 0 and s[3] > 0 and s[15] == 0 and s[0] - s[1] >= 2, (g, s)
        assert any(a <= 60.0 < b for a, b in pairs)             # kept by the repaired score alone
        assert any(a <= 60.0 and b <= 60.0 for a, b in pairs)   # dropped by both
        assert any(a < b and b >= 98.0 and b < 100.0 for a, b in pairs) and any(a < b < 98.0 and a > 60.0 for a, b in pairs)
        if g != 1:
            assert (95.0, 95.0) in pairs and any(b == 98.0 for a, b in pairs) and any(b == 97.5 for a, b in pairs)
            assert any(b == 60.5 and a < 60.0 for a, b in pairs)


def test_the_region_case_covers_every_class(tmp_path):
    bam_path, table, fasta = hm.write_region_inputs(tmp_path)
    rows = regions.wgs_rows(regions.read_wgs_region_file(table), fasta)
    _, _, _, raw = hm.region_case()
    assert [r["Name"] for r in rows] == ["hdr_region_0", "hdr_region_1"]
    assert rows[0]["Expected_HDR"] == raw[0]["Expected_HDR"] and rows[1]["Expected_HDR"] == ""
    assert [len(r["Amplicon_Sequence"]) for r in rows] == list(hm.REGION_SIZES)
    reads = hm.region_model_reads()
    assert [len(r) for r in reads] == list(hm.REGION_RECORDS)
    s, sr, sp = hm.oracle_slots(rows[0], reads[0])
    assert s[0] == 24 and s[1] == 20 and min(s[2:6]) > 0 and s[15] == 0
    assert 98.1 in sp.tolist() and 96.9 in sp.tolist()
    s, _, _ = hm.oracle_slots(rows[1], reads[1])
    assert s[0] == 20 and s[1] == 15 and s[2] > 0 and s[3] > 0 and s[4] == s[5] == 0
