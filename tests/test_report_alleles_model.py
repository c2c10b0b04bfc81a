"""The allele tables of a result folder without a GPU (crispresso_amd/report.py): write_report with
``alleles`` / ``around_cut`` set writes Alleles_frequency_table.txt and one
Alleles_frequency_table_around_cut_site_for_<sgRNA>.txt per pair of zip(guides, cut_points), byte
for byte as the reference's to_csv calls (CRISPRessoCORE.py:3835, 3643-3654); with both None the
folder is what it was; and the callers refuse ``alleles`` without ``reports``."""
import io
import os

import numpy as np
import pandas as pd
import pytest
from pandas.testing import assert_frame_equal

from crispresso_amd import alleles, demux, quantify, regions, report
from tests import report_model as rm
from tests.test_report_model import panel

GUIDE_A, GUIDE_B = "ACGTTGCAACGGTCATGCAT", "TTGACCGATAGGCTAACCGT"
FILL = "GATTACAGGCTTAACCGGTATCGGATCCAT"
ALLELE_HEADER = "Aligned_Sequence\tReference_Sequence\tNHEJ\tUNMODIFIED\tHDR\tn_deleted\tn_inserted\tn_mutated\t#Reads\t%Reads\n"
AROUND_HEADER = "Aligned_Sequence\tReference_Sequence\tUnedited\t%Reads\t#Reads\n"


def allele_frame(amp):
    """A df_alleles of five alleles of amp: unedited, a substitution, a deletion and an insertion
    near the middle, and two alleles with equal counts (a tie the sort has to keep)."""
    m = len(amp) // 2
    sub = amp[:m] + ("A" if amp[m] != "A" else "C") + amp[m + 1:]
    rows = [(amp, amp, 0, 0, 0, 0, 40), (sub, amp, 1, 0, 0, 1, 7), (amp[:m] + "---" + amp[m + 3:], amp, 1, 3, 0, 0, 7),
            (amp[:m] + "GG" + amp[m:], amp[:m] + "--" + amp[m:], 1, 0, 2, 0, 3),
            (amp[:5] + "T" + amp[6:] if amp[5] != "T" else amp[:5] + "G" + amp[6:], amp, 1, 0, 0, 1, 1)]
    frame = pd.DataFrame({
        "Aligned_Sequence": [r[0] for r in rows], "Reference_Sequence": [r[1] for r in rows],
        "NHEJ": [r[2] == 1 for r in rows], "UNMODIFIED": [r[2] == 0 for r in rows], "HDR": [False] * len(rows),
        "n_deleted": np.array([r[3] for r in rows], np.int64), "n_inserted": np.array([r[4] for r in rows], np.int64),
        "n_mutated": np.array([r[5] for r in rows], np.int64), "#Reads": np.array([r[6] for r in rows], np.int64)})
    return alleles.merge_allele_tables([frame])


def with_tables(amp, guide_seq, offset=20):
    rep, summary = panel("plain")
    rep.amplicon = amp
    cuts = quantify.compute_cut_points(amp, guide_seq)
    rep.cut_points = cuts
    table = allele_frame(amp)
    table["ref_positions"] = [alleles.ref_positions(r) for r in table["Reference_Sequence"]]   # (cut off by :"%Reads")
    rep.alleles = table
    pairs = report.guide_cut_pairs(guide_seq, cuts)
    rep.around_cut = [(sg, c, alleles.around_cut_from_alleles(table, c, offset)) for sg, c in pairs]
    return rep, report.tables(rep), cuts, pairs      # (the histogram tables of the new amplicon and cut points)


def allele_bytes(table) -> bytes:
    buf = io.StringIO()
    table.loc[:, :"%Reads"].to_csv(buf, sep="\t", header=True, index=None)
    return buf.getvalue().encode()


def around_bytes(frame) -> bytes:
    buf = io.StringIO()
    frame.to_csv(buf, sep="\t", header=True)
    return buf.getvalue().encode()


def read_folder(folder):
    out = {}
    for name in os.listdir(folder):
        with open(os.path.join(folder, name), "rb") as f:
            out[name] = f.read()
    return out


def test_two_guides_write_the_allele_table_and_a_file_each(tmp_path):
    amp = FILL + GUIDE_A + FILL[::-1] + GUIDE_B + FILL
    rep, summary, cuts, pairs = with_tables(amp, GUIDE_A.lower() + "," + GUIDE_B)
    assert len(cuts) == 2 and pairs == [(GUIDE_A, cuts[0]), (GUIDE_B, cuts[1])]
    folder = str(tmp_path / "two")
    written = report.write_report(folder, rep)
    got = read_folder(folder)
    want = rm.expected_files(rep, summary)
    want[report.ALLELES_FILE] = allele_bytes(rep.alleles)
    for sg, _, frame in rep.around_cut:
        want["Alleles_frequency_table_around_cut_site_for_%s.txt" % sg] = around_bytes(frame)
    assert sorted(got) == sorted(want) == sorted(written) and len(want) == 12 + 3
    for name, body in want.items():
        assert got[name] == body, name
    text = got["Alleles_frequency_table.txt"].decode()
    assert text.startswith(ALLELE_HEADER) and "ref_positions" not in text and text.count("\n") == 1 + len(rep.alleles)
    first = text.split("\n")[1].split("\t")
    assert first[:2] == [amp, amp] and first[2:5] == ["False", "True", "False"] and first[8] == "40"
    assert float(first[9]) == 40 / 58 * 100.0
    for sg, c, frame in rep.around_cut:
        body = got["Alleles_frequency_table_around_cut_site_for_%s.txt" % sg].decode()
        assert body.startswith(AROUND_HEADER)
        assert body.split("\n")[1].split("\t")[:3] == [amp[c - 19:c + 21], amp[c - 19:c + 21], "True"]
        back = pd.read_csv(io.StringIO(body), sep="\t").set_index("Aligned_Sequence")
        assert_frame_equal(back, frame)
    back = pd.read_csv(io.StringIO(text), sep="\t")
    assert_frame_equal(back, rep.alleles.loc[:, :"%Reads"].reset_index(drop=True))


def test_one_guide_with_two_matches_writes_the_file_of_its_first_cut_point(tmp_path):
    """zip(guides, cut_points) ends with the shorter list: the second match has no file."""
    amp = FILL + GUIDE_A + FILL[::-1] + GUIDE_A + FILL
    rep, summary, cuts, pairs = with_tables(amp, GUIDE_A)
    assert len(cuts) == 2 and pairs == [(GUIDE_A, cuts[0])]
    folder = str(tmp_path / "twice")
    written = report.write_report(folder, rep)
    got = read_folder(folder)
    name = "Alleles_frequency_table_around_cut_site_for_%s.txt" % GUIDE_A
    assert sorted(got) == sorted(written) == sorted(list(rm.expected_files(rep, summary)) + [report.ALLELES_FILE, name])
    assert got[name] == around_bytes(alleles.around_cut_from_alleles(rep.alleles, cuts[0], 20))
    assert got[name] != around_bytes(alleles.around_cut_from_alleles(rep.alleles, cuts[1], 20))
    assert got[report.ALLELES_FILE] == allele_bytes(rep.alleles)


def test_without_a_guide_only_the_allele_table_is_added(tmp_path):
    amp = FILL + GUIDE_A + FILL
    rep, summary, cuts, pairs = with_tables(amp, None)
    assert cuts == [] and pairs == [] and rep.around_cut == []
    folder = str(tmp_path / "none")
    written = report.write_report(folder, rep)
    got = read_folder(folder)
    assert sorted(got) == sorted(written) == sorted(list(rm.expected_files(rep, summary)) + [report.ALLELES_FILE])
    assert got[report.ALLELES_FILE] == allele_bytes(rep.alleles)
    # the around-cut tables alone, without the allele table
    rep2, _, cuts2, _ = with_tables(amp, GUIDE_A)
    rep2.alleles = None
    written2 = report.write_report(str(tmp_path / "around"), rep2)
    assert report.ALLELES_FILE not in written2 and report.around_cut_file(GUIDE_A) in written2


@pytest.mark.parametrize("kind", ["plain", "coding", "hdr"])
def test_with_both_none_the_folder_is_todays(tmp_path, kind):
    rep, summary = panel(kind)
    assert rep.alleles is None and rep.around_cut is None
    folder = str(tmp_path / "plain")
    written = report.write_report(folder, rep)
    want = rm.expected_files(rep, summary)
    assert sorted(written) == sorted(want) and read_folder(folder) == want
    assert len(want) == {"plain": 12, "coding": 17, "hdr": 18}[kind]


def test_guide_cut_pairs():
    assert report.guide_cut_pairs(None, []) == [] and report.guide_cut_pairs("", [3]) == []
    assert report.guide_cut_pairs(" acgt,GGCC ", [5, 9, 11]) == [("ACGT", 5), ("GGCC", 9)]
    assert report.guide_cut_pairs("ACGT,GGCC", [5]) == [("ACGT", 5)]


def test_alleles_without_reports_is_refused(tmp_path, capsys):
    table, fq = tmp_path / "a.txt", tmp_path / "r.fq"
    table.write_text("A\tACGTACGTACGTACGTACGT\n")
    fq.write_text("@r\nACGT\n+\nIIII\n")
    for extra in ([], ["--summary"]):
        with pytest.raises(SystemExit) as exc:
            demux.main(["-f", str(table), "-r1", str(fq), "-o", str(tmp_path / "o"), "--alleles"] + extra)
        assert exc.value.code == 2 and "--alleles is used only with --reports" in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        demux.main(["-f", str(table), "-r1", str(fq), "-o", str(tmp_path / "o"), "--summary", "--reports",
                    "--offset_around_cut_to_plot", "10"])
    assert exc.value.code == 2 and "--offset_around_cut_to_plot is used only with --alleles" in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        regions.main(["--bam", str(tmp_path / "x.bam"), "--regions", str(table), "--genome", str(table), "--summary",
                      "--out", str(tmp_path / "o"), "--alleles"])
    assert exc.value.code == 2 and "--alleles is used only with --reports" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "o")
    rows = [{"Name": "A", "Amplicon_Sequence": "ACGTACGTACGTACGTACGT", "sgRNA": "", "Coding_sequence": ""}]
    with pytest.raises(ValueError, match="pass reports as well"):
        demux.summarize_pooled(rows, [b"ACGT"], None, alleles=True)
    with pytest.raises(ValueError, match="pass reports as well"):
        regions.summarize_regions(rows, None, None, alleles=True)
    with pytest.raises(ValueError, match="pass reports as well"):
        demux.demultiplex_fastq(str(table), str(fq), str(tmp_path / "o"), summary={}, alleles=True)
    with pytest.raises(ValueError, match="pass reports as well"):
        demux._summarize_groups(rows, ["ACGT"], [], 0, None, None, None, None, None, "amplicon", 60.0, {}, None,
                                alleles=True)
    assert not os.path.exists(tmp_path / "o")
