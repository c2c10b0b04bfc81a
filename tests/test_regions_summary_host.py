"""The host side of the WGS / genome-mode summary (crispresso_amd/regions.py): the reference's
seven-column region file, the rows built from a FASTA with the reference's sgRNA rules
(CRISPRessoWGSCORE.py:613-641), and the command line's refusals.  No GPU."""
import pytest

from crispresso_amd import regions

CHR1 = ("acgtacgtagGATTACAGATTACACCCGGGTTTAAACCCGGGTATATATATCGCGCGATCGATCGGCTAGCTAGCATCGATCAGCTACGACTACGACGAGCGAGC"
        "ttttggggccccaaaa")          # 121 bases, lower case at both ends


def write_fasta(tmp_path):
    path = tmp_path / "genome.fa"
    lines = [">chr1 test"] + [CHR1[i:i + 50] for i in range(0, len(CHR1), 50)] + [">chr2", "ACGT" * 10]
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_read_wgs_region_file(tmp_path):
    path = tmp_path / "regions.txt"
    path.write_text("# a comment\n"
                    "chr1\t11\t61\n"
                    "chr1\t11\t61\tfour\n"
                    "chr1\t20\t70\tfive guides\tgattaca,ACGT\n"
                    "chr1\t20\t70\tsix\tGATTACA\tacgt\n"
                    "chr2\t1\t30\tseven\t\t\tacgtac  # trailing comment\n"
                    "\n"
                    "chr2\t\t30\tdropped\n")
    rows = regions.read_wgs_region_file(str(path))
    assert [tuple(r) for r in rows] == [regions.WGS_COLUMNS] * 5
    assert [r["Name"] for r in rows] == ["chr1_11_61", "four", "five_guides", "six", "seven"]
    assert [(r["chr_id"], r["bpstart"], r["bpend"]) for r in rows][::4] == [("chr1", 11, 61), ("chr2", 1, 30)]
    assert [r["sgRNA"] for r in rows] == ["", "", "GATTACA,ACGT", "GATTACA", ""]
    assert [r["Expected_HDR"] for r in rows] == ["", "", "", "ACGT", ""]
    assert rows[4]["Coding_sequence"].strip() == "ACGTAC" and rows[0]["Coding_sequence"] == ""
    # the same table through the three-column reader agrees on what both hold
    assert [(c, s, e, n.replace(" ", "_")) for c, s, e, n in regions.read_region_file(str(path))] == \
        [(r["chr_id"], r["bpstart"], r["bpend"], r["Name"]) for r in rows]
    path.write_text("chr1\t1\t5\tsame\nchr1\t2\t6\tsame\n")
    with pytest.raises(ValueError, match="distinct"):
        regions.read_wgs_region_file(str(path))


def row(chr_id, s, e, name, guide=""):
    return {"chr_id": chr_id, "bpstart": s, "bpend": e, "Name": name, "sgRNA": guide, "Expected_HDR": "",
            "Coding_sequence": ""}


def test_wgs_rows(tmp_path):
    fasta = write_fasta(tmp_path)
    region_rows = [row("chr1", 1, 41, "upper", "GATTACAG"),                 # forward, over the lower-case start
                   row("chr1", 11, 61, "revcomp", "AAA,TGTAATC"),           # only the reverse complement occurs
                   row("chr1", 11, 61, "nowhere", "GGGGGGGGGG,CCCCCCCCCCC"),
                   row("chr1", 101, 200, "end", ""),                        # cut to the contig's end
                   row("chr1", 500, 600, "past", "ACGT"),                   # past the end: empty
                   row("chr9", 1, 10, "nochr", "")]
    rows = regions.wgs_rows(region_rows, fasta)
    assert rows[0]["Amplicon_Sequence"] == CHR1[:40].upper() and rows[0]["Amplicon_Sequence"].startswith("ACGTACGTAGGATTACAG")
    assert rows[0]["sgRNA"] == "GATTACAG"
    assert "TGTAATC" not in rows[1]["Amplicon_Sequence"] and "GATTACA" in rows[1]["Amplicon_Sequence"]
    assert rows[1]["sgRNA"] == "AAA,TGTAATC"                                # kept whole when one guide is found
    assert rows[2]["sgRNA"] == "" and rows[2]["Amplicon_Sequence"] == rows[1]["Amplicon_Sequence"] == CHR1[10:60].upper()
    assert rows[3]["Amplicon_Sequence"] == CHR1[100:].upper() and len(rows[3]["Amplicon_Sequence"]) == len(CHR1) - 100 == 21
    assert rows[4]["Amplicon_Sequence"] == "" and rows[4]["sgRNA"] == "" and rows[5]["Amplicon_Sequence"] == ""
    assert [r["Name"] for r in rows] == [r["Name"] for r in region_rows] and region_rows[2]["sgRNA"]      # inputs untouched
    # the reference looks for the guide in the sequence as stored: a guide over lower-case bases is not found
    assert regions.wgs_rows([row("chr1", 1, 41, "lower", "ACGTACGT")], fasta)[0]["sgRNA"] == ""
    with pytest.raises(ValueError, match="wrong characters:U"):
        regions.wgs_rows([row("chr1", 1, 41, "bad", "GATUACA")], fasta)
    with pytest.raises(ValueError, match="wrong characters"):
        regions.checked_guides("GATTACA,GAT-ACA", CHR1)
    assert regions.checked_guides("", CHR1) == "" and regions.checked_guides("gattaca", CHR1) == "gattaca"


def test_discovered_rows(tmp_path):
    fasta = write_fasta(tmp_path)

    class Found:
        target_names = ["REGION_chr1_11_61", "REGION_chr2_-3_9"]
        regions = [("chr1", 11, 61), ("chr2", -3, 9)]

    rows = regions.discovered_rows(Found(), fasta)
    assert [r["Name"] for r in rows] == Found.target_names and [r["sgRNA"] for r in rows] == ["", ""]
    assert rows[0]["Amplicon_Sequence"] == CHR1[10:60].upper() and rows[1]["Amplicon_Sequence"] == "ACGTACGT"


@pytest.mark.parametrize("extra", [["--regions", "R", "--summary"],                      # no --genome
                                   ["--by-reference", "--summary", "--genome", "G"],
                                   ["--discover", "--summary", "--genome", "G", "--reference-order"],
                                   ["--regions", "R", "--genome", "G"]])                 # --genome without --summary
def test_command_line_refusals(tmp_path, capsys, extra):
    files = {"B": tmp_path / "in.bam", "R": tmp_path / "regions.txt", "G": tmp_path / "genome.fa"}
    for f in files.values():
        f.write_bytes(b"")
    argv = ["--bam", str(files["B"]), "--out", str(tmp_path / "out")] + [str(files.get(a, a)) for a in extra]
    with pytest.raises(SystemExit) as exc:
        regions.main(argv)
    assert exc.value.code == 2 and "error:" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
