"""The host side of crispresso_amd/demux.py: the ABI listing, the refusals made before any GPU
call, the amplicon table, the report and the FASTQ writer (no GPU here)."""
import gzip

import numpy as np
import pytest

from crispresso_amd import _lib, demux
from tests import demux_model as dm
from tests.test_abi import declared_symbols


def test_header_and_binding_agree():
    assert declared_symbols("crispr_demux.h", "nwd_") == set(_lib.DEMUX_EXPORTS)
    assert len(set(_lib.DEMUX_EXPORTS)) == len(_lib.DEMUX_EXPORTS)
    assert (_lib.NWD_NO_HIT, _lib.NWD_TIE) == (dm.NO_HIT, dm.TIE) == (-1, -2)


def test_library_exports_every_demux_symbol():
    exported = _lib.exported_symbols()
    assert [k for k in _lib.DEMUX_EXPORTS if not exported.get(k)] == []


class NoGpu(demux.GpuDemultiplexer):
    """A demultiplexer whose every use is an error: the refusals below must come first."""

    def __init__(self):
        pass

    def set_amplicons(self, *a, **k):
        raise AssertionError("the GPU was called")

    assign = gather = set_amplicons


AMPS = ["ACGTACGGTTCAGGATCCAGTTGACC", "TTGACCAGTAGCAAGGTCTTACGGAT"]
READS = ["ACGTACGGTTCAGGATCC"]


def refused(amps=AMPS, reads=READS, **kw):
    with pytest.raises(ValueError) as e:
        demux.demultiplex(amps, reads, demultiplexer=NoGpu(), **kw)
    return str(e.value)


@pytest.mark.parametrize("k", [7, 32, 0, -1])
def test_window_length_refused(k):
    assert "8 to 31" in refused(k=k)


def test_limits_themselves_pass_the_checks():
    assert demux.check_params(8, 1) == (8, 1) and demux.check_params(31, 2) == (31, 2)
    buf, off = demux.pack_amplicons(["ACGT"] * 65535)
    assert len(off) == 65536
    demux.check_offsets(np.zeros(4096, np.uint8), np.array([0, 4096], np.int64), "reads", demux.MAX_READ)


def test_min_hits_refused():
    assert "at least 1" in refused(min_hits=0)


def test_amplicon_counts_refused():
    assert "0 amplicons" in refused(amps=[])
    assert "65536 amplicons" in refused(amps=["ACGT"] * 65536)
    buf = np.zeros((1 << 24) + 1, np.uint8)
    assert "amplicon bases" in refused(amps=(buf, np.array([0, len(buf)], np.int64)))


@pytest.mark.parametrize("off", [[0, 8, 4], [4, 0], [0, 4, 19], [-1, 4]])
def test_bad_read_offsets_refused(off):
    buf = np.frombuffer(READS[0].encode(), np.uint8)
    refused(reads=(buf, np.array(off, np.int64)))


def test_bad_amplicon_offsets_refused():
    buf = np.frombuffer(AMPS[0].encode(), np.uint8)
    assert "do not ascend" in refused(amps=(buf, np.array([0, 20, 10], np.int64)))


def test_long_read_refused():
    assert "4097" in refused(reads=["A" * 4097])
    assert "4097" in refused(reads=["ACGT", "C" * 4097, "ACGT"])


def test_read_amplicons_file(tmp_path):
    p = tmp_path / "amplicons.txt"
    p.write_text("# name\tsequence\tguide\n"
                 "FANC F\tacgtACGTnn\tACGT\tACGTTCGTNN\tCGTA\n"
                 "\n"
                 "EMX1\tTTGACCAGTA\n"
                 "no_sequence\n"
                 "\tGGGG\n"
                 "HEK (site 3)\tCCCCAAAATT\t\t\t  # a comment\r\n")
    rows = demux.read_amplicons_file(str(p))
    assert [r["Name"] for r in rows] == ["FANC_F", "EMX1", "HEK_(site_3)"]
    assert [r["Amplicon_Sequence"] for r in rows] == ["ACGTACGTNN", "TTGACCAGTA", "CCCCAAAATT"]
    assert rows[0]["sgRNA"] == "ACGT" and rows[0]["Expected_HDR"] == "ACGTTCGTNN" and rows[0]["Coding_sequence"] == "CGTA"
    assert rows[1]["sgRNA"] == "" and rows[2]["Coding_sequence"] == ""
    assert demux.clean_filename("AMPL_HEK_(site_3)") == "AMPL_HEK_(site_3)"
    assert demux.clean_filename("AMPL_a/b:c*dé") == "AMPL_abcd"


@pytest.mark.parametrize("text, msg", [("a\tACGT\nb\tacgt\n", "amplicons should be all distinct"),
                                       ("a\tACGT\na\tACGG\n", "names should be all distinct"),
                                       ("a\tACGU\n", "wrong characters:U"), ("# nothing\n", "no amplicon")])
def test_amplicons_file_refused(tmp_path, text, msg):
    p = tmp_path / "amplicons.txt"
    p.write_text(text)
    with pytest.raises(ValueError) as e:
        demux.read_amplicons_file(str(p))
    assert msg in str(e.value)


def test_report_columns():
    rows = [{"Name": "a", "Amplicon_Sequence": "ACGT", "sgRNA": "AC", "Expected_HDR": "", "Coding_sequence": ""},
            {"Name": "b", "Amplicon_Sequence": "TTGA", "sgRNA": "", "Expected_HDR": "TTGC", "Coding_sequence": "TG"}]
    lines = demux.report_lines(rows, ["out/AMPL_a.fastq.gz", "out/AMPL_b.fastq.gz"], [30, 10])
    assert lines[0].split("\t") == ["Name", "Amplicon_Sequence", "sgRNA", "Expected_HDR", "Coding_sequence",
                                    "Demultiplexed_fastq.gz_filename", "n_reads", "n_reads_aligned_%"]
    assert lines[1].split("\t") == ["a", "ACGT", "AC", "NA", "NA", "out/AMPL_a.fastq.gz", "30", "75.0"]
    assert lines[2].split("\t") == ["b", "TTGA", "NA", "TTGC", "TG", "out/AMPL_b.fastq.gz", "10", "25.0"]
    # the reference's expression: n_reads / float(N_READS_ALIGNED) * 100.
    assert float(lines[1].split("\t")[-1]) == 30 / float(40) * 100.
    assert demux.report_lines(rows, ["x", "y"], [0, 0])[1].split("\t")[-2:] == ["0", "NA"]
    assert demux.unassigned_report_lines(40, 3, 10) == ["reason\tn_reads\tn_reads_%", "tie\t3\t7.5", "no_hit\t10\t25.0"]


def test_fastq_writer_reverse_strand_record(tmp_path):
    assert demux.fastq_record(b"r1 1:N:0", b"AACGTN-acgX", b"ABCDEFGHIJK", 0) == b"@r1 1:N:0\nAACGTN-acgX\n+\nABCDEFGHIJK\n"
    assert demux.fastq_record(b"r1 1:N:0", b"AACGTN-acgX", b"ABCDEFGHIJK", 1) == b"@r1 1:N:0\nXcgt-NACGTT\n+\nKJIHGFEDCBA\n"
    assert demux.reverse_complement(b"AaCcGgTtN-x") == dm.revcomp(b"AaCcGgTtN-x") == b"x-NaAcCgGtT"
    p = tmp_path / "AMPL_a.fastq.gz"
    n = demux.write_fastq_gz(str(p), [b"r0", b"r1"], [b"ACGG", b"TTGN"], [b"IIH#", b"ABCD"], [0, 1])
    assert n == 2
    with gzip.open(p, "rb") as f:
        assert f.read() == b"@r0\nACGG\n+\nIIH#\n@r1\nNCAA\n+\nDCBA\n"
