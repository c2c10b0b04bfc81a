"""The host side of crispresso_amd/count.py: the ABI listing, the refusals made before any GPU
call, the whitelist file, the reference's table and the output names (no GPU here)."""
import numpy as np
import pandas as pd
import pytest

from crispresso_amd import _lib, count
from tests.test_abi import declared_symbols


def test_header_and_binding_agree():
    assert declared_symbols("crispr_count.h", "nwc_") == set(_lib.COUNT_EXPORTS)
    assert len(set(_lib.COUNT_EXPORTS)) == len(_lib.COUNT_EXPORTS)


def test_library_exports_every_count_symbol():
    exported = _lib.exported_symbols()
    assert [k for k in _lib.COUNT_EXPORTS if not exported.get(k)] == []


class NoGpu(count.GpuGuideCounter):
    """A counter whose every use is an error: the refusals below must come first."""

    def __init__(self):
        pass

    def count(self, *a, **k):
        raise AssertionError("the GPU was called")


TEXT = np.frombuffer(b"ACGTACGTACGT", np.uint8)
OFF = np.array([0, 4, 12], np.int64)


@pytest.mark.parametrize("tracr, names", [("", "empty"), ("   ", "empty"), ("ACGU", "U"), ("AC-GT.", "- ."),
                                          ("ACGTRYK", "K R Y")])
def test_tracr_refused(tracr, names):
    with pytest.raises(ValueError) as e:
        count.count_guides(TEXT, OFF, tracr, counter=NoGpu())
    assert names in str(e.value)


def test_tracr_is_stripped_and_upper_cased():
    assert count.check_tracr("  gttnTAG\n") == b"GTTNTAG"
    assert count.check_tracr(b"acgt") == b"ACGT"


@pytest.mark.parametrize("kw", [dict(tracrRNA="A" * 129), dict(guide_length=-1), dict(guide_length=65)])
def test_lengths_out_of_range_refused(kw):
    with pytest.raises(ValueError):
        count.count_guides(TEXT, OFF, **dict(dict(tracrRNA="ACGT"), **kw), counter=NoGpu())


def test_limits_themselves_pass_the_checks():
    assert len(count.check_tracr("A" * 128)) == 128 and count.check_tracr("A") == b"A"
    assert count.check_guide_length(0) == 0 and count.check_guide_length(64) == 64


@pytest.mark.parametrize("off", [[0, 8, 4], [4, 0], [0, 4, 13], [-1, 4]])
def test_bad_offsets_refused(off):
    with pytest.raises(ValueError):
        count.count_guides(TEXT, np.array(off, np.int64), "ACGT", counter=NoGpu())


def test_read_guides_file(tmp_path):
    p = tmp_path / "guides.txt"
    p.write_bytes(b"AAAAAGATGATTTTTTTCTC\nAAAATATTTTTATCCCCTAA\r\n  AAAAAGATGATTTTTTTCTC \n\nacgt\n\nACGTACGTACGTACGTACG")
    assert count.read_guides_file(str(p)) == [b"AAAAAGATGATTTTTTTCTC", b"AAAATATTTTTATCCCCTAA", b"", b"acgt",
                                              b"ACGTACGTACGTACGTACG"]


def reference_frame(guides_count, N_READS):
    """The reference's three expressions (CountCORE:344-347) and its sort, made stable."""
    df_guide_counts = pd.Series(guides_count, name="Read_Counts").to_frame()
    df_guide_counts.index.name = "Guide_Sequence"
    df_guide_counts["Read_%"] = df_guide_counts["Read_Counts"] / N_READS * 100
    df_guide_counts["RPM"] = df_guide_counts["Read_Counts"] / N_READS * 1000000
    return df_guide_counts.sort_values(by="Read_Counts", ascending=False, kind="stable")


def test_to_frame_is_the_references_table():
    d = {"ACGT": 5, "TTTT": 9, "": 5, "acgt": 0, "GGGG": 9, "CCCC": 1, "NNNN": 5}
    gc = count.GuideCounts([k.encode() for k in d], np.array(list(d.values()), np.int64),
                           np.arange(len(d), dtype=np.int64), n_reads=40, n_found=34, n_counted=34)
    got = gc.to_frame()
    pd.testing.assert_frame_equal(got, reference_frame(d, 40))
    # ties in the defined order: the order of the dict
    assert list(got.index) == ["TTTT", "GGGG", "ACGT", "", "NNNN", "CCCC", "acgt"]
    assert list(got.columns) == ["Read_Counts", "Read_%", "RPM"] and got.index.name == "Guide_Sequence"
    assert got["Read_%"].tolist()[0] == 9 / 40 * 100 and got["RPM"].tolist()[-2] == 1 / 40 * 1000000


def test_table_round_trip(tmp_path):
    d = {"ACGT": 5, "TTTT": 9, "GGGG": 9}
    gc = count.GuideCounts([k.encode() for k in d], np.array(list(d.values()), np.int64),
                           np.arange(3, dtype=np.int64), 30, 23, 23)
    p = tmp_path / "t.txt"
    gc.to_frame().to_csv(p, sep="\t")
    back = pd.read_csv(p, sep="\t", index_col=0, keep_default_na=False)
    pd.testing.assert_frame_equal(back, gc.to_frame())


def test_output_paths(tmp_path):
    d, f = count.output_paths("/data/run1/lib_R1.fastq.gz")
    assert d == "CRISPRessoCount_on_lib_R1" and f == d + "/CRISPRessoCount_no_ref_guides_on_lib_R1.fastq.gz.txt"
    d, f = count.output_paths("lib.fastq", name="screen", output_folder=str(tmp_path), with_guides=True)
    assert d == str(tmp_path / "CRISPRessoCount_on_screen")
    assert f == d + "/CRISPRessoCount_only_ref_guides_on_lib.fastq.txt"
