"""The parser of Trimmomatic step strings (crispresso_amd.trim.TrimProgram) and the presence of
the program entry point: what is accepted, what is refused by name, and that TrimOptions keeps
its narrower contract."""
import ctypes
import os

import numpy as np
import pytest

from crispresso_amd import _lib
from crispresso_amd.trim import (MAX_STEPS, TrimOptions, TrimProgram, TrimStep, UnsupportedTrimStep)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
FASTA = os.path.join(GOLDEN, "NexteraPE-PE.fa")
CLIP = "ILLUMINACLIP:" + FASTA + ":2:30:10"


def test_the_manuals_string():
    p = TrimProgram.from_steps(CLIP + " LEADING:3 TRAILING:3 SLIDINGWINDOW:4:15 MINLEN:36")
    assert p.steps == [TrimStep("LEADING", 3), TrimStep("TRAILING", 3), TrimStep("SLIDINGWINDOW", 4, 15.0),
                       TrimStep("MINLEN", 36)]
    o = TrimOptions.from_steps(CLIP)
    assert p.clip == o and p.clip.minlen == 0
    assert (o.seed_mismatches, o.palindrome_threshold, o.simple_threshold, o.min_prefix) == (2, 30, 10, 8)
    as_list = TrimProgram.from_steps([CLIP, "LEADING:3", "TRAILING:3", "SLIDINGWINDOW:4:15", "MINLEN:36"])
    assert as_list == p


def test_a_program_without_clip_and_every_step():
    p = TrimProgram.from_steps("HEADCROP:2 CROP:100 AVGQUAL:20 SLIDINGWINDOW:5:25.5 MINLEN:0")
    assert p.clip is None
    assert p.steps == [TrimStep("HEADCROP", 2), TrimStep("CROP", 100), TrimStep("AVGQUAL", 20),
                       TrimStep("SLIDINGWINDOW", 5, 25.5), TrimStep("MINLEN", 0)]
    native = p.native_steps()
    assert [(s.op, s.arg) for s in native[:5]] == [(5, 2), (4, 100), (6, 20), (3, 5), (7, 0)]
    assert native[3].r == 25.5 and native[3].R == 127.5
    # r is a float32, and r * w a float32 product
    q = TrimProgram.from_steps("SLIDINGWINDOW:3:0.1").native_steps()[0]
    assert q.r == float(np.float32(0.1)) and q.R == float(np.float32(np.float32(0.1) * np.float32(3)))
    assert TrimProgram.from_steps("SLIDINGWINDOW:4:.5").steps[0].r == 0.5
    assert TrimProgram.from_steps("CROP:1048576 LEADING:1000").steps == [TrimStep("CROP", 1 << 20),
                                                                          TrimStep("LEADING", 1000)]


@pytest.mark.parametrize("steps,named", [
    ("LEADING:3 MAXINFO:40:0.5", "MAXINFO:40:0.5"),
    ("TOPHRED33", "TOPHRED33"),
    ("CROP:10 TOPHRED64", "TOPHRED64"),
    ("LEADING:3 SLIDINGWINDOWS:4:15", "SLIDINGWINDOWS:4:15"),
    ("leading:3", "leading:3"),
    ("LEADING:3 " + CLIP, "ILLUMINACLIP"),
    (CLIP + " " + CLIP + " LEADING:3", "ILLUMINACLIP"),
    ("CROP:-1", "CROP:-1"),
    ("CROP:+1", r"CROP:\+1"),
    ("CROP:1e3", "CROP:1e3"),
    ("CROP:0x10", "CROP:0x10"),
    ("CROP:1048577", "CROP:1048577"),
    ("CROP:99999999999999999999", "CROP:9999"),
    ("CROP", "CROP"),
    ("CROP:", "CROP:"),
    ("CROP:1:2", "CROP:1:2"),
    ("LEADING:1001", "LEADING:1001"),
    ("TRAILING:1001", "TRAILING:1001"),
    ("AVGQUAL:1001", "AVGQUAL:1001"),
    ("SLIDINGWINDOW:0:15", "SLIDINGWINDOW:0:15"),
    ("SLIDINGWINDOW:4", "SLIDINGWINDOW:4"),
    ("SLIDINGWINDOW:4:-1", "SLIDINGWINDOW:4:-1"),
    ("SLIDINGWINDOW:4:1e1", "SLIDINGWINDOW:4:1e1"),
    ("SLIDINGWINDOW:4:abc", "SLIDINGWINDOW:4:abc"),
    ("SLIDINGWINDOW:4:nan", "SLIDINGWINDOW:4:nan"),
    ("SLIDINGWINDOW:4:.", r"SLIDINGWINDOW:4:\."),
    ("SLIDINGWINDOW:4:1001", "SLIDINGWINDOW:4:1001"),
])
def test_refusals_name_the_step(steps, named):
    with pytest.raises(UnsupportedTrimStep, match=named):
        TrimProgram.from_steps(steps)


def test_sixteen_steps_after_the_clip_and_no_more():
    assert MAX_STEPS == 16
    p = TrimProgram.from_steps([CLIP] + ["CROP:%d" % (100 - k) for k in range(16)])
    assert len(p.steps) == 16 and p.clip is not None
    with pytest.raises(UnsupportedTrimStep, match="CROP:84"):
        TrimProgram.from_steps([CLIP] + ["CROP:%d" % (100 - k) for k in range(17)])


def test_trim_options_from_steps_is_unchanged():
    with pytest.raises(UnsupportedTrimStep, match="LEADING:3"):
        TrimOptions.from_steps(CLIP + " LEADING:3 MINLEN:40")
    o = TrimOptions.from_steps("MINLEN:40 " + CLIP)
    assert o.minlen == 40 and len(o.adapters) == 4


def test_the_program_entry_is_exported_and_declared():
    assert "nwt_trim_program" in _lib.TRIM_EXPORTS
    assert _lib.exported_symbols()["nwt_trim_program"]
    with open(os.path.join(ROOT, "include", "crispr_trim.h")) as f:
        text = f.read()
    assert " nwt_trim_program(" in text and "nwt_step" in text and "NWT_MAX_STEPS = 16" in text
    assert ctypes.sizeof(_lib.NwtStep) == 16


def test_the_single_end_adapter_fixture():
    from crispresso_amd.trim import read_adapter_fasta
    recs = read_adapter_fasta(os.path.join(GOLDEN, "TruSeq3-SE.fa"))
    assert [len(s) for _, s in recs] == [34, 34]
    o = TrimOptions.from_steps("ILLUMINACLIP:" + os.path.join(GOLDEN, "TruSeq3-SE.fa") + ":0:90:10:0:true")
    assert len(o.common_adapters) == 2 and o.prefix_pairs == []
