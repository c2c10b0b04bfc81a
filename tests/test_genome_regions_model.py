"""tests/genome_regions_model.py against itself (ops == text) and against the recorded output of
the reference's own genome-mode pipe (tests/golden/genome_regions.json.gz, made by
tests/golden/make_genome_regions_golden.py), and the host side of discover_regions:
region_sequences and the command line's argument errors.  No GPU."""
import gzip
import json
import os

import numpy as np
import pytest

from crispresso_amd import regions
from tests import genome_regions_model as gm

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(HERE, "golden", "genome_regions.json.gz")) as f:
        return json.loads(f.read())["cases"]


def test_issue_cases():
    assert gm.span_ops(100, "5=3X2M") == (100, 105) and gm.span_ops(100, "10M5=") == (100, 115)
    assert gm.span_ops(100, "3S5=2M") == (97, 105) and gm.span_ops(100, "3S3S10M") == (94, 110)
    assert gm.span_ops(2, "5S10M") == (-3, 12) and gm.span_ops(100, "*") == (100, 100)
    assert gm.span_ops(100, "2I3S10M") == (97, 110) and gm.span_ops(100, "10M2S3M") == (100, 115)
    assert gm.span_ops(100, "5=3S") == (95, 100)
    assert gm.span_ops(100, "5=3X2M", eqx=True) == (100, 110) and gm.span_ops(100, "10M5=", eqx=True) == (100, 115)
    assert gm.span_ops(100, "2H3S40M2I5M3D2M4S1H") == (97, 154)


def test_ops_equal_text_on_the_golden_cigars(golden):
    n = 0
    for case in golden:
        for r in gm.parse_sam(case["sam"])[1]:
            assert gm.span_ops(r["pos"], r["cigar"]) == gm.span_text(r["pos"], r["cigar"]), r["cigar"]
            assert gm.span_ops(r["pos"], r["cigar"], True) == gm.span_text_eqx(r["pos"], r["cigar"]), r["cigar"]
            n += 1
    assert n > 50


def test_ops_equal_text_on_random_cigars():
    rng = np.random.Generator(np.random.PCG64(7))
    seen = set()
    for _ in range(4000):
        ops = "".join("%d%s" % (int(rng.integers(0, 60)), "MIDNSHP=X"[int(rng.integers(0, 9))])
                      for _ in range(int(rng.integers(1, 9))))
        pos = int(rng.integers(1, 300))
        assert gm.span_ops(pos, ops) == gm.span_text(pos, ops), ops
        assert gm.span_ops(pos, ops, True) == gm.span_text_eqx(pos, ops), ops
        seen |= set(c for c in ops if not c.isdigit())
    assert seen == set("MIDNSHP=X")


def test_model_equals_the_reference_pipe(golden):
    assert [c["name"] for c in golden] == ["cigars", "order", "references"]
    for case in golden:
        refs, records = gm.parse_sam(case["sam"])
        for span in (None, gm.span_text):
            m = gm.discover(records, span=span)
            got = {gm.region_name(refs[k[0]][0], k) + ".fastq": gm.fastq_reference_order(h, s).decode("latin-1")
                   for k, h, s in zip(m["regions"], m["hits"], m["strand"])}
            assert sorted(got) == sorted(case["files"]), case["name"]
            for name in got:
                assert got[name] == case["files"][name], (case["name"], name)
            assert m["n_records"] == [case["files"][n].count("\n") // 4 for n in
                                      (gm.region_name(refs[k[0]][0], k) + ".fastq" for k in m["regions"])]
    by = {c["name"]: c for c in golden}
    assert "REGION_chr1_-3_12.fastq" in by["cigars"]["files"] and "REGION_chr1_100_105.fastq" not in by["cigars"]["files"]
    assert {"REGION_chr1_100_101.fastq", "REGION_chr1_100_1005.fastq", "REGION_chr10_100_101.fastq",
            "REGION_chr2_100_101.fastq"} <= set(by["references"]["files"])
    assert len(by["order"]["files"]) == 1 and len(by["order"]["sam"]) == 18


def test_regions_are_in_numeric_order(golden):
    refs, records = gm.parse_sam(next(c for c in golden if c["name"] == "references")["sam"])
    m = gm.discover(records)
    assert [r[0] for r in refs] == ["chr1", "chr10", "chr2"]
    assert m["regions"] == sorted(m["regions"]) and m["regions"][0] == (0, -2, 5)
    assert m["regions"].index((0, 100, 101)) < m["regions"].index((0, 100, 1005))       # 1005 < 101 as text
    assert gm.discover(records, min_reads=2)["n_records"] == m["n_records"]
    assert [len(h) for h in gm.discover(records, min_reads=2)["hits"]] == [n if n >= 2 else 0 for n in m["n_records"]]


FASTA = ">chrA first\nACGTACGTAC\nGGGGGCCCCC\nTTT\n>chrB\nAAAAACCCCC\n>chrC\n\n"


@pytest.mark.parametrize("fai", [False, True])
@pytest.mark.parametrize("newline", ["\n", "\r\n"])
def test_region_sequences(tmp_path, fai, newline):
    path = tmp_path / "g.fa"
    path.write_bytes(FASTA.replace("\n", newline).encode())
    if fai:
        w = 10 + len(newline)
        first = len(">chrA first" + newline)
        second = first + 2 * w + 3 + len(newline) + len(">chrB" + newline)
        (tmp_path / "g.fa.fai").write_text("chrA\t23\t%d\t10\t%d\nchrB\t10\t%d\t10\t%d\n" % (first, w, second, w))
    whole = "ACGTACGTACGGGGGCCCCCTTT"
    regs = [("chrA", 1, 24), ("chrA", 1, 2), ("chrA", 10, 12), ("chrA", 11, 21), ("chrA", 20, 30), ("chrA", 0, 3),
            ("chrA", -5, 2), ("chrA", 24, 30), ("chrA", 5, 5), ("chrB", 6, 11), ("chrZ", 1, 5), ("chrA", 23, 24)]
    got = regions.region_sequences(str(path), regs)
    assert got == [whole, "A", whole[9:11], whole[10:20], whole[19:], whole[:2], "A", "", "", "CCCCC", "", "T"]
    for (c, s, e), seq in zip(regs, got):       # [bpstart, bpend) cut to [1, length]
        if c == "chrA":
            assert seq == whole[max(s, 1) - 1:max(e - 1, 0)]


@pytest.mark.parametrize("argv", [
    ["--bam", "x.bam", "--discover", "--by-reference", "--out", "o"],
    ["--bam", "x.bam", "--discover", "--regions", "r.txt", "--out", "o"],
    ["--bam", "x.bam", "--out", "o"],
    ["--bam", "x.bam", "--by-reference", "--min-reads", "5", "--out", "o"],
    ["--bam", "x.bam", "--by-reference", "--reference-order", "--out", "o"],
    ["--bam", "x.bam", "--by-reference", "--genome", "g.fa", "--out", "o"],
    ["--bam", "x.bam", "--discover", "--min-reads", "-1", "--out", "o"],
    ["--bam", "x.bam", "--discover", "--min-reads", "many", "--out", "o"],
    ["--bam", "missing.bam", "--discover", "--out", "o"],
    ["--bam", "x.bam", "--discover", "--genome", "missing.fa", "--out", "o"],
    ["--bam", "x.bam", "--discover"],
])
def test_command_line_argument_errors(argv, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    (tmp_path / "x.bam").write_bytes(b"")
    (tmp_path / "g.fa").write_text(FASTA)
    (tmp_path / "r.txt").write_text("chrA\t1\t5\n")
    with pytest.raises(SystemExit) as e:
        regions.main(argv)
    assert e.value.code == 2 and "usage:" in capsys.readouterr().err
    assert not (tmp_path / "o").exists()
