"""discover_regions (nwr_discover, crispresso_amd/csrc/nw_regions.hip) against
tests/genome_regions_model.py: the keys in order, n_records, n_aligned, n_no_seq and every hit's
src, bases, qualities, name and strand; and against the recorded output of the reference's own
pipe (tests/golden/genome_regions.json.gz)."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from crispresso_amd import regions, synth
from crispresso_amd.pooled import align_pooled
from tests import genome_regions_model as gm
from tests import regions_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS = [("chr1", 0), ("chr10", 0), ("chr2", 0)]
FIELDS = ("region_offsets", "src", "st", "en", "text_offsets", "text", "qual", "region_table", "n_records")


@pytest.fixture(scope="module")
def extractor():
    with regions.GpuRegionExtractor(0) as x:
        yield x


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "genome_regions.json.gz")) as f:
        return json.loads(f.read())["cases"]


def bam_of(refs, records):
    return regions.read_bam(rc.bam_plain(refs, records))


def compare(res, refs, records, eqx=False, min_reads=0):
    """The result against the model, field by field."""
    want = gm.discover(records, eqx, min_reads)
    table = [tuple(int(v) for v in (r["ref_id"], r["bpstart"], r["bpend"])) for r in res.region_table]
    assert table == want["regions"]
    assert res.region_table["bpstart"].dtype == np.int64 and res.region_table["bpend"].dtype == np.int64
    assert res.regions == [(refs[k[0]][0], k[1], k[2]) for k in want["regions"]]
    assert res.target_names == [gm.region_name(refs[k[0]][0], k) for k in want["regions"]]
    assert res.n_records.tolist() == want["n_records"] and res.n_records.dtype == np.int64
    assert (res.n_aligned, res.n_no_seq, res.n_kept) == (want["n_aligned"], want["n_no_seq"], want["n_kept"])
    assert res.n_emitted == sum(n >= min_reads for n in want["n_records"])
    bad = rc.mismatches(rc.got_hits(res), want)
    assert not bad, "\n".join(bad)
    assert res.n_reads.tolist() == [len(h) for h in want["hits"]]
    assert len(res.region_offsets) == len(want["regions"]) + 1 and res.region_offsets[0] == 0
    assert (np.diff(res.region_offsets) >= 0).all() and res.region_offsets[-1] == len(res.src)
    for g, s in enumerate(want["strand"]):
        assert res.strand(g).tobytes() == b"".join(s) and res.strand(g).dtype == np.uint8
    return want


def check(extractor, refs, records, eqx=False, min_reads=0):
    res = regions.discover_regions(bam_of(refs, records), min_reads, eqx, extractor=extractor)
    return res, compare(res, refs, records, eqx, min_reads)


def same(a, b, fields=FIELDS):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in fields) and a.n_no_seq == b.n_no_seq and \
        a.target_names == b.target_names and getattr(a, "n_aligned", None) == getattr(b, "n_aligned", None)


CIGARS = ["50M", "3S47M", "47M3S", "2H3S40M2I5M3D2M4S1H", "2I3S10M", "3S3S10M", "10M2S3M", "40M10N10M", "40M10P10M",
          "5=3X2M", "10M5=", "3S5=2M", "5=3S", "*"]


def cigar_records():
    records = [rc.rec("c%d" % k, k % 3, 100, c, flag=16 * (k % 2), seq="ACGTAC" if c == "*" else None)
               for k, c in enumerate(CIGARS)]
    records.append(rc.rec("low", 0, 2, "5S10M"))
    records.append(rc.rec("long", 1, 1000, "1M1D2=1I" * 500))          # 2,000 ops
    return records


@pytest.mark.parametrize("eqx", [False, True])
def test_cigars(extractor, eqx):
    res, want = check(extractor, REFS, cigar_records(), eqx)
    span = {r["name"]: gm.span_ops(r["pos"], r["cigar"], eqx) for r in cigar_records()}
    assert span[b"c0"] == (100, 150) and span[b"c1"] == (97, 147) and span[b"c2"] == (100, 150) and span[b"c3"] == (97, 154)
    assert span[b"c4"] == (97, 110) and span[b"c5"] == (94, 110) and span[b"c6"] == (100, 115)
    assert span[b"c7"] == span[b"c8"] == (100, 160) and span[b"c13"] == (100, 100) and span[b"low"] == (-3, 12)
    if eqx:
        assert (span[b"c9"], span[b"c10"], span[b"c11"], span[b"c12"]) == ((100, 110), (100, 115), (97, 107), (100, 108))
        assert span[b"long"] == (1000, 3000)                # 1M, 1D, an M of 2, an I
    else:
        assert (span[b"c9"], span[b"c10"], span[b"c11"], span[b"c12"]) == ((100, 105), (100, 115), (97, 105), (95, 100))
        assert span[b"long"] == (1000, 2000) == gm.span_text(1000, "1M1D2=1I" * 500)      # "2=1I" is one I: nothing
    assert (0, -3, 12) in want["regions"] and (1, 1000, span[b"long"][1]) in want["regions"]


@pytest.mark.parametrize("eqx", [False, True])
def test_golden_cigars_and_files(extractor, golden, eqx):
    for case in golden:
        refs, records = gm.parse_sam(case["sam"])
        res, want = check(extractor, refs, records, eqx)
        if eqx:
            continue
        got = {name + ".fastq": res.fastq_bytes(g, order=res.reference_order(g)).decode("latin-1")
               for g, name in enumerate(res.target_names)}
        assert got == case["files"], case["name"]
        if case["name"] == "order":
            assert res.reference_order(0) != list(range(int(res.n_reads[0])))
            assert res.fastq_bytes(0) == rc.rm.fastq(want["hits"][0])          # the default stays record order


def test_record_filter(extractor):
    seq20 = "ACGTACGTACGTACGTACGT"
    records = [
        rc.rec("mapped", 0, 100, "20M"),
        rc.rec("flag4", 0, 100, "20M", flag=4),
        rc.rec("flag4_more", 0, 300, "20M", flag=4 | 1 | 64),
        rc.rec("noref", -1, 100, "20M"),
        rc.rec("noseq", 0, 100, "20M", seq="*"),
        rc.rec("noqual", 0, 100, "20M", seq=seq20, noqual=True),
        rc.rec("only_noseq_here", 1, 700, "20M", seq="*"),               # a region all of whose records lack sequence
        rc.rec("only_noqual_here", 1, 700, "20M", seq=seq20, noqual=True),
        rc.rec("secondary", 0, 100, "20M", flag=256),
        rc.rec("supplementary", 0, 100, "20M", flag=2048 | 16),
        rc.rec("same_span_other_ref", 2, 100, "20M", flag=16),
        rc.rec("same_start", 0, 100, "30M"),
        rc.rec("mapped2", 0, 100, "20M", flag=16 | 1 | 32),
    ]
    res, want = check(extractor, REFS, records)
    assert want["regions"] == [(0, 100, 120), (0, 100, 130), (2, 100, 120)]
    assert [[h[0] for h in g] for g in want["hits"]] == [[0, 8, 9, 12], [11], [10]]
    assert want["n_no_seq"] == 4 and want["n_aligned"] == 9 and res.strand(0).tobytes() == b"++--"


@pytest.mark.parametrize("n", [255, 256, 257, 1025])
def test_block_edges(extractor, n):
    records = [rc.rec("r%d" % i, i % 3, 10 + (i * 7) % 40, "%dM" % (12 + i % 5), flag=4 if i % 50 == 49 else 0) for i in range(n)]
    records[-1] = rc.rec("last", 2, 999, "3S9M")
    res, want = check(extractor, REFS, records)
    assert want["regions"][-1] == (2, 996, 1008) and want["hits"][-1][0][0] == n - 1


def test_one_large_region_and_many_singletons(extractor):
    records = [rc.rec("r%d" % i, 0, 500, "30M", flag=16 * (i % 2)) for i in range(3000)]
    res, want = check(extractor, REFS, records)
    assert want["n_records"] == [3000] and [h[0] for h in want["hits"][0]] == list(range(3000))
    records = [rc.rec("s%d" % i, (i * 5) % 3, 1 + (i * 7919) % 1000003, "10M") for i in range(5000)]
    res, want = check(extractor, REFS, records)
    assert want["n_records"] == [1] * 5000
    res, want = check(extractor, REFS, records, min_reads=2)
    assert res.n_emitted == 0 and len(res.src) == 0 and len(res.text) == 0 and len(res) == 5000


def keys300():
    return [rc.rec("k%d" % i, i % 3, 100 + 13 * (i % 300), "%dM" % (10 + (i % 300) % 7), flag=16 * (i % 2)) for i in range(900)]


@pytest.mark.parametrize("bits", [0, 2, 6])
def test_hash_bits(extractor, bits, monkeypatch):
    records = keys300()
    plain, want = check(extractor, REFS, records)
    assert len(want["regions"]) == 300 and want["n_records"] == [3] * 300
    monkeypatch.setenv("CRISPR_NWR_HASH_BITS", str(bits))
    with regions.GpuRegionExtractor(0) as x:
        got, _ = check(x, REFS, records)
        assert same(plain, got)
        assert same(got, check(x, REFS, records)[0])


@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_chunks(extractor, chunk, monkeypatch):
    records = keys300()[:400] + cigar_records()
    one, want = check(extractor, REFS, records)
    assert max(want["n_records"]) >= 2 and any(h[-1][0] - h[0][0] >= 300 for h in want["hits"] if h)     # spread over chunks
    monkeypatch.setenv("CRISPR_NWR_CHUNK", str(chunk))
    with regions.GpuRegionExtractor(0) as x:
        for min_reads in (0, 2):
            got, _ = check(x, REFS, records, min_reads=min_reads)
            assert min_reads or same(one, got)
        # the context's other calls after a discovery
        assert same(regions.demux_by_reference(one.bam, extractor=x), regions.demux_by_reference(one.bam, extractor=extractor),
                    FIELDS[:7])


def test_min_reads(extractor):
    records = [rc.rec("a%d" % i, 0, 100, "20M") for i in range(5)] + [rc.rec("b%d" % i, 1, 200, "20M") for i in range(4)]
    records += [rc.rec("c", 2, 300, "20M")]
    records = [records[(i * 3) % 10] for i in range(10)]
    for min_reads, emitted in ((0, 3), (1, 3), (2, 2), (3, 2), (4, 2), (5, 1), (6, 0)):
        res, want = check(extractor, REFS, records, min_reads=min_reads)
        assert want["n_records"] == [5, 4, 1] and res.n_emitted == emitted
        assert res.n_reads.tolist() == [n if n >= min_reads else 0 for n in (5, 4, 1)]
        assert res.target_names == ["REGION_chr1_100_120", "REGION_chr10_200_220", "REGION_chr2_300_320"]
        assert res.reads(2)[1].tolist() == ([0, 20] if min_reads <= 1 else [0]) and (res.fastq_bytes(2) == b"") == (min_reads > 1)


def test_bases_and_qualities(extractor):
    records = [
        rc.rec("even", 0, 10, "16M", seq=rc.NIBBLES, qual=[0, 93] * 8),
        rc.rec("odd", 0, 10, "15M", seq=rc.NIBBLES[1:], qual=[93, 0] * 7 + [93]),
        rc.rec("one", 0, 40, "1M", seq="G", qual=[93]),
        rc.rec("short_seq", 0, 60, "20M", seq="ACGTACGTAC"),
        rc.rec("reverse", 1, 10, "16M", seq=rc.NIBBLES[::-1], qual=[93, 0] * 8, flag=16),      # as stored: no reverse complement
    ]
    res, want = check(extractor, REFS, records)
    assert [h[3] for g in want["hits"] for h in g] == [rc.NIBBLES[1:].encode(), rc.NIBBLES.encode(), b"G", b"ACGTACGTAC",
                                                      rc.NIBBLES[::-1].encode()]
    assert want["hits"][1][0][4] == b"!~" * 8


def test_determinism(extractor):
    records = keys300() + cigar_records() + [rc.rec("s%d" % i, i % 3, 5000 + 17 * i, "10M") for i in range(700)]
    bam = bam_of(REFS, records)
    runs = [regions.discover_regions(bam, 2, extractor=extractor) for _ in range(3)]
    compare(runs[0], REFS, records, min_reads=2)
    assert same(runs[0], runs[1]) and same(runs[0], runs[2]) and len(runs[0].text) > 1000
    empty = regions.discover_regions(bam_of(REFS, []), extractor=extractor)
    assert len(empty) == 0 and empty.regions == [] and empty.n_aligned == 0 and empty.region_offsets.tolist() == [0]


def test_end_to_end(extractor, gpu_aligner_factory, tmp_path):
    amp = synth.random_amplicon(150, 4)
    genome = "T" * 70 + amp + "G" * 45
    (tmp_path / "genome.fa").write_text(">chrA test\n" + "\n".join(genome[i:i + 60] for i in range(0, len(genome), 60)) + "\n"
                                        + ">chrB\nACGT\n")
    records = []
    for k in range(24):
        if k % 3 == 1:        # a 3-base deletion: the span stays the amplicon's
            at = 50 + k
            seq, cigar = amp[:at] + amp[at + 3:], "%dM3D%dM" % (at, 150 - at - 3)
        elif k % 3 == 2:      # clipped ends count into the span
            seq, cigar = amp, "4S142M4S"
        else:
            seq, cigar = amp, "150M"
        records.append(rc.rec("z%02d" % (23 - k), 0, 75 if k % 3 == 2 else 71, cigar, seq=seq, flag=16 * (k % 2)))
    records += [rc.rec("off%d" % k, 1, 1 + k, "4M") for k in range(3)]
    refs = [("chrA", len(genome)), ("chrB", 4)]
    path = tmp_path / "in.bam"
    path.write_bytes(rc.bgzf(rc.bam_plain(refs, records), [3000]))
    res = regions.discover_regions(regions.read_bam(str(path)), min_reads=24, extractor=extractor)
    want = compare(res, refs, records, min_reads=24)
    assert res.regions == [("chrA", 71, 221), ("chrB", 1, 5), ("chrB", 2, 6), ("chrB", 3, 7)] and res.n_reads.tolist() == [24, 0, 0, 0]
    seqs = regions.region_sequences(str(tmp_path / "genome.fa"), res.regions)
    assert seqs == [amp, "ACGT", "CGT", "GT"]
    aligner = gpu_aligner_factory()
    got = align_pooled([seqs[0]], [res.reads(0)], aligner)[0]
    ref = align_pooled([amp], [[h[3].decode() for h in want["hits"][0]]], aligner)[0]
    assert len(got) == 24 and np.array_equal(got.stats, ref.stats) and np.array_equal(got.aln, ref.aln)
    assert int(got.stats["n_ident"].min()) >= 147
    # the command line on the same BAM
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "crispresso_amd.regions", "--bam", str(path), "--discover", "--min-reads", "24",
                        "--genome", str(tmp_path / "genome.fa"), "--reference-order", "--out", str(tmp_path / "cli")],
                       capture_output=True, text=True, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    assert p.stdout.splitlines() == ["REGION_chrA_71_221\t24"]
    assert sorted(os.listdir(str(tmp_path / "cli"))) == ["REGION_chrA_71_221.fastq.gz", "regions.tsv"]
    assert gzip.open(str(tmp_path / "cli" / "REGION_chrA_71_221.fastq.gz")).read() == \
        gm.fastq_reference_order(want["hits"][0], want["strand"][0])
    rows = [line.split("\t") for line in (tmp_path / "cli" / "regions.tsv").read_text().splitlines()]
    assert rows[0] == ["chr_id", "bpstart", "bpend", "n_reads", "n_reads_aligned_%", "sequence"]
    assert rows[1] == ["chrA", "71", "221", "24", "%.6g" % (24 / 27.0 * 100), amp] and rows[4][:4] == ["chrB", "3", "7", "1"]
