"""The region extraction kernels (crispresso_amd/csrc/nw_regions.hip, include/crispr_regions.h)
through crispresso_amd/regions.py against tests/regions_model.py: every hit of every region --
src, st, en, text, quals and name (tests/regions_cases.mismatches names the region and the hit
that differ)."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from crispresso_amd import regions, synth
from crispresso_amd.pooled import align_pooled
from tests import regions_cases as rc
from tests import regions_model as rm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def extractor():
    with regions.GpuRegionExtractor(0) as x:
        yield x


def run(extractor, refs, records, regs, eqx=False, cuts=None):
    bam = regions.read_bam(rc.bgzf(rc.bam_plain(refs, records), cuts))
    return regions.extract_regions(bam, regs, eqx_as_match=eqx, extractor=extractor)


def check(extractor, refs, records, regs, eqx=False, want=None):
    want = want or rm.extract(records, regs, eqx)
    res = run(extractor, refs, records, regs, eqx)
    bad = rc.mismatches(rc.got_hits(res), want)
    assert not bad, "\n".join(bad)
    assert res.n_reads.tolist() == [len(h) for h in want["hits"]]
    assert res.src.dtype == np.int64 and res.st.dtype == np.int32 and res.text.dtype == np.uint8
    return res, want


@pytest.mark.parametrize("eqx", [False, True])
def test_cigar_edges(extractor, eqx):
    refs, records, regs = rc.cigar_edges()
    res, want = check(extractor, refs, records, regs, eqx)
    hits = {regs[g]: [h[:3] for h in want["hits"][g]] for g in range(len(regs))}
    assert hits[(0, 101, 109)] == [(0, 4, 13)] and hits[(0, 101, 108)] == [] and hits[(0, 100, 111)] == [(0, 3, 15)]
    assert hits[(0, 104, 110)] == [(0, 9, 14)]                                  # right after the I
    assert hits[(0, 200, 309)] == [(1, 3, 12)]                                  # behind H and S
    assert hits[(0, 250, 305)] == [] and hits[(0, 204, 304)] == [] and hits[(0, 204, 305)] == [(1, 7, 8)]      # the N gap
    assert hits[(0, 300, 307)] == [(2, 0, 7)]                                   # P advances nothing
    assert hits[(0, 400, 401)] == [(3, 0, 1)]
    assert hits[(0, 400, 409)] == ([] if not eqx else [(3, 0, 9)])
    assert hits[(0, 500, 514)] == ([] if not eqx else [(4, 0, 14)])
    assert hits[(0, 600, 600)] == []                                            # no CIGAR
    assert hits[(0, 1000, 2998)] == [(6, 0, 999)] and hits[(0, 1001, 1002)] == []
    assert sum(map(len, want["hits"])) > 150


def test_slice_edges(extractor):
    refs, records, regs = rc.slice_edges()
    res, want = check(extractor, refs, records, regs)
    by = {regs[g]: want["hits"][g] for g in range(len(regs))}
    assert len(by[(1, 1, 70000)][0][3]) == 69999 and by[(1, 70000, 1)][0][3] == b""
    assert [h[3] for h in by[(0, 12, 12)]] == [b"", b""] and [h[5] for h in by[(0, 12, 12)]] == [b"even_1", b"odd_2"]
    assert [h[3] for h in by[(0, 20, 12)]] == [b"", b""]                         # bpend < bpstart: counted
    assert by[(0, 10, 25)][0][3] == rc.NIBBLES[:15].encode() and by[(0, 10, 25)][0][4][:2] == b"!~"
    assert {(h[1] & 1, h[2] & 1) for g in want["hits"] for h in g if h[2] > h[1]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert by[(0, 64, 77)][0][1:4] == (4, 17, b"ACGTAC") and by[(0, 75, 79)][0][3] == b""      # cut to l_seq
    assert any(len(h[3]) == 1 for g in want["hits"] for h in g)


def test_record_filter(extractor):
    refs, records, regs = rc.record_filter()
    res, want = check(extractor, refs, records, regs)
    assert [[h[0] for h in g] for g in want["hits"]] == [[0, 8, 9], [4], [0, 8], [], []]
    assert res.n_no_seq == want["n_no_seq"] == 4      # noseq and noqual, on the two regions they lie on


def test_region_table(extractor):
    refs, records, regs = rc.many_regions_one_record()
    res, want = check(extractor, refs, records, regs)
    assert all(0 in [h[0] for h in g] for g in want["hits"]) and len(regs) == 70
    refs, records, regs = rc.many_records_one_region()
    res, want = check(extractor, refs, records, regs)
    assert len(want["hits"][0]) > 1500 and want["hits"][1] == [] and want["hits"][3] == []
    assert want["hits"][0] == want["hits"][2]                                    # the duplicate
    refs, records, regs = rc.random_case()                                       # unsorted regions
    assert regs != sorted(regs)
    res, want = check(extractor, refs, records, regs)
    assert sum(map(len, want["hits"])) > 100 and want["n_no_seq"] > 0
    refs, records, regs = rc.table_past_lds()
    assert len(regs) == 5000
    res, want = check(extractor, refs, records, regs)
    assert sum(map(len, want["hits"])) > 1000


def test_zero_regions_and_zero_records(extractor):
    refs, records, regs = rc.random_case(50, 5)
    res = run(extractor, refs, records, [])
    assert len(res) == 0 and len(res.src) == 0 and len(res.text) == 0 and res.n_no_seq == 0
    res = run(extractor, refs, [], regs)
    assert res.n_reads.tolist() == [0] * len(regs) and len(res.text) == 0
    assert res.reads(0)[1].tolist() == [0] and res.fastq_bytes(0) == b"" and res.names(0) == []
    res = regions.demux_by_reference(regions.read_bam(rc.bam_plain([], [])), extractor=extractor)
    assert len(res) == 0


def same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in
               ("region_offsets", "src", "st", "en", "text_offsets", "text", "qual")) and a.n_no_seq == b.n_no_seq


@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_chunks(extractor, chunk, monkeypatch):
    refs, records, regs = rc.random_case(500, 40)
    one, want = check(extractor, refs, records, regs)
    again = run(extractor, refs, records, regs)                  # two calls on one context
    assert same(one, again)
    monkeypatch.setenv("CRISPR_NWR_CHUNK", str(chunk))
    with regions.GpuRegionExtractor(0) as x:
        got = run(x, refs, records, regs)
        assert same(one, got), rc.mismatches(rc.got_hits(got), want)
        by_ref = regions.demux_by_reference(got.bam, extractor=x)
    assert same(by_ref, regions.demux_by_reference(one.bam, extractor=extractor))


def test_demux_by_reference(extractor):
    refs, records = rc.demux_case()
    want = rm.demux(records, len(refs))
    bam = regions.read_bam(rc.bgzf(rc.bam_plain(refs, records), [777]))
    res = regions.demux_by_reference(bam, extractor=extractor)
    bad = rc.mismatches(rc.got_hits(res), want)
    assert not bad, "\n".join(bad)
    assert res.target_names == [n for n, _ in refs] and res.n_reads[7] == 0 and (np.delete(res.n_reads, 7) > 0).all()
    assert res.n_no_seq == want["n_no_seq"] == 2
    assert res.fastq_bytes(3) == rm.fastq(want["hits"][3]) and res.names(3)[0] == records[want["hits"][3][0][0]]["name"]


def test_determinism(extractor):
    refs, records, regs = rc.table_past_lds(1000)
    runs = [run(extractor, refs, records, regs) for _ in range(3)]
    assert same(runs[0], runs[1]) and same(runs[0], runs[2]) and len(runs[0].text) > 1000


def pooled_case():
    """3 amplicons laid on one reference; reads that span them with soft clips, an insertion and
    a deletion."""
    amps = [synth.random_amplicon(n, seed) for n, seed in ((150, 1), (180, 2), (201, 3))]
    genome = "".join("T" * 50 + a for a in amps) + "T" * 50
    starts = [genome.index(a) + 1 for a in amps]
    refs = [("chrA", len(genome)), ("chrB", 1000)]
    records = []
    for g, (a, s) in enumerate(zip(amps, starts)):
        for k in range(20):
            lead, tail = 5 + k % 7, 3 + k % 5
            body = genome[s - 1 - lead:s - 1 + len(a) + tail]
            if k % 4 == 1:        # a 3-base deletion in the middle
                at = lead + 60 + k
                seq, cigar = body[:at] + body[at + 3:], "%dM3D%dM" % (at, len(body) - at - 3)
            elif k % 4 == 2:      # a 2-base insertion
                at = lead + 40 + k
                seq, cigar = body[:at] + "GG" + body[at:], "%dM2I%dM" % (at, len(body) - at)
            else:
                seq, cigar = "AC" + body, "2S%dM" % len(body)
            records.append(rc.rec("a%d_%d" % (g, k), 0, s - lead, cigar, seq=seq))
    records.append(rc.rec("elsewhere", 1, starts[0], "200M"))
    regs = [("chrA", s, s + len(a), "amp%d" % g) for g, (a, s) in enumerate(zip(amps, starts))]
    return amps, refs, records, regs


def test_end_to_end(extractor, gpu_aligner_factory, tmp_path):
    amps, refs, records, regs = pooled_case()
    want = rm.extract(records, [(0, s, e) for _c, s, e, _n in regs])
    assert [len(h) for h in want["hits"]] == [20, 20, 20]
    path = tmp_path / "in.bam"
    path.write_bytes(rc.bgzf(rc.bam_plain(refs, records), [5000]))
    bam = regions.read_bam(str(path))
    res = regions.extract_regions(bam, regs, extractor=extractor)
    assert not rc.mismatches(rc.got_hits(res), want)
    aligner = gpu_aligner_factory()
    got = align_pooled(amps, [res.reads(g) for g in range(3)], aligner)
    ref = align_pooled(amps, [[h[3].decode() for h in want["hits"][g]] for g in range(3)], aligner)
    for g in range(3):
        assert len(got[g]) == 20 and np.array_equal(got[g].stats, ref[g].stats)
        assert np.array_equal(got[g].aln, ref[g].aln)
        assert int(got[g].stats["n_ident"].min()) >= len(amps[g]) - 4
    # the FASTQ of a target, and the command line on the same BAM
    for g in range(3):
        out = tmp_path / ("w%d.fastq.gz" % g)
        assert res.write_fastq_gz(g, str(out)) == 20
        assert gzip.open(str(out)).read() == rm.fastq(want["hits"][g])
    region_file = tmp_path / "regions.txt"
    region_file.write_text("".join("%s\t%d\t%d\t%s\n" % r for r in regs))
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "crispresso_amd.regions", "--bam", str(path), "--regions", str(region_file),
                        "--out", str(tmp_path / "cli")], capture_output=True, text=True, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    assert p.stdout.splitlines() == ["amp%d\t20" % g for g in range(3)]
    for g in range(3):
        assert gzip.open(str(tmp_path / "cli" / ("amp%d.fastq.gz" % g))).read() == rm.fastq(want["hits"][g])
