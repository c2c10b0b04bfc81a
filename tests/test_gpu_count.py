"""The sgRNA counting kernels (crispresso_amd/csrc/nw_count.hip, include/crispr_count.h) through
crispresso_amd/count.py against tests/count_model.py: every read's pos and group_of_read, every
group's key, first and count (tests/count_cases.mismatches names the read or group that differs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from crispresso_amd import count, fastq
from tests import count_cases as cc
from tests import count_model as cm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "test_L001_R1_001.fastq.gz")
MS = (1, 3, 4, 5, 20, 33, 64, 128)
LS = (0, 1, 19, 20, 21, 64)


@pytest.fixture(scope="module")
def counter():
    with count.GpuGuideCounter(0) as c:
        yield c


@pytest.fixture(scope="module")
def mixed():
    reads, T, L, info = cc.mixed_batch()
    want = cm.fast_model(reads, T, L)
    # sizes: a seed change cannot quietly empty the case
    assert len(reads) == 50000 and len(info["library"]) == 1000
    assert info["sub"] > 2000 and info["miss"] > 800
    assert want["n_found"] == 50000 - info["miss"] and len(want["guides"]) > 2500
    return reads, T, L, want


def check(counter, reads, T, L, guides=None, lead=0, want=None, collided=0):
    want = want or cm.fast_model(reads, T, L, guides)
    got = cc.run(counter, reads, T, L, guides, lead)
    bad = cc.mismatches(got, want)
    assert not bad, "\n".join(bad)
    assert got.first.dtype == np.int64 and got.counts.dtype == np.int64
    if guides is None:
        assert all(a < b for a, b in zip(got.first.tolist(), got.first.tolist()[1:]))
    if collided is not None:
        assert got.collided == collided
    return got


@pytest.mark.parametrize("m", MS)
def test_find_edges(counter, m):
    for L in LS:
        reads, T, sizes = cc.edge_batch(m, L)
        assert sizes["every_position"] == (70 if m <= 64 else m + 6) - m + 1
        assert sizes["one_substitution"] == m and sizes["long"] == 5 and sizes["straddle"] == (0 if m == 1 else 4 if m < 4 else 6)
        assert max(len(r) for r in reads) > 70000 and sizes["reads"] >= 150
        want = cm.fast_model(reads, T, L)
        assert want["n_found"] >= sizes["every_position"] and -1 in want["pos"]
        check(counter, reads, T, L, want=want)


def test_python_slice_cases(counter):
    for reads, T, L in cc.slice_cases():
        check(counter, reads, T, L)
    # the two hand-computed ones, spelled out
    got = cc.run(counter, [b"cccACGTAccccccc"], b"ACGTA", 20)
    assert got.pos.tolist() == [3] and got.guides == [b"ccc"]
    got = cc.run(counter, [b"cccACGTA" + b"c" * 17], b"ACGTA", 22)
    assert got.pos.tolist() == [3] and got.guides == [b""]


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_every_start_alignment(counter, lead):
    """The batch starts at every offset mod 4 of its allocation; odd read lengths move every
    later start."""
    reads, T, sizes = cc.edge_batch(5, 20)
    odd = [r[: len(r) - (len(r) % 2 == 0)] if len(r) > 1 else r for r in reads]
    assert sum(len(r) % 2 for r in odd) > 150
    check(counter, odd, T, 20, lead=lead)
    check(counter, odd, T, 20, guides=[b"", odd[30][:20], b"ACGT"], lead=lead)


def test_identical_reads_one_slot(counter):
    """20,000 copies of one read: one slot, the count added once per wavefront."""
    read = b"ac" + b"ACGTTGCAACGTTGCAACGT" + cc.T20 + b"cag"
    for _ in range(2):
        got = check(counter, [read] * 20000, cc.T20, 20)
        assert got.guides == [read[2:22]] and got.counts.tolist() == [20000]


def test_all_distinct_guides(counter):
    """20,000 distinct guides: every read claims a slot (probe chains at half load)."""
    reads, T, L = cc.distinct_batch()
    assert len(reads) == 20000 and len({r[2:22] for r in reads}) == 20000
    for _ in range(2):
        got = check(counter, reads, T, L)
        assert len(got) == 20000


def test_mixed_batch_and_context_reuse(counter, mixed):
    reads, T, L, want = mixed
    for _ in range(2):
        check(counter, reads, T, L, want=want)
    # a smaller batch with another (T, L) on the same context
    small, T2, _ = cc.edge_batch(33, 19)
    check(counter, small, T2, 19)
    reads3, T3, L3, _ = cc.mixed_batch(3000, 50, 31, b"GTTTTAGAG", 7)
    check(counter, reads3, T3, L3)


def child(mode, **env):
    p = subprocess.run([sys.executable, "-m", "tests.count_cases", mode], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("bits", [4, 8])
def test_collided_path(bits, mixed):
    """CRISPR_NWC_HASH_BITS cuts the hash (read at nwc_create: a child process each): equal
    hashes of different guides go through the probe chains, verify and the host's exact
    grouping, and the groups are still the model's."""
    assert len(mixed[3]["guides"]) > 2 ** bits             # collisions are certain, not just likely
    out = child("mixed", CRISPR_NWC_HASH_BITS=str(bits))
    assert out["ok"], out["bad"]
    assert out["collided"][0] > 0


def test_full_hash_has_no_collided_read(counter, mixed):
    reads, T, L, want = mixed
    got = check(counter, reads, T, L, want=want, collided=0)
    assert counter.last_collided() == 0 and got.collided == 0


@pytest.fixture(scope="module")
def whitelist():
    reads, T, L, lines, info = cc.whitelist_batch()
    want = cm.fast_model(reads, T, L, lines)
    keys = want["guides"]
    assert len(keys) == 1000 + 40 + 2 and len(lines) == len(keys) + 2          # two duplicated lines
    assert want["n_counted"] < want["n_found"] - 3000                            # guides that are no members
    assert all(want["counts"][keys.index(k)] == 0 for k in info["absent"])      # members with zero reads
    assert want["counts"][keys.index(b"")] == 4                                  # the key b"" and empty guides
    assert len(info["short"]) == 19 and want["counts"][keys.index(info["short"])] == 0
    assert sum(c > 0 for c in want["counts"]) > 900
    return reads, T, L, lines, want


def test_whitelist(counter, whitelist):
    reads, T, L, lines, want = whitelist
    for _ in range(2):
        got = check(counter, reads, T, L, guides=lines, want=want)
        assert got.first.tolist() == [-1] * len(got)
    check(counter, reads, T, L, guides=[])
    check(counter, reads[:10], T, L, guides=[b"A" * 70, b"", b"A" * 70])        # a key longer than any guide


def test_whitelist_short_hash(whitelist):
    out = child("whitelist", CRISPR_NWC_HASH_BITS="6")
    assert out["ok"], out["bad"]
    assert out["collided"] == [0]


def test_chunks(counter):
    """CRISPR_NWC_CHUNK=1000 in a child: the table lives across the chunks, and the result is the
    one-chunk run's byte for byte."""
    reads, T, L, special = cc.chunk_batch()
    want = cm.fast_model(reads, T, L)
    assert len(reads) == 10500
    g = want["guides"].index(special)
    assert want["first"][g] == 2500 and want["counts"][g] == 3
    assert [r for r, x in enumerate(want["group_of_read"]) if x == g] == [2500, 6500, 10200]
    assert all(p < 0 for p in want["pos"][4000:5000]) and want["pos"][3999] >= 0 and want["pos"][5000] >= 0
    out = child("chunks", CRISPR_NWC_CHUNK="1000")
    assert out["ok"], out["bad"]
    here = [check(counter, reads, T, L, want=want),
            check(counter, reads, T, L, guides=[reads[2500][4:24], reads[0][4:24], b""]),
            check(counter, [], T, L), check(counter, reads[2500:2501], T, L), check(counter, reads[4000:4001], T, L)]
    assert out["digest"] == [cc.digest(x) for x in here]
    assert len(here[2]) == 0 and here[2].n_reads == 0 and here[3].counts.tolist() == [1] and len(here[4]) == 0


@pytest.fixture(scope="module")
def golden_reads():
    _, buf, off = fastq.read_fastq_as_fasta_py(GOLDEN)
    return [bytes(buf[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def test_fastq(counter, golden_reads):
    want = cm.fast_model(golden_reads, b"TAGCCCCTTAAG", 20)
    assert (want["n_reads"], want["n_found"], len(want["guides"])) == (8906, 6604, 87)
    got = count.count_fastq(GOLDEN, "TAGCCCCTTAAG", 20, counter=counter, want_pos=True, want_group_of_read=True)
    assert not cc.mismatches(got, want)
    # a 12-mer near the reads' start: idx < L, the Python-slice cases on real reads
    want = cm.fast_model(golden_reads, b"CCCTCAAATCTT", 20)
    assert sum(0 <= p < 20 for p in want["pos"]) == 8022
    got = count.count_fastq(GOLDEN, "ccctcaaatctt", 20, counter=counter, want_pos=True, want_group_of_read=True)
    assert not cc.mismatches(got, want)


def test_fastq_quality_filter(counter):
    _, buf, off = fastq.read_fastq_as_fasta_py(GOLDEN, 30, 0)
    reads = [bytes(buf[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
    assert len(reads) == 7691
    want = cm.fast_model(reads, b"TAGCCCCTTAAG", 20)
    got = count.count_fastq(GOLDEN, "TAGCCCCTTAAG", 20, min_average_read_quality=30, counter=counter, want_pos=True,
                            want_group_of_read=True)
    assert not cc.mismatches(got, want)


@pytest.mark.parametrize("with_guides", [False, True])
def test_cli_file(tmp_path, counter, golden_reads, with_guides):
    args = [sys.executable, "-m", "crispresso_amd.count", "-r", GOLDEN, "-t", "TAGCCCCTTAAG", "-l", "20", "-o",
            str(tmp_path), "-n", "pin"]
    guides = None
    if with_guides:
        first = cm.fast_model(golden_reads, b"TAGCCCCTTAAG", 20)["guides"]
        guides = first[:40] + [b"ACGTACGTACGTACGTACGT", first[3]]
        (tmp_path / "guides.txt").write_bytes(b"\n".join(guides) + b"\n")
        args += ["-f", str(tmp_path / "guides.txt")]
    p = subprocess.run(args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    name = "CRISPRessoCount_%s_on_test_L001_R1_001.fastq.gz.txt" % ("only_ref_guides" if with_guides else "no_ref_guides")
    back = pd.read_csv(tmp_path / "CRISPRessoCount_on_pin" / name, sep="\t", index_col=0, keep_default_na=False)
    want = count.count_fastq(GOLDEN, "TAGCCCCTTAAG", 20, guides, counter=counter).to_frame()
    pd.testing.assert_frame_equal(back, want)
    assert len(back) == (41 if with_guides else 87)


def test_determinism(counter, mixed):
    reads, T, L, want = mixed
    a, b = cc.run(counter, reads, T, L), cc.run(counter, reads, T, L)
    assert a.guides == b.guides
    for x, y in ((a.counts, b.counts), (a.first, b.first), (a.pos, b.pos), (a.group_of_read, b.group_of_read)):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert cc.digest(a) == cc.digest(b)


def test_capacity_and_unsupported(counter):
    """More groups than the first call's room: they are fetched without a second count; the
    C entry itself refuses m and L outside its limits."""
    import ctypes

    from crispresso_amd import _lib

    reads, T, L = cc.distinct_batch(70000 - 1, 25)
    got = check(counter, reads, T, L)
    assert len(got) == 70000 - 1 > 1 << 16
    lib, ctx = counter._lib, counter._ctx
    buf, off = cc.pack([b"ACGT"])
    outs = [ctypes.c_int64() for _ in range(4)]
    for m, L in ((0, 20), (129, 20), (4, -1), (4, 65)):
        rc = lib.nwc_count(ctx, _lib.ptr(buf), _lib.ptr(off), 1, b"A" * max(m, 1), m, L, None, None, -1, None, None,
                           None, None, 0, 0, None, None, *[ctypes.byref(o) for o in outs], None)
        assert rc == _lib.NW_E_UNSUPPORTED and lib.nwc_last_error(ctx)
