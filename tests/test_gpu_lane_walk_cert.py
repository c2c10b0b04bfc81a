"""The lane walk's refined certificate (nw_band_walk.hip, count_mis): its counts over the single diagonals
beyond the band stop once they are past the bound that decides the certificate.  Every case is a resident
pass run with the lane walk and with the wave walk: the same records, run offsets, runs and path counts
bit for bit, and every read of the lane-walk pass against the CPU oracle (tests/every_read.py)."""
import numpy as np
import pytest

from crispresso_amd import synth
from crispresso_amd.aligner import pack_2bit, pack_reads
from crispresso_amd.needle_options import NeedleOptions
from tests.every_read import every_read
from tests.test_gpu_wide_first import OTHER, amplicon, deletion, same, subs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aligner(gpu_aligner_factory):
    return gpu_aligner_factory()   # one context for the module's cases


def resident(a, amp, pr, n, lane):
    a.set_reference(amp)
    a.upload_packed(pr)
    a.set_lane_walk(lane)
    try:
        a.run_async()
        a.sync()
        ob = a.download_ops(n)
    finally:
        a.set_lane_walk(False)
    return ob, (ob.stats.copy(), ob.ops_off.copy(), ob.ops[: int(ob.ops_off[n])].copy()), a.path_counts()


def both_walks(a, amp, reads, oracle_params=None):
    """-> the lane-walk pass's batch, the path counts (the same for both walks)."""
    buf, off = pack_reads(reads)
    pr = pack_2bit(buf, off)
    n = len(off) - 1
    ob, lane, c_lane = resident(a, amp, pr, n, True)
    chk = every_read(amp, buf, off, ob, threads=16, oracle_params=oracle_params)
    assert chk["mismatches"] == 0, (chk, c_lane)
    _, wave, c_wave = resident(a, amp, pr, n, False)
    same(lane, wave, "lane walk / wave walk")
    assert c_lane == c_wave, (c_lane, c_wave)
    print("path counts", c_lane)
    return ob, c_lane


def shuffled(rng, reads):
    return [reads[i] for i in rng.permutation(len(reads))]


@pytest.mark.parametrize("La", [40, 100, 250, 256])
def test_five_substitutions_take_the_refined_certificate(aligner, La):
    """m La - 5 (m + x) is within O of m pmax: the bound alone does not certify these reads, the counts over
    the diagonals just beyond the band do -- each past its bound within its first dwords.  (4 substitutions
    beside them: certified by the bound.)  No read leaves the first level."""
    rng = np.random.Generator(np.random.PCG64(600 + La))
    amp = amplicon(La, 600 + La)
    reads = [subs(amp, 4 + q % 2, rng) for q in range(301)] + [amp] * 600
    _, c = both_walks(aligner, amp, shuffled(rng, reads))
    assert c["band16"] == 301 and c["band32"] == 0 and c["band_fallback"] == c["wide_first"] == 0, c


def periodic_batch():
    """An amplicon of period 9: the diagonal d = 9, the first beyond the band of an equal-length pair
    (diagonals -7 .. 8), pairs every read base from the tenth on with a copy of its own amplicon base.
    A read with its 5 substitutions among the first 9 bases has no mismatch on that diagonal: where the
    main diagonal is the read's best alignment (the unit resembles itself, so small gaps score higher for
    most of these reads), the diagonal ties its score, the count runs to its end within the bound and the
    certificate fails -- the next level's read.  One with a substitution at base 245 as well is past the
    bound only with the diagonal's last dwords."""
    rng = np.random.Generator(np.random.PCG64(99))
    unit = "ACGTTGCAG"
    amp = (unit * 28)[:250]
    flip = lambda s, at: "".join(OTHER[ch] if p in at else ch for p, ch in enumerate(s))
    tied = [flip(amp, set(rng.choice(9, 5, replace=False).tolist())) for _ in range(40)]
    late = [flip(amp, set(rng.choice(9, 4, replace=False).tolist()) | {245}) for _ in range(40)]
    return amp, tied, late, rng


def test_a_diagonal_counted_to_its_end(aligner):
    amp, tied, late, rng = periodic_batch()
    for r in tied:   # the precondition: d = 9 ties the main diagonal's score
        x, y = np.frombuffer(amp.encode(), np.uint8), np.frombuffer(r.encode(), np.uint8)
        assert (x[:-9] != y[9:]).sum() == 0 and (x != y).sum() == 5
    reads = shuffled(rng, tied + late + [amp] * 300)
    ob, c = both_walks(aligner, amp, reads)
    assert c["band16"] == len(tied) + len(late), c
    # the tied reads whose verified score is the main diagonal's, m La - 5 (m + x): d = 9 reaches it, so the
    # 16-diagonal band cannot certify them and they left the first level
    main = 5 * ob.scale * len(amp) - 5 * 9 * ob.scale
    is_tied = set(tied)
    n_tied = sum(1 for i, r in enumerate(reads) if r in is_tied and int(ob.stats["score"][i]) == main)
    assert n_tied > 0 and c["band32"] + c["band_fallback"] >= n_tied, (n_tied, c)


def test_other_gap_penalties(gpu_aligner_factory, oracle):
    """-gapopen=12 -gapextend=1 (scale 1: m = 5, O = 12): the bounds come from the call's penalties."""
    go, ge = 12.0, 1.0
    a = gpu_aligner_factory(NeedleOptions.parse(f"-gapopen={go} -gapextend={ge}"))
    try:
        rng = np.random.Generator(np.random.PCG64(121))
        amp = amplicon(100, 121)
        reads = [subs(amp, 4 + q % 3, rng) for q in range(240)] + [subs(deletion(amp, 50, 3), 2, rng)]
        both_walks(a, amp, shuffled(rng, reads + [amp] * 300), oracle_params=oracle.params(go, ge))
    finally:
        a.close()


def test_c2_mix_of_20k(aligner):
    """The benchmark's read mix (its DP reads: mostly 4 and 5 substitutions)."""
    amp = synth.random_amplicon(250, 1)
    buf, off = synth.reads_from(amp, 20_000, 12)
    both_walks(aligner, amp, synth.unpack(buf, off))
