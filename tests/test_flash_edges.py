"""The paired-end merge kernel (crispresso_amd/csrc/flash_merge.hip) held to the FLASH 1.2.11
restatement (oracle/flash_oracle.py) where tests/test_flash.py does not reach: tied overlaps, pairs on
and one mismatch over the density limit, length / quality / option / alphabet edges, reads up to the
4096-base limit, a batch larger than the launch grid (a wavefront's second pair), the C ABI's refusals
and the empty batch.  The restatement itself is first held to plain scalar loops (CPU).

Every GPU test compares merge_pairs(...).merged(i) with Merger(**same options).merge_pair(...) for every
pair -- bytes, qualities and the outie flag -- and asserts on the CPU, before it calls the GPU, that its
inputs exercise what they were built for."""
import os
import sys

import numpy as np
import pytest

from crispresso_amd import _lib
from crispresso_amd.flash import FlashError, FlashOptions, MergeResult, merge_packed, merge_pairs
from tests.test_flash import synth_pairs

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import flash_oracle  # noqa: E402

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
ACGT = np.frombuffer(b"ACGT", np.uint8)
CRISPRESSO = dict(min_overlap=4, max_overlap=100, max_mismatch_density=0.25, allow_outies=True)


def rc(s):
    return bytes(s)[::-1].translate(COMP)


def rnd(rng, k):
    return bytes(rng.choice(ACGT, k)) if k else b""


def rnd_quals(rng, k, lo=35, hi=75):
    return bytes(rng.integers(lo, hi, k).astype(np.uint8))


def substitute(rng, read, where):
    """read with the base at every index of `where` replaced by a different one of A C G T."""
    r = bytearray(read)
    for p in where:
        r[p] = b"ACGT"[(b"ACGT".index(r[p]) + int(rng.integers(1, 4))) % 4]
    return bytes(r)


def oracle_all(pairs, kw):
    m = flash_oracle.Merger(**kw)
    return [m.merge_pair(*p) for p in pairs]


def gpu_merge(pairs, kw):
    s1, q1, s2, q2 = ([p[i] for p in pairs] for i in range(4))
    return merge_pairs(s1, q1, s2, q2, FlashOptions(**kw))


def assert_gpu_is(pairs, kw, exp, what):
    res = gpu_merge(pairs, kw)
    assert len(res.length) == len(pairs)
    for i, e in enumerate(exp):
        assert res.merged(i) == e, f"{what} {kw}: pair {i} (reads of {len(pairs[i][0])} and {len(pairs[i][2])})"
    return res


def staged(m, s1, q1, s2, q2):
    """Merger.merge_pair's view of a pair: read 1 and the reverse-complemented read 2, canonical bases,
    qualities minus the offset."""
    r1 = flash_oracle._CANON[np.frombuffer(s1, dtype=np.uint8)]
    a1 = np.frombuffer(q1, dtype=np.uint8).astype(np.int32) - m.off
    r2 = flash_oracle._COMP[flash_oracle._CANON[np.frombuffer(s2, dtype=np.uint8)]][::-1]
    a2 = (np.frombuffer(q2, dtype=np.uint8).astype(np.int32) - m.off)[::-1]
    return r1, a1, r2, a2


# ---- A. the restatement against scalar loops (CPU) ----

def scalar_merge(s1, qs1, s2, qs2, min_overlap=10, max_overlap=65, max_mismatch_density=0.25, allow_outies=False,
                 phred_offset=33, cap_mismatch_quals=False):
    """The rules of oracle/flash_oracle.py's docstring as plain loops: one over positions, one over bases;
    np.float32 only for the two divisions and the comparisons; the first candidate wins ties."""
    def canon(c):
        c = c - 32 if ord("a") <= c <= ord("z") else c
        return c if c in b"ACGT" else ord("N")

    comp = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A"), ord("N"): ord("N")}
    r1 = [canon(c) for c in s1]
    q1 = [c - phred_offset for c in qs1]
    r2 = [comp[canon(c)] for c in reversed(s2)]
    q2 = [c - phred_offset for c in reversed(qs2)]
    best = None   # (density, quality score, outie, position)
    scans = [(False, r1, q1, r2, q2, 0)]
    if allow_outies:
        scans.append((True, r2, q2, r1, q1, 1))
    for outie, a, qa, b, qb, first in scans:
        if len(b) < min_overlap:
            continue
        for pos in range(first, len(a) - min_overlap + 1):
            eff = min(len(a) - pos, len(b), max_overlap)
            mm = qt = 0
            for k in range(eff):
                if a[pos + k] != b[k]:
                    mm += 1
                    qt += min(qa[pos + k], qb[k])
            d = np.float32(mm) / np.float32(eff)
            q = np.float32(qt) / np.float32(eff)
            if best is None or d < best[0] or (d == best[0] and q < best[1]):
                best = (d, q, outie, pos)
    if best is None or best[0] > np.float32(max_mismatch_density):
        return None
    _, _, outie, pos = best
    a, qa, b, qb = (r2, q2, r1, q1) if outie else (r1, q1, r2, q2)
    ov = min(len(a) - pos, len(b))
    seq, qual = list(a[:pos]), list(qa[:pos])
    for k in range(ov):
        x, y, qx, qy = a[pos + k], b[k], qa[pos + k], qb[k]
        if x == y:
            seq.append(x)
            qual.append(max(qx, qy))
        else:
            seq.append(x if qx > qy else y)
            mq = max(abs(qx - qy), 2)
            qual.append(min(mq, 2) if cap_mismatch_quals else mq)
    if len(b) > ov:
        seq += b[ov:]
        qual += qb[ov:]
    else:
        seq += a[pos + ov:]
        qual += qa[pos + ov:]
    return bytes(seq), bytes((q + phred_offset) & 0xff for q in qual), outie


RESTATEMENT_SETTINGS = [
    CRISPRESSO,
    dict(min_overlap=1, max_overlap=7, max_mismatch_density=0.1, allow_outies=True, cap_mismatch_quals=True),
    dict(min_overlap=10, max_overlap=5, max_mismatch_density=1.0, allow_outies=False),
    dict(min_overlap=6, max_overlap=30, max_mismatch_density=0.0, allow_outies=True, phred_offset=64),
]


def restatement_pairs(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    other = b"ACGTNacgtnRY.-"
    out = []
    for k in range(n):
        flen = int(rng.integers(0, 121))
        if (k // 4) % 2 == 0:      # (k // 4: every option set sees both kinds)
            frag = rnd(rng, flen)
        else:                      # a tandem repeat of a 1-5 base unit
            unit = rnd(rng, int(rng.integers(1, 6)))
            frag = (unit * (flen // len(unit) + 1))[:flen]
        la, lb = int(rng.integers(0, 71)), int(rng.integers(0, 71))
        r1, r2 = bytearray(frag[:la]), bytearray(rc(frag)[:lb])
        if k % 5 == 4:             # both reads run through a 30-base fragment
            frag = (frag + rnd(rng, 30))[:30]
            r1 = bytearray((frag + rnd(rng, 40))[:max(la, 31)])
            r2 = bytearray((rc(frag) + rnd(rng, 40))[:max(lb, 31)])
        for r in (r1, r2):
            for _ in range(int(rng.integers(0, 3))):
                if len(r):
                    r[int(rng.integers(0, len(r)))] = other[int(rng.integers(0, len(other)))]
        out.append((bytes(r1), rnd_quals(rng, len(r1), 33, 127), bytes(r2), rnd_quals(rng, len(r2), 33, 127)))
    return out


def test_restatement_matches_scalar_loops():
    pairs = restatement_pairs(1600, 101)
    n_comb = n_out = n_empty = 0
    for k, p in enumerate(pairs):
        kw = RESTATEMENT_SETTINGS[k % 4]
        exp = scalar_merge(*p, **kw)
        got = flash_oracle.Merger(**kw).merge_pair(*p)
        assert got == exp, f"pair {k} under {kw}: {p}"
        n_comb += exp is not None
        n_out += exp is not None and exp[2]
        n_empty += len(p[0]) == 0 or len(p[2]) == 0
    print(f"restatement: {len(pairs)} pairs, {n_comb} combined, {n_out} outies, {n_empty} with an empty read")
    assert n_comb >= 500 and n_out >= 100 and n_empty >= 10


# ---- B. ties ----

def tie_pairs():
    rng = np.random.Generator(np.random.PCG64(21))
    out = []
    for _ in range(200):
        unit = rnd(rng, int(rng.integers(1, 7)))
        flen = int(rng.integers(60, 201))
        frag = (unit * (flen // len(unit) + 1))[:flen]
        frag = substitute(rng, frag, rng.integers(0, flen, int(rng.integers(0, 4))))
        r1 = frag[:int(rng.integers(40, 151))]
        r2 = rc(frag)[:int(rng.integers(40, 151))]
        out.append((r1, rnd_quals(rng, len(r1)), r2, rnd_quals(rng, len(r2))))
    hand = [(b"A" * 50, b"T" * 50), (b"A" * 150, b"T" * 150), (b"A" * 300, b"T" * 300),   # several lane strides
            (b"A" * 80, b"T" * 50), (b"A" * 50, b"T" * 80), (b"A" * 200, b"T" * 70),      # an innie ties an outie
            (b"AC" * 40, b"GT" * 40), (b"N" * 90, b"N" * 90), (b"N" * 64, b"N" * 130)]
    for a, b in hand:
        out.append((a, b"I" * len(a), b, b"I" * len(b)))                # equal qualities: scan order decides
        out.append((a, rnd_quals(rng, len(a)), b, rnd_quals(rng, len(b))))
    return out


def tied_minimum(m, p):
    """Is the lowest density of the pair's scans reached at two or more positions?"""
    r1, a1, r2, a2 = staged(m, *p)
    scans = [m._scan(r1, a1, r2, a2, 0)] + ([m._scan(r2, a2, r1, a1, 1)] if m.allow_outies else [])
    dens = np.concatenate([sc[0] for sc in scans if sc is not None])
    return dens.size > 0 and int((dens == dens.min()).sum()) >= 2


@pytest.mark.gpu
def test_gpu_merge_ties():
    pairs = tie_pairs()
    for kw in (CRISPRESSO, dict(min_overlap=10, max_overlap=30, allow_outies=False)):
        m = flash_oracle.Merger(**kw)
        exp = oracle_all(pairs, kw)
        tied = sum(tied_minimum(m, p) for p in pairs[:200])
        n_comb = sum(e is not None for e in exp)
        print(f"ties {kw}: {len(pairs)} pairs, {n_comb} combined, {tied} of the 200 seeded with a tied minimum")
        assert tied >= 150
        assert all(tied_minimum(m, p) for p in pairs[200:])
        assert n_comb >= 150
        assert_gpu_is(pairs, kw, exp, "ties")


# ---- C. the density limit ----

def density_limit_pairs(md, max_ov, seed):
    """60 error-free pairs, read 1 damaged at k = int(md * eff) places of the scored window (on the
    limit) and at k + 1 (over it) -> (on-limit pairs, over-limit pairs)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    on, over = [], []
    for _ in range(60):
        L = int(rng.integers(60, 151))
        ov = int(rng.integers(12, min(L, 140)))
        frag = rnd(rng, 2 * L - ov)
        r1, r2 = frag[:L], rc(frag)[:L]
        q1, q2 = rnd_quals(rng, L), rnd_quals(rng, L)
        eff = min(ov, max_ov)
        k = int(np.float32(md) * np.float32(eff))
        where = (L - ov) + rng.permutation(eff)[:k + 1]   # read 2 starts under read 1's base L - ov
        on.append((substitute(rng, r1, where[:k]), q1, r2, q2))
        over.append((substitute(rng, r1, where), q1, r2, q2))
    return on, over


@pytest.mark.gpu
@pytest.mark.parametrize("md,max_ov", [(0.25, 100), (0.1, 30), (0.25, 65)])
def test_gpu_merge_near_the_density_limit(md, max_ov):
    kw = dict(min_overlap=10, max_overlap=max_ov, max_mismatch_density=md, allow_outies=False)
    on, over = density_limit_pairs(md, max_ov, 31)
    exp_on, exp_over = oracle_all(on, kw), oracle_all(over, kw)
    n_on = sum(e is not None for e in exp_on)
    n_over = sum(e is None for e in exp_over)
    print(f"density limit {md} / {max_ov}: {n_on} of 60 on the limit combined, {n_over} of 60 over it not")
    assert n_on >= 50 and n_over >= 50
    assert_gpu_is(on + over, kw, exp_on + exp_over, "density limit")


# ---- D. lengths ----

MATE_LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 67, 127, 128, 129, 191, 192, 193, 255, 256, 257]
PARTNER_LENGTHS = [0, 1, 4, 10, 33, 64, 130]


def length_edge_pairs(seed, sub_rate=None, quals=None):
    """Both reads cut from one fragment in three geometries -> [(geometry, pair)].  sub_rate (lo, hi):
    substitutions at that rate, half in each read; quals: the quality bytes to draw from."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []

    def add(geometry, r1, r2):
        if sub_rate is not None:
            rate = rng.uniform(*sub_rate) / 2
            r1 = substitute(rng, r1, np.flatnonzero(rng.random(len(r1)) < rate))
            r2 = substitute(rng, r2, np.flatnonzero(rng.random(len(r2)) < rate))
        if quals is None:
            q1, q2 = rnd_quals(rng, len(r1)), rnd_quals(rng, len(r2))
        else:
            q1, q2 = (bytes(rng.choice(np.frombuffer(quals, np.uint8), len(r))) if r else b"" for r in (r1, r2))
        out.append((geometry, (r1, q1, r2, q2)))

    for i, la in enumerate(MATE_LENGTHS):
        for j, lb in enumerate(PARTNER_LENGTHS):
            n1, n2 = (la, lb) if (i + j) % 2 else (lb, la)
            # a plain innie: read 2 starts under read 1's base n1 - ov
            ov = min(n1, n2, 40)
            frag = rnd(rng, n1 + n2 - ov)
            add("innie", frag[:n1], rc(frag)[:n2])
            # read 2 inside read 1, not at its start, read 1's tail after it
            big, small = max(n1, n2), min(n1, n2)
            if small >= 1 and big >= small + 2:
                frag = rnd(rng, big)
                at = int(rng.integers(1, big - small))
                add("contained", frag, rc(frag[at:at + small]))
            # both reads run through a short fragment into unrelated tails: an outie
            if min(n1, n2) >= 2:
                flen = max(1, min(n1, n2) * 2 // 3)
                frag = rnd(rng, flen)
                add("outie", frag + rnd(rng, n1 - flen), rc(frag) + rnd(rng, n2 - flen))
    return out


@pytest.mark.gpu
def test_gpu_merge_length_edges():
    tagged = length_edge_pairs(41)
    pairs = [p for _, p in tagged]
    assert {len(p[0]) for p in pairs} | {len(p[2]) for p in pairs} >= set(MATE_LENGTHS)
    for min_ov in (1, 4, 10):
        kw = dict(CRISPRESSO, min_overlap=min_ov)
        exp = oracle_all(pairs, kw)
        comb = {g: sum(e is not None and e[2] == (g == "outie") for (t, _), e in zip(tagged, exp) if t == g)
                for g in ("innie", "contained", "outie")}
        shorter = sum(min(len(p[0]), len(p[2])) < min_ov for p in pairs)
        exactly = sum(min_ov in (len(p[0]), len(p[2])) for p in pairs)
        print(f"lengths, min_overlap {min_ov}: {len(pairs)} pairs, combined {comb}, "
              f"{shorter} with a read shorter than min_overlap, {exactly} with one exactly that long")
        assert min(comb.values()) >= 20 and shorter >= 10 and exactly >= 1
        assert_gpu_is(pairs, kw, exp, "lengths")
    empty = [(b"", b"", b"", b"")] * 5
    res = assert_gpu_is(empty, CRISPRESSO, [None] * 5, "empty reads")
    assert not res.flags.any()


# ---- E. qualities ----

def mismatch_quality_counts(m, pairs):
    """Overlap mismatches at the position the restatement chose: (with equal qualities, with a
    quality difference of 1)."""
    equal = one = 0
    for p in pairs:
        r1, a1, r2, a2 = staged(m, *p)
        pos, outie = m.align(r1, a1, r2, a2)
        if pos < 0:
            continue
        a, qa, b, qb = (r2, a2, r1, a1) if outie else (r1, a1, r2, a2)
        ov = min(len(a) - pos, len(b))
        mis = a[pos:pos + ov] != b[:ov]
        diff = np.abs(qa[pos:pos + ov] - qb[:ov])
        equal += int((mis & (diff == 0)).sum())
        one += int((mis & (diff == 1)).sum())
    return equal, one


@pytest.mark.gpu
def test_gpu_merge_quality_edges():
    pairs = [p for _, p in length_edge_pairs(51, sub_rate=(0.05, 0.10), quals=b'!"#I~')
             if min(len(p[0]), len(p[2])) >= 4]
    settings = [dict(CRISPRESSO), dict(CRISPRESSO, cap_mismatch_quals=True), dict(CRISPRESSO, phred_offset=64)]
    for kw in settings:
        m = flash_oracle.Merger(**kw)
        exp = oracle_all(pairs, kw)
        equal, one = mismatch_quality_counts(m, pairs)
        n_comb = sum(e is not None for e in exp)
        print(f"qualities {kw}: {len(pairs)} pairs, {n_comb} combined, overlap mismatches with equal "
              f"qualities {equal}, a difference of 1 {one}")
        assert equal >= 50 and one >= 50 and n_comb >= 100
        assert_gpu_is(pairs, kw, exp, "qualities")


# ---- F. alphabet ----

@pytest.mark.gpu
def test_gpu_merge_other_bytes():
    rng = np.random.Generator(np.random.PCG64(61))
    other = b"RYKMSWBDHVryn.-*"
    s1, q1, s2, q2 = synth_pairs(600, 13)
    replaced = 0
    for reads in (s1, s2):
        for i, r in enumerate(reads):
            r = bytearray(r)
            for _ in range(int(rng.integers(0, 7))):
                r[int(rng.integers(0, len(r)))] = other[int(rng.integers(0, len(other)))]
            reads[i] = bytes(r)
            replaced += sum(c not in b"ACGTNacgtn" for c in r)
    pairs = list(zip(s1, q1, s2, q2))
    assert replaced >= 2000
    for kw in (CRISPRESSO, dict(min_overlap=10, max_overlap=65, allow_outies=False)):
        exp = oracle_all(pairs, kw)
        n_comb = sum(e is not None for e in exp)
        print(f"other bytes {kw}: {len(pairs)} pairs, {replaced} bytes outside ACGTNacgtn, {n_comb} combined")
        assert n_comb >= 150
        assert_gpu_is(pairs, kw, exp, "other bytes")


# ---- G. options ----

@pytest.mark.gpu
def test_gpu_merge_option_edges():
    rng = np.random.Generator(np.random.PCG64(71))
    pairs = list(zip(*synth_pairs(300, 17)))
    for k in range(0, 300, 10):   # a tenth of the pairs free of errors
        frag = rnd(rng, int(rng.integers(120, 260)))
        r1, r2 = frag[:int(rng.integers(80, 120))], rc(frag)[:int(rng.integers(80, 120))]
        pairs[k] = (r1, rnd_quals(rng, len(r1)), r2, rnd_quals(rng, len(r2)))
    for over in (dict(min_overlap=1), dict(max_overlap=1), dict(min_overlap=10, max_overlap=5),
                 dict(max_mismatch_density=0.0), dict(max_mismatch_density=1.0)):
        kw = dict(CRISPRESSO, **over)
        exp = oracle_all(pairs, kw)
        n_comb = sum(e is not None for e in exp)
        print(f"options {over}: {len(pairs)} pairs, {n_comb} combined")
        assert n_comb >= 10
        assert_gpu_is(pairs, kw, exp, "options")


# ---- H. long reads ----

def innie(rng, n1, n2, ov):
    frag = rnd(rng, n1 + n2 - ov)
    r1, r2 = frag[:n1], rc(frag)[:n2]
    return (r1, rnd_quals(rng, n1), r2, rnd_quals(rng, n2))


@pytest.mark.gpu
def test_gpu_merge_long_reads():
    """Reads up to the 4096-base limit of include/crispr_flash.h, on both sides of the 4080 bases up to
    which four staged pairs fit 64 KiB of LDS, with short pairs in the same batch."""
    rng = np.random.Generator(np.random.PCG64(81))
    short = list(zip(*synth_pairs(9, 19)))
    f = rnd(rng, 1500)
    r1, r2 = f + rnd(rng, 500), rc(f) + rnd(rng, 300)   # 2000 and 1800 bases through a 1500-base fragment
    through = (r1, rnd_quals(rng, 2000), r2, rnd_quals(rng, 1800))
    batches = [([innie(rng, 4080, 4080, 200)], [7960]),
               ([innie(rng, 4096, 4096, 100), innie(rng, 4081, 300, 150), innie(rng, 300, 4096, 120), through],
                [8092, 4231, 4276, 2300])]
    for longs, lengths in batches:
        pairs = short[:5] + longs + short[5:]
        exp = oracle_all(pairs, CRISPRESSO)
        got = [e and len(e[0]) for e in exp[5:5 + len(longs)]]
        print(f"long reads: {len(pairs)} pairs, {sum(e is not None for e in exp)} combined, long ones {got}")
        assert got == lengths
        if len(longs) == 4:
            assert exp[8][2] is True   # the read-through pair combines as an outie
        res = assert_gpu_is(pairs, CRISPRESSO, exp, "long reads")
        assert list(res.length[5:5 + len(longs)]) == lengths
    with pytest.raises(FlashError, match="4096"):
        gpu_merge([(b"A" * 4097, b"I" * 4097, b"ACGT" * 10, b"I" * 40)], CRISPRESSO)


# ---- I. a batch larger than the grid ----

def device_cus():
    try:
        import torch
        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        return 256


@pytest.mark.gpu
def test_gpu_merge_batch_larger_than_the_grid():
    """The launch is capped at 16 blocks of 4 wavefronts per CU: in a larger batch a wavefront merges a
    second and a third pair over the LDS bytes its previous pair left behind."""
    rng = np.random.Generator(np.random.PCG64(91))
    stride = 4 * 16 * device_cus()
    n = 2 * stride + 5
    assert n > stride
    pool = list(zip(*synth_pairs(600, 11)))
    for _ in range(8):
        pool.append(innie(rng, int(rng.integers(600, 1001)), int(rng.integers(600, 1001)), int(rng.integers(50, 400))))
    exp = oracle_all(pool, CRISPRESSO)
    assert sum(e is not None for e in exp) >= 150 and all(e is not None for e in exp[600:])
    idx = rng.integers(0, len(pool), n)
    short_after_long = sum(idx[i] >= 600 and idx[i + stride] < 600 for i in range(n - stride))
    n_comb = sum(exp[j] is not None for j in idx)
    print(f"batch of {n} pairs over {stride} wavefronts: {n_comb} combined, "
          f"{short_after_long} short pairs after a long one in the same wavefront")
    assert short_after_long >= 50
    pairs = [pool[j] for j in idx]
    first = gpu_merge(pairs, CRISPRESSO)
    again = gpu_merge(pairs, CRISPRESSO)
    assert len(first.length) == n
    for i, j in enumerate(idx):
        assert first.merged(i) == exp[j], f"pair {i} (pool entry {j})"
    assert np.array_equal(first.length, again.length) and np.array_equal(first.flags, again.flags)
    for i in range(n):   # bytes outside a pair's merged range are not specified
        assert again.merged(i) == first.merged(i), f"second call, pair {i}"


# ---- J. the C ABI's refusals and the empty batch ----

@pytest.mark.gpu
def test_gpu_merge_refusals_and_empty_batch():
    res = merge_pairs([], [], [], [])
    assert isinstance(res, MergeResult) and res.length.shape == (0,) and res.flags.shape == (0,)
    lib = _lib.load()
    s = np.frombuffer(b"ACGTACGTAC", np.uint8)
    q = np.frombuffer(b"IIIIIIIIII", np.uint8)
    good = np.array([0, 5, 10], np.int64)
    cases = [((np.array([1, 5, 10], np.int64), good), FlashOptions(), "offsets must start at 0"),
             ((good, np.array([1, 5, 10], np.int64)), FlashOptions(), "offsets must start at 0"),
             ((np.array([0, 7, 5], np.int64), good), FlashOptions(), "offsets not ascending"),
             ((good, good), FlashOptions(min_overlap=0), "min_overlap and max_overlap must be >= 1"),
             ((good, good), FlashOptions(max_overlap=0), "min_overlap and max_overlap must be >= 1")]
    for (off1, off2), opts, message in cases:
        with pytest.raises(FlashError, match="nwf_merge_batch: " + message):
            merge_packed(s, q, off1, s, q, off2, opts)
        assert lib.nwf_last_error().decode().startswith("nwf_merge_batch")
    # a refusal leaves the library usable
    assert merge_packed(s, q, good, s, q, good).length.shape == (2,)
