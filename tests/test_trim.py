"""GPU adapter trimming (crispresso_amd/trim.py, csrc/trim_clip.hip) against the Trimmomatic 0.33
restatement (oracle/trimmomatic_oracle.py): every read's keep length after ILLUMINACLIP + MINLEN on
the reference's own test1 pairs, on seeded synthetic pairs under four ILLUMINACLIP settings, on pairs
built to sit on either side of the palindrome threshold, on hand-written edge cases, single-end, the
four output files, and the chain trim -> merge against the pinned e2e fixture."""
import functools
import gzip
import json
import os
import sys

import numpy as np
import pytest

from crispresso_amd import _lib
from crispresso_amd.trim import (TrimError, TrimOptions, UnsupportedTrimStep, run_trimmomatic_pe, trim_pairs)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import trimmomatic_oracle as tmo  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
FASTA = os.path.join(GOLDEN, "NexteraPE-PE.fa")
DEFAULT = ":0:90:10:0:true"
SPECS = [DEFAULT, ":2:30:10", ":1:30:7:1:false", ":0:12:4:8:true"]
NEVER = sys.maxsize

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
A1 = b"CTGTCTCTTATACACATCTCCGAGCCCACGAGAC"  # what read 1 runs into
A2 = b"CTGTCTCTTATACACATCTGACGCTGCCGACGA"   # what read 2 runs into


def synth_pairs(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    ACGT = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda k: bytes(rng.choice(ACGT, k))  # noqa: E731
    out = []
    for k in range(n):
        kind = k % 6
        L1 = int(rng.integers(8, 152))
        L2 = int(rng.integers(8, 152))
        if kind in (0, 1, 2):                      # short fragment, both reads reach the adapters
            f = rnd(int(rng.integers(0, 140)))
            if kind == 0:
                L1 = L2 = 151
            r1 = bytearray((f + A1 + rnd(160))[:L1])
            r2 = bytearray((f[::-1].translate(COMP) + A2 + rnd(160))[:L2])
        elif kind == 3:                            # adapter in read 1 only
            r1 = bytearray(rnd(L1))
            r2 = bytearray(rnd(L2))
            p = int(rng.integers(0, L1))
            r1[p:] = (A1 + rnd(160))[:L1 - p]
        elif kind == 4:                            # long fragment
            f = rnd(int(rng.integers(160, 320)))
            r1 = bytearray(f[:L1])
            r2 = bytearray(f[::-1].translate(COMP)[:L2])
        else:                                      # unrelated mates
            r1 = bytearray(rnd(L1))
            r2 = bytearray(rnd(L2))
        q1 = rng.integers(2, 42, len(r1)).astype(np.uint8)
        q2 = rng.integers(2, 42, len(r2)).astype(np.uint8)
        nerr = int(rng.integers(0, 5)) if kind != 2 else int(rng.integers(4, 14))
        for r in (r1, r2):
            for _ in range(nerr):
                if len(r):
                    r[int(rng.integers(0, len(r)))] = b"ACGTN"[int(rng.integers(0, 5))]
        out.append((bytes(r1), bytes(q1 + 33), bytes(r2), bytes(q2 + 33)))
    return out


def oracle_clip(clip, pairs, single_end=False):
    """IlluminaClip.process on every pair -> the clipped lengths (0 = dropped), before MINLEN, and how
    often each test fired: palindrome hits, read-1 / read-2 simple-mode clips, reads 2 dropped."""
    pal, simple = [], []
    for pp in clip.pairs:
        pp.compare = (lambda *a, _f=pp.compare: (pal.append(_f(*a)), pal[-1])[1])
    for cs in clip.fwd + clip.rev + clip.com:
        cs.compare = (lambda *a, _f=cs.compare: (simple.append(_f(*a)), simple[-1])[1])
    n_r1 = len(clip.fwd) + len(clip.com)
    k1, k2 = [], []
    counts = dict(palindrome=0, simple1=0, simple2=0, dropped2=0)
    for s1, q1, s2, q2 in pairs:
        del pal[:], simple[:]
        a = ("r", s1.decode(), q1.decode())
        b = None if single_end else ("r", s2.decode(), q2.decode())
        ca, cb = clip.process(a, b)
        k1.append(0 if ca is None else len(ca[1]))
        k2.append(0 if cb is None else len(cb[1]))
        counts["palindrome"] += any(x != NEVER for x in pal)
        counts["simple1"] += any(x != NEVER for x in simple[:n_r1])
        counts["simple2"] += any(x != NEVER for x in simple[n_r1:])
        counts["dropped2"] += (not single_end) and cb is None
    for x in clip.pairs + clip.fwd + clip.rev + clip.com:
        del x.compare
    return np.array(k1, np.int32), np.array(k2, np.int32), counts


def minlen_applied(k, minlen):
    k = k.copy()
    k[k < minlen] = 0
    return k


def gpu_keeps(pairs, spec, minlen, single_end=False):
    steps = ["ILLUMINACLIP:" + FASTA + spec] + ([f"MINLEN:{minlen}"] if minlen else [])
    o = TrimOptions.from_steps(steps)
    s1, q1, s2, q2 = ([p[i] for p in pairs] for i in range(4))
    return trim_pairs(s1, q1, None if single_end else s2, None if single_end else q2, o)


def assert_same(res, exp1, exp2, what):
    d1 = np.flatnonzero(res.keep1 != exp1)
    assert d1.size == 0, f"{what}: read 1 differs at {d1[:10]}: {res.keep1[d1[:10]]} != {exp1[d1[:10]]}"
    if exp2 is not None:
        d2 = np.flatnonzero(res.keep2 != exp2)
        assert d2.size == 0, f"{what}: read 2 differs at {d2[:10]}: {res.keep2[d2[:10]]} != {exp2[d2[:10]]}"


@functools.lru_cache(maxsize=None)
def synth600():
    return synth_pairs(600, 7)


@functools.lru_cache(maxsize=None)
def synth600_oracle(spec):
    return oracle_clip(tmo.IlluminaClip(FASTA + spec), synth600())


# ---- CPU ----

def test_trim_symbols_exported():
    syms = _lib.exported_symbols()
    assert all(syms[s] for s in _lib.TRIM_EXPORTS)


def test_trim_header_declares_the_exports():
    with open(os.path.join(ROOT, "include", "crispr_trim.h")) as f:
        text = f.read()
    for s in _lib.TRIM_EXPORTS:
        assert f" {s}(" in text


def test_default_options_string():
    o = TrimOptions.from_steps("ILLUMINACLIP:" + FASTA + ":0:90:10:0:true MINLEN:40")
    assert len(o.prefix_pairs) == 1 and [len(p) for p in o.prefix_pairs[0]] == [19, 19]
    assert len(o.common_adapters) == 4 and len(o.adapters) == 4
    assert (o.seed_mismatches, o.palindrome_threshold, o.simple_threshold) == (0, 90, 10)
    assert o.min_prefix == 0 and o.keep_both is True and o.minlen == 40
    as_list = TrimOptions.from_steps(["ILLUMINACLIP:" + FASTA + ":0:90:10:0:true", "MINLEN:40"])
    assert as_list == o
    assert TrimOptions.from_steps("ILLUMINACLIP:" + FASTA + ":2:30:10").min_prefix == 8


def test_other_steps_are_refused():
    with pytest.raises(UnsupportedTrimStep, match="LEADING:3"):
        TrimOptions.from_steps("ILLUMINACLIP:" + FASTA + ":0:90:10:0:true LEADING:3 MINLEN:40")
    assert issubclass(UnsupportedTrimStep, ValueError)


def test_mismatched_inputs_raise():
    o = TrimOptions(minlen=10)
    with pytest.raises(TrimError):
        trim_pairs([b"ACGT", b"ACGT"], [b"IIII", b"IIII"], [b"ACGT"], [b"IIII"], o)
    with pytest.raises(TrimError):
        trim_pairs([b"ACGT"], [b"III"], [b"ACGT"], [b"IIII"], o)


# ---- GPU ----

def read_golden_pairs(limit=None):
    r1 = tmo.read_fastq(os.path.join(GOLDEN, "test1_L001_R1_001.fastq.gz"))
    r2 = tmo.read_fastq(os.path.join(GOLDEN, "test1_L001_R2_001.fastq.gz"))
    out = []
    for a, b in zip(r1, r2):
        out.append((a[1].encode(), a[2].encode(), b[1].encode(), b[2].encode()))
        if limit and len(out) == limit:
            break
    return out


@pytest.mark.gpu
def test_gpu_trim_matches_oracle_real_pairs():
    pairs = read_golden_pairs(1000)
    assert len(pairs) == 1000
    k1, k2, counts = oracle_clip(tmo.IlluminaClip(FASTA + DEFAULT), pairs)
    print(counts)
    assert counts["simple1"] >= 100 and counts["simple2"] >= 40
    res = gpu_keeps(pairs, DEFAULT, 40)
    assert_same(res, minlen_applied(k1, 40), minlen_applied(k2, 40), "test1")


@pytest.mark.gpu
@pytest.mark.parametrize("minlen", [0, 40])
@pytest.mark.parametrize("spec", SPECS)
def test_gpu_trim_matches_oracle_synthetic(spec, minlen):
    k1, k2, counts = synth600_oracle(spec)
    print(spec, counts)
    assert counts["palindrome"] >= (10 if spec == DEFAULT else 100)
    assert counts["simple1"] >= 150 and counts["simple2"] >= 100 and counts["dropped2"] >= 1
    res = gpu_keeps(synth600(), spec, minlen)
    assert_same(res, minlen_applied(k1, minlen), minlen_applied(k2, minlen), f"{spec} MINLEN {minlen}")


def near_threshold_pairs(spec, n=40, seed=3):
    """Error-free short-fragment pairs, read 1 damaged one base at a time in the fragment's second
    half until PrefixPair.compare first stops hitting: the last hitting and the first non-hitting
    version of each pair -> (pairs, hits among them)."""
    clip = tmo.IlluminaClip(FASTA + spec)
    pp = clip.pairs[0]
    rng = np.random.Generator(np.random.PCG64(seed))
    ACGT = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda k: bytes(rng.choice(ACGT, k))  # noqa: E731
    out, hits = [], 0
    for _ in range(n):
        L = int(rng.integers(115, 140))
        f = rnd(L)
        r1 = bytearray((f + A1 + rnd(160))[:151])
        r2 = (f[::-1].translate(COMP) + A2 + rnd(160))[:151]
        q1 = bytes(rng.integers(2, 42, 151).astype(np.uint8) + 33)
        q2 = bytes(rng.integers(2, 42, 151).astype(np.uint8) + 33)
        ql1, ql2 = [c - 33 for c in q1], [c - 33 for c in q2]
        s2 = r2.decode()
        if pp.compare(r1.decode(), ql1, s2, ql2) == NEVER:
            continue
        for pos in rng.permutation(np.arange(L // 2, L)):
            last = bytes(r1)
            r1[pos] = b"ACGT"[(b"ACGT".index(r1[pos]) + int(rng.integers(1, 4))) % 4]
            if pp.compare(r1.decode(), ql1, s2, ql2) == NEVER:
                out.append((last, q1, r2, q2))
                out.append((bytes(r1), q1, r2, q2))
                hits += 1
                break
    return out, hits


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [DEFAULT, ":2:30:10:1:true"])
def test_gpu_trim_near_the_palindrome_threshold(spec):
    pairs, hits = near_threshold_pairs(spec)
    print(spec, len(pairs), hits)
    assert hits >= 25 and len(pairs) - hits >= 25
    k1, k2, _ = oracle_clip(tmo.IlluminaClip(FASTA + spec), pairs)
    for minlen in (0, 40):
        res = gpu_keeps(pairs, spec, minlen)
        assert_same(res, minlen_applied(k1, minlen), minlen_applied(k2, minlen), f"{spec} MINLEN {minlen}")


@pytest.mark.gpu
def test_gpu_trim_edges():
    rng = np.random.Generator(np.random.PCG64(11))
    ACGT = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda k: bytes(rng.choice(ACGT, k))  # noqa: E731
    q = lambda s, v=30: bytes([33 + v]) * len(s)  # noqa: E731
    ad = A2                                        # Trans1_rc, a common adapter of the FASTA
    filler = rnd(100)
    seqs = [
        (b"", filler),                             # an empty read
        (filler, b""),
        (rnd(15), rnd(16)),                        # reads of 15 and 16 bases
        (rnd(16), rnd(15)),
        (ad, filler),                              # a read equal to an adapter: keep 0, dropped
        (filler, ad),
        (ad[5:] + rnd(60), filler),                # the adapter from its 6th base: negative offset, dropped
        (b"N" * 80, b"N" * 151),                   # all N
        (rnd(151), rnd(37)),                       # mates of unequal length
        (rnd(70) + ad[:20], rnd(40) + ad),         # adapter tails at the 3' end
        (rnd(140) + ad[:11], rnd(146) + ad[:5]),
    ]
    f = rnd(60)                                    # a short fragment read through, mates of unequal length
    seqs.append(((f + A1 + rnd(80))[:151], (f[::-1].translate(COMP) + A2 + rnd(80))[:120]))
    pairs = [(a, q(a), b, q(b, 12)) for a, b in seqs]
    clip = tmo.IlluminaClip(FASTA + DEFAULT)
    k1, k2, _ = oracle_clip(clip, pairs)
    assert k1[4] == 0 and k2[5] == 0 and k1[6] == 0 and k1[-1] == 60 and k2[-1] == 60
    for minlen in (0, 40):
        res = gpu_keeps(pairs, DEFAULT, minlen)
        assert_same(res, minlen_applied(k1, minlen), minlen_applied(k2, minlen), f"edges MINLEN {minlen}")
    # a single-pair batch, and one that is no multiple of the block's pairs
    e1, e2, _ = synth600_oracle(DEFAULT)
    for count in (1, 257):
        res = gpu_keeps(synth600()[:count], DEFAULT, 0)
        assert len(res.keep1) == count
        assert_same(res, e1[:count], e2[:count], f"batch of {count}")


@pytest.mark.gpu
def test_gpu_trim_long_reads():
    """Reads in the thousands of bases (up to the 4096 limit) take the kernel's one-wave-per-block
    launch; the short pairs of the same batch go with them."""
    rng = np.random.Generator(np.random.PCG64(13))
    ACGT = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda k: bytes(rng.choice(ACGT, k))  # noqa: E731
    q = lambda s: bytes(rng.integers(2, 42, len(s)).astype(np.uint8) + 33)  # noqa: E731
    f = rnd(1500)
    seqs = [((f + A1 + rnd(600))[:2000], (f[::-1].translate(COMP) + A2 + rnd(600))[:1800]),
            (rnd(4000) + (A1 + rnd(96))[:96], rnd(4096)),
            (rnd(1700), rnd(3000) + A2[:14])]
    pairs = [(a, q(a), b, q(b)) for a, b in seqs] + synth600()[:9]
    k1, k2, counts = oracle_clip(tmo.IlluminaClip(FASTA + DEFAULT), pairs)
    assert (k1[0], k2[0], k1[1], k2[1], k1[2], k2[2]) == (1500, 1500, 4000, 4096, 1700, 3014)
    assert counts["palindrome"] >= 1
    res = gpu_keeps(pairs, DEFAULT, 40)
    assert_same(res, minlen_applied(k1, 40), minlen_applied(k2, 40), "long reads")


@pytest.mark.gpu
def test_gpu_trim_batch_larger_than_the_grid():
    """The launch is capped at 16 blocks of 4 wavefronts per CU: in a larger batch a wavefront clips a
    second and a third pair over the LDS bytes its previous pair left behind."""
    try:
        import torch
        cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        cus = 256
    n = 2 * (4 * 16 * cus) + 5
    assert n > 4 * 16 * cus
    e1, e2, _ = synth600_oracle(DEFAULT)
    idx = np.random.Generator(np.random.PCG64(17)).integers(0, 600, n)
    pool = synth600()
    pairs = [pool[j] for j in idx]
    for minlen in (0, 40):
        res = gpu_keeps(pairs, DEFAULT, minlen)
        assert len(res.keep1) == n and len(res.keep2) == n
        assert_same(res, minlen_applied(e1[idx], minlen), minlen_applied(e2[idx], minlen),
                    f"batch of {n} MINLEN {minlen}")


@pytest.mark.gpu
def test_gpu_trim_single_end():
    pairs = synth600()
    k1, _, counts = oracle_clip(tmo.IlluminaClip(FASTA + DEFAULT), pairs, single_end=True)
    assert counts["palindrome"] == 0 and counts["simple1"] >= 150
    res = gpu_keeps(pairs, DEFAULT, 40, single_end=True)
    assert res.keep2 is None
    assert_same(res, minlen_applied(k1, 40), None, "single-end")


@pytest.mark.gpu
def test_gpu_run_trimmomatic_pe_files_match_oracle(tmp_path):
    pairs = synth_pairs(300, 5)
    for name, si, qi in (("r1.fastq", 0, 1), ("r2.fastq", 2, 3)):
        with open(tmp_path / name, "wb") as f:
            for i, p in enumerate(pairs):
                f.write(b"@read%d/%s\n%s\n+\n%s\n" % (i, name[1].encode(), p[si], p[qi]))
    steps = ["ILLUMINACLIP:" + FASTA + ":2:30:10:1:false", "MINLEN:40"]
    names = ("fp.fq.gz", "fu.fq", "rp.fq.gz", "ru.fq.gz")
    gpu = [str(tmp_path / ("gpu_" + n)) for n in names]
    cpu = [str(tmp_path / ("cpu_" + n)) for n in names]
    st_gpu = run_trimmomatic_pe(str(tmp_path / "r1.fastq"), str(tmp_path / "r2.fastq"), gpu, " ".join(steps))
    st_cpu = tmo.run_pe(str(tmp_path / "r1.fastq"), str(tmp_path / "r2.fastq"), cpu, steps)
    assert st_gpu == st_cpu
    assert min(st_cpu["both"], st_cpu["fwd_only"], st_cpu["dropped"]) > 0
    for a, b in zip(gpu, cpu):
        op = gzip.open if a.endswith(".gz") else open
        with op(a, "rb") as fa, op(b, "rb") as fb:
            assert fa.read() == fb.read(), a


@pytest.mark.gpu
def test_gpu_trim_then_merge_reproduces_the_fixture(tmp_path):
    """CORE:1620-1677 on the device: the raw test1 pairs -> run_trimmomatic_pe (default steps) ->
    run_flash (CRISPResso's options) give the pinned fixture's merged reads."""
    from crispresso_amd.flash import FlashOptions, read_fastq, run_flash

    with gzip.open(os.path.join(GOLDEN, "e2e_test1_data.json.gz"), "rt") as f:
        fx = json.load(f)
    outs = [str(tmp_path / f"{n}.fq.gz") for n in ("fp", "fu", "rp", "ru")]
    st = run_trimmomatic_pe(os.path.join(GOLDEN, "test1_L001_R1_001.fastq.gz"),
                            os.path.join(GOLDEN, "test1_L001_R2_001.fastq.gz"), outs,
                            "ILLUMINACLIP:" + FASTA + ":0:90:10:0:true MINLEN:40")
    assert st["pairs"] == 4941
    fl = run_flash(outs[0], outs[2], str(tmp_path / "flash"),
                   options=FlashOptions(min_overlap=4, max_overlap=100, allow_outies=True))
    assert fl["combined"] == 4093
    names, seqs, _ = read_fastq(str(tmp_path / "flash" / "out.extendedFrags.fastq.gz"))
    assert [tuple(x) for x in fx["merged_reads"]] == [(n.decode(), s.decode()) for n, s in zip(names, seqs)]


@pytest.mark.gpu
def test_gpu_trim_refusals():
    ok = TrimOptions.from_steps("ILLUMINACLIP:" + FASTA + DEFAULT)
    short = TrimOptions(simple_threshold=7, adapters=[(b"CTGTCTCTTATACACATCTG", 0)])
    with pytest.raises(TrimError, match="24"):
        trim_pairs([b"ACGT" * 10], [b"I" * 40], [b"ACGT" * 10], [b"I" * 40], short)
    with pytest.raises(TrimError, match="4096"):
        trim_pairs([b"ACGT" * 1250], [b"I" * 5000], [b"ACGT" * 10], [b"I" * 40], ok)
    with pytest.raises(TrimError, match="quality"):
        trim_pairs([b"ACGT" * 10], [b"I" * 39 + b" "], [b"ACGT" * 10], [b"I" * 40], ok)
    lib = _lib.load()
    assert lib.nwt_last_error().decode().startswith("nwt_trim_batch")
