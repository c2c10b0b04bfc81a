"""The steps kernel (crispresso_amd/csrc/trim_steps.hip, nwt_trim_program) against the restatement
tests/trim_steps_model.py: every read's start and keep, exactly.  Edge lengths at the lane, dword
per lane and strip borders with planted quality patterns, each step alone and each ordered pair;
state carried across steps; the reference's test1 pairs and synthetic pairs with and without
ILLUMINACLIP; single-end; batch sizes around the launch cap; the program and read limits; the
output files of both file modes."""
import ctypes
import functools
import gzip
import os

import numpy as np
import pytest

from crispresso_amd import _lib
from crispresso_amd.trim import (TrimError, TrimProgram, TrimStep, UnsupportedTrimStep, run_trimmomatic_pe,
                                 run_trimmomatic_se, trim_program_pairs)
from tests import trim_steps_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FASTA = os.path.join(GOLDEN, "NexteraPE-PE.fa")
FASTA_SE = os.path.join(GOLDEN, "TruSeq3-SE.fa")
CLIP = "ILLUMINACLIP:" + FASTA + ":0:90:10:0:true"
CLIP_SE = "ILLUMINACLIP:" + FASTA_SE + ":0:90:10:0:true"
CHAIN_A = "LEADING:3 TRAILING:3 SLIDINGWINDOW:4:15 MINLEN:36"
CHAIN_B = "TRAILING:20 LEADING:20 SLIDINGWINDOW:5:25.5 AVGQUAL:33 MINLEN:50"

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
A1 = b"CTGTCTCTTATACACATCTCCGAGCCCACGAGAC"  # what read 1 runs into (Nextera)
A2 = b"CTGTCTCTTATACACATCTGACGCTGCCGACGA"   # what read 2 runs into
TRUSEQ = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"

pytestmark = pytest.mark.gpu


def synth_pairs(n, seed):
    """The generator of tests/test_trim.py, restated: short fragments read through into the
    adapters, an adapter in read 1 only, long fragments, unrelated mates; qualities 2..41."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ACGT = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda k: bytes(rng.choice(ACGT, k))  # noqa: E731
    out = []
    for k in range(n):
        kind = k % 6
        L1 = int(rng.integers(8, 152))
        L2 = int(rng.integers(8, 152))
        if kind in (0, 1, 2):
            f = rnd(int(rng.integers(0, 140)))
            if kind == 0:
                L1 = L2 = 151
            r1 = bytearray((f + A1 + rnd(160))[:L1])
            r2 = bytearray((f[::-1].translate(COMP) + A2 + rnd(160))[:L2])
        elif kind == 3:
            r1 = bytearray(rnd(L1))
            r2 = bytearray(rnd(L2))
            p = int(rng.integers(0, L1))
            r1[p:] = (A1 + rnd(160))[:L1 - p]
        elif kind == 4:
            f = rnd(int(rng.integers(160, 320)))
            r1 = bytearray(f[:L1])
            r2 = bytearray(f[::-1].translate(COMP)[:L2])
        else:
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


def sequencer_qualities(pairs, seed):
    """The same reads with qualities as a sequencer gives them: 20..40, and in 30 % of the reads
    2..12 from a random position in the last third to the end."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def qual(n):
        q = rng.integers(20, 41, n).astype(np.uint8)
        if n and rng.random() < 0.3:
            p = int(rng.integers(2 * n // 3, n))
            q[p:] = rng.integers(2, 13, n - p)
        return bytes(q + 33)
    return [(s1, qual(len(s1)), s2, qual(len(s2))) for s1, _, s2, _ in pairs]


def gpu_windows(steps, pairs, single_end=False):
    prog = steps if isinstance(steps, TrimProgram) else TrimProgram.from_steps(steps)
    s1, q1, s2, q2 = ([p[i] for p in pairs] for i in range(4))
    return trim_program_pairs(s1, q1, None if single_end else s2, None if single_end else q2, prog)


def assert_windows(w, exp1, exp2, what):
    for mate, start, keep, exp in ((1, w.start1, w.keep1, exp1), (2, w.start2, w.keep2, exp2)):
        if exp is None:
            assert start is None and keep is None
            continue
        es, ek = m.windows(exp)
        bad = np.flatnonzero((start != es) | (keep != ek))
        assert bad.size == 0, (f"{what}: read {mate} differs at {bad[:8]}: start {start[bad[:8]]} keep {keep[bad[:8]]}"
                               f" != start {es[bad[:8]]} keep {ek[bad[:8]]}")


def check(steps, pairs, what=None, single_end=False):
    e1, e2 = m.run_pairs(steps, pairs, single_end)
    w = gpu_windows(steps, pairs, single_end)
    assert_windows(w, e1, None if single_end else e2, what or str(steps))
    return e1, e2, w


# ---- edge lengths ----

LENGTHS = [0, 1, 2, 3, 4, 5, 6, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096]   # w - 1, w, w + 1 for w = 4 and 5
STEPS = ["LEADING:20", "TRAILING:20", "SLIDINGWINDOW:4:15", "SLIDINGWINDOW:5:25.5", "CROP:60", "HEADCROP:3",
         "AVGQUAL:20", "MINLEN:5"]


@functools.lru_cache(maxsize=None)
def edge_reads():
    """(sequence, quality line) of every length under every planted pattern."""
    rng = np.random.Generator(np.random.PCG64(23))
    ACGT = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for L in LENGTHS:
        seq = bytes(rng.choice(ACGT, L))
        pats = [rng.integers(0, 42, L)]                           # random
        pats.append(np.full(L, 2))                                # all bad
        only_first = np.full(L, 2)
        only_first[:1] = 40
        pats.append(only_first)                                   # only base 0 good
        only_last = np.full(L, 2)
        only_last[L - 1:] = 40
        pats.append(only_last)                                    # only the last base good
        pats.append(np.full(L, 15))                               # every window of 4 totals R = 60 exactly
        last4 = np.full(L, 15)
        last4[L - 1:] = 14
        pats.append(last4)                                        # only the last window of 4 fails
        last5 = np.full(L, 26)
        last5[L - 1:] = 22
        pats.append(last5)                                        # only the last window of 5 fails (126 < 127.5)
        pats.append(np.where(np.arange(L) % 2 == 0, 26, 25))      # windows of 5 total 128, 127, 128, ...
        one = np.full(L, 14)
        one[:1] = 93
        pats.append(one)                                          # the walk back goes down to one base
        tail = rng.integers(20, 42, L)
        if L:
            p = int(rng.integers(2 * L // 3, L))
            tail[p:] = rng.integers(2, 13, L - p)
        pats.append(tail)                                         # a sequencer's bad tail
        for q in pats:
            out.append((seq, bytes(np.asarray(q, np.uint8) + 33)))
        with_n = bytearray(seq)
        if L >= 3:
            with_n[L // 2] = ord("N")
            with_n[L // 3] = ord("n")
        out.append((bytes(with_n), bytes([40 + 33]) * L))         # N and n at Q40 inside a window
        head = rng.integers(0, 20, L)
        head[L // 2:] = rng.integers(20, 42, L - L // 2)
        out.append((bytes(with_n), bytes(np.asarray(head, np.uint8) + 33)))   # a bad head: LEADING moves far
    return out


@functools.lru_cache(maxsize=None)
def edge_zq():
    return [m.zero_n(s, q) for s, q in edge_reads()]


@functools.lru_cache(maxsize=None)
def edge_step(step, k, rec):
    return m.apply_step(step, edge_zq()[k], rec)


def edge_expected(steps):
    out = []
    for k, (s, _) in enumerate(edge_reads()):
        rec = (0, len(s))
        for st in steps:
            if rec is None:
                break
            rec = edge_step(st, k, rec)
        out.append(rec)
    return out


@pytest.mark.parametrize("first", STEPS)
def test_gpu_steps_edge_lengths(first):
    """`first` alone, then followed by every step; the reads as mate 1 and, in reverse order, as mate 2."""
    reads = edge_reads()
    pairs = [(a[0], a[1], b[0], b[1]) for a, b in zip(reads, reads[::-1])]
    for steps in [[first]] + [[first, second] for second in STEPS]:
        exp = edge_expected(tuple(steps))
        w = gpu_windows(steps, pairs)
        assert_windows(w, exp, exp[::-1], " ".join(steps))
    alone = edge_expected((first,))
    assert any(r is not None for r in alone) and (first.startswith("CROP") or any(r is None for r in alone))


def test_gpu_steps_state_across_steps():
    reads = edge_reads()
    pairs = [(a[0], a[1], b[0], b[1]) for a, b in zip(reads, reads[::-1])]
    progs = ["HEADCROP:7 LEADING:20 TRAILING:20 SLIDINGWINDOW:4:15 AVGQUAL:20",
             "LEADING:30 SLIDINGWINDOW:5:25.5 TRAILING:30 SLIDINGWINDOW:4:15",
             "HEADCROP:70 SLIDINGWINDOW:4:15 SLIDINGWINDOW:5:25.5 LEADING:40 TRAILING:40",
             "HEADCROP:1 HEADCROP:1 CROP:300 SLIDINGWINDOW:64:20 SLIDINGWINDOW:300:10 MINLEN:2",
             "SLIDINGWINDOW:4:35 AVGQUAL:39",       # an N at Q40 fails its windows, an n does not
             "MINLEN:70 CROP:10",                   # a drop in the middle, then CROP
             "AVGQUAL:25 CROP:3 LEADING:2",
             "CROP:0 MINLEN:0 AVGQUAL:40 CROP:5"]   # a live record of length 0
    for prog in progs:
        steps = tuple(prog.split())
        exp = edge_expected(steps)
        assert_windows(gpu_windows(prog, pairs), exp, exp[::-1], prog)
        live = [r for r in exp if r is not None]
        assert live and (len(live) < len(exp) or prog.startswith("CROP:0")), prog
        if prog.startswith(("HEADCROP", "LEADING")):
            assert sum(r[0] > 0 for r in live) >= 5, prog   # later scans ran on a moved start
    assert all(r == (0, 0) for r in edge_expected(tuple(progs[-1].split())) if r is not None)


# ---- real and synthetic pairs ----

@functools.lru_cache(maxsize=None)
def golden_pairs():
    r1 = m.read_fastq(os.path.join(GOLDEN, "test1_L001_R1_001.fastq.gz"))[:1000]
    r2 = m.read_fastq(os.path.join(GOLDEN, "test1_L001_R2_001.fastq.gz"))[:1000]
    return [(a[1], a[2], b[1], b[2]) for a, b in zip(r1, r2)]


@functools.lru_cache(maxsize=None)
def synth600():
    return synth_pairs(600, 7)


@functools.lru_cache(maxsize=None)
def synth600_expected():
    return m.run_pairs(CLIP + " " + CHAIN_A, synth600())


def survivors(e1, e2):
    both = sum(x is not None and y is not None for x, y in zip(e1, e2))
    fwd = sum(x is not None and y is None for x, y in zip(e1, e2))
    rev = sum(x is None and y is not None for x, y in zip(e1, e2))
    return both, fwd, rev, len(e1) - both - fwd - rev


@pytest.mark.parametrize("chain", [CHAIN_A, CHAIN_B])
def test_gpu_steps_golden_pairs(chain):
    e1, e2, w = check(chain, golden_pairs())
    assert w.kernel_ms_clip == 0.0 and w.kernel_ms_steps > 0.0
    if chain == CHAIN_B:
        assert sum(r is not None and r[0] > 0 for r in e1) == 29
        assert sum(r is not None and r[0] > 0 for r in e2) == 21


def test_gpu_clip_then_steps_golden_pairs():
    e1, e2, w = check(CLIP + " " + CHAIN_A, golden_pairs())
    assert survivors(e1, e2) == (845, 21, 51, 83)
    assert w.kernel_ms_clip > 0.0 and w.kernel_ms_steps > 0.0


def test_gpu_clip_then_steps_synthetic_pairs():
    e1, e2 = synth600_expected()
    assert_windows(gpu_windows(CLIP + " " + CHAIN_A, synth600()), e1, e2, "synthetic 600")
    assert min(survivors(e1, e2)) > 0
    # the same reads with a sequencer's qualities, so that the clip and the window both decide
    pairs = sequencer_qualities(synth600()[:300], 31)
    e1, e2, _ = check(CLIP + " " + CHAIN_A, pairs)
    c1, _ = m.run_pairs(CLIP, pairs)
    n1, _ = m.run_pairs(CHAIN_A, pairs)
    assert sum(a != b for a, b in zip(e1, c1)) >= 30 and sum(a != b for a, b in zip(e1, n1)) >= 30


def test_gpu_steps_single_end():
    rng = np.random.Generator(np.random.PCG64(41))
    ACGT = np.frombuffer(b"ACGT", np.uint8)
    reads = []
    for k in range(300):
        L = int(rng.integers(30, 152))
        r = bytes(rng.choice(ACGT, L))
        if k % 3 == 0:   # the TruSeq adapter from a random position on
            p = int(rng.integers(0, L))
            r = (r[:p] + TRUSEQ + bytes(rng.choice(ACGT, 160)))[:L]
        reads.append((r, b"", b"", b""))
    pairs = sequencer_qualities(reads, 43)
    prog = CLIP_SE + " " + CHAIN_A
    e1, _, w = check(prog, pairs, single_end=True)
    assert w.start2 is None and w.keep2 is None
    c1, _ = m.run_pairs(CLIP_SE, pairs, single_end=True)
    assert sum(r is None or r[1] < len(p[0]) for r, p in zip(c1, pairs)) >= 60   # the clip acts
    assert sum(a != b for a, b in zip(e1, c1)) >= 60                             # and so do the steps
    check(CHAIN_B, pairs, single_end=True)


def test_gpu_steps_batch_sizes():
    try:
        import torch
        cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        cus = 256
    pool = synth600()
    e1, e2 = synth600_expected()
    prog = TrimProgram.from_steps(CLIP + " " + CHAIN_A)
    for count in (1, 257):
        w = gpu_windows(prog, pool[:count])
        assert len(w.keep1) == count and len(w.keep2) == count
        assert_windows(w, e1[:count], e2[:count], f"batch of {count}")
    n = 2 * (4 * 16 * cus) + 5   # more reads than the capped grid has wavefronts, per mate
    idx = np.random.Generator(np.random.PCG64(17)).integers(0, 600, n)
    w = gpu_windows(prog, [pool[j] for j in idx])
    assert len(w.keep1) == n
    assert_windows(w, [e1[j] for j in idx], [e2[j] for j in idx], f"batch of {n}")
    # the steps kernel alone on the same batch
    f1, f2 = m.run_pairs(CHAIN_B, pool)
    w = gpu_windows(CHAIN_B, [pool[j] for j in idx])
    assert_windows(w, [f1[j] for j in idx], [f2[j] for j in idx], f"batch of {n}, no clip")


def test_gpu_steps_maximum_program():
    pairs = sequencer_qualities(synth600()[:100], 47)
    steps = ["HEADCROP:1", "LEADING:21", "CROP:140", "TRAILING:21", "SLIDINGWINDOW:6:24.5", "HEADCROP:2",
             "SLIDINGWINDOW:4:15", "AVGQUAL:25", "CROP:120", "LEADING:30", "TRAILING:30", "SLIDINGWINDOW:10:28",
             "HEADCROP:1", "MINLEN:20", "CROP:90", "AVGQUAL:30"]
    assert len(steps) == 16
    e1, e2, _ = check(" ".join(steps), pairs)
    assert 10 <= sum(r is not None for r in e1) <= 90
    prog = TrimProgram(None, [TrimStep("CROP", 100)] * 17)
    s1, q1, s2, q2 = ([p[i] for p in pairs[:4]] for i in range(4))
    with pytest.raises(UnsupportedTrimStep, match="16"):
        trim_program_pairs(s1, q1, s2, q2, prog)
    # and the library's own check
    lib = _lib.load()
    arr = (_lib.NwtStep * 17)(*[_lib.NwtStep(4, 100, 0.0, 0.0)] * 17)
    seq = np.frombuffer(b"ACGT", np.uint8).copy()
    qual = np.frombuffer(b"IIII", np.uint8).copy()
    off = np.array([0, 4], np.int64)
    start, keep = np.zeros(1, np.int32), np.zeros(1, np.int32)
    args = (_lib.ptr(seq), _lib.ptr(qual), _lib.ptr(off), None, None, None, 1, _lib.ptr(start), _lib.ptr(keep), None,
            None, (ctypes.c_float * 2)())
    assert lib.nwt_trim_program(0, None, None, None, None, 0, None, None, 0, arr, 17, *args) == -1
    assert lib.nwt_last_error().decode().startswith("nwt_trim_program: more than 16 steps")
    assert lib.nwt_trim_program(0, None, None, None, None, 0, None, None, 0, arr, 16, *args) == 0
    assert (int(start[0]), int(keep[0])) == (0, 4)


def test_gpu_steps_refusals():
    prog = TrimProgram.from_steps(CHAIN_A)
    with pytest.raises(TrimError, match="4096"):
        trim_program_pairs([b"A" * 4097], [b"I" * 4097], None, None, prog)
    with pytest.raises(TrimError, match="quality"):
        trim_program_pairs([b"ACGT" * 10], [b"I" * 39 + b" "], [b"ACGT" * 10], [b"I" * 40], prog)
    with pytest.raises(TrimError, match="quality"):
        trim_program_pairs([b"ACGT" * 10], [b"I" * 40], [b"ACGT" * 10], [b"\x7f" + b"I" * 39], prog)
    assert _lib.load().nwt_last_error().decode().startswith("nwt_trim_program")
    w = trim_program_pairs([b"A" * 4096], [b"I" * 4096], None, None, prog)
    assert (int(w.start1[0]), int(w.keep1[0])) == (0, 4096)


# ---- files ----

def write_fastq(path, pairs, si, qi, tag):
    with open(path, "wb") as f:
        for i, p in enumerate(pairs):
            f.write(b"@read%d/%s\n%s\n+\n%s\n" % (i, tag, p[si], p[qi]))


def same_file(a, b):
    op = gzip.open if a.endswith(".gz") else open
    with op(a, "rb") as fa, op(b, "rb") as fb:
        x, y = fa.read(), fb.read()
    assert x == y, a
    return len(x)


def test_gpu_run_trimmomatic_pe_files_match_the_model(tmp_path):
    pairs = sequencer_qualities(synth_pairs(300, 5), 53)
    write_fastq(tmp_path / "r1.fastq", pairs, 0, 1, b"1")
    write_fastq(tmp_path / "r2.fastq", pairs, 2, 3, b"2")
    steps = [CLIP, "HEADCROP:2"] + CHAIN_A.split()
    names = ("fp.fq.gz", "fu.fq", "rp.fq.gz", "ru.fq.gz")
    gpu = [str(tmp_path / ("gpu_" + n)) for n in names]
    cpu = [str(tmp_path / ("cpu_" + n)) for n in names]
    st_gpu = run_trimmomatic_pe(str(tmp_path / "r1.fastq"), str(tmp_path / "r2.fastq"), gpu, " ".join(steps))
    st_cpu = m.run_pe(str(tmp_path / "r1.fastq"), str(tmp_path / "r2.fastq"), cpu, steps)
    assert st_gpu == st_cpu and st_cpu["pairs"] == 300
    assert min(st_cpu["both"], st_cpu["fwd_only"], st_cpu["rev_only"], st_cpu["dropped"]) > 0
    for a, b in zip(gpu, cpu):
        assert same_file(a, b) > 0


def test_gpu_run_trimmomatic_se_file_matches_the_model(tmp_path):
    pairs = sequencer_qualities(synth_pairs(300, 9), 59)
    write_fastq(tmp_path / "r1.fastq", pairs, 0, 1, b"1")
    steps = CLIP_SE + " LEADING:3 TRAILING:3 SLIDINGWINDOW:4:15 MINLEN:36"
    for name in ("reads.trimmed.fq.gz", "reads.trimmed.fq"):
        gpu, cpu = str(tmp_path / ("gpu_" + name)), str(tmp_path / ("cpu_" + name))
        st_gpu = run_trimmomatic_se(str(tmp_path / "r1.fastq"), gpu, steps)
        st_cpu = m.run_se(str(tmp_path / "r1.fastq"), cpu, steps.split())
        assert st_gpu == st_cpu and st_cpu["reads"] == 300
        assert st_cpu["surviving"] > 0 and st_cpu["dropped"] > 0
        assert same_file(gpu, cpu) > 0
    with open(str(tmp_path / "gpu_reads.trimmed.fq.gz"), "rb") as f:
        assert f.read(2) == b"\x1f\x8b"
