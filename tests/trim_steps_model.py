"""Restatement of Trimmomatic 0.33's quality and crop steps, for the tests of
crispresso_amd/csrc/trim_steps.hip: plain Python, one function per step, float32 through numpy.

A record is ``(start, length)``, a window of its read, or ``None`` (dropped).  ``q[i]`` is the
phred-33 quality of base ``i`` of the window; the steps marked zeroN count the quality of an
upper-case ``N`` as 0.  ILLUMINACLIP is oracle/trimmomatic_oracle.py's ``IlluminaClip`` (the only
step that sees both mates).  Parity with the Java program on these steps is unpinned: no
output of it with them exists in this tree."""
import gzip
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import trimmomatic_oracle as tmo  # noqa: E402

f32 = np.float32


def zero_n(seq, qual):
    """Qualities (byte - 33) of the whole read, 0 where the base is 'N'."""
    return [0 if s == 78 else c - 33 for s, c in zip(seq, qual)]


def leading(q, rec, t):
    start, n = rec
    for i in range(n):
        if q[start + i] >= t:
            return (start + i, n - i)
    return None


def trailing(q, rec, t):
    start, n = rec
    for i in range(n - 1, 0, -1):
        if q[start + i] >= t:
            return (start, i + 1)
    return None


def sliding_window(q, rec, w, r):
    start, n = rec
    r = f32(r)
    need = f32(r * f32(w))
    if n < w:
        return None
    total = sum(q[start:start + w])
    if f32(total) < need:
        return None
    keep = n
    for i in range(n - w):
        total += q[start + i + w] - q[start + i]
        if f32(total) < need:
            keep = i + w
            break
    while f32(q[start + keep - 1]) < r and keep > 1:
        keep -= 1
    return (start, keep)


def crop(rec, n):
    return rec if rec[1] < n else (rec[0], n)


def headcrop(rec, n):
    return None if rec[1] <= n else (rec[0] + n, rec[1] - n)


def avgqual(q, rec, t):
    start, n = rec
    return None if sum(q[start:start + n]) < t * n else rec


def minlen(rec, n):
    return None if rec[1] < n else rec


def apply_step(step, q, rec):
    """One step other than ILLUMINACLIP on a live record."""
    name, _, args = step.partition(":")
    if name == "SLIDINGWINDOW":
        w, r = args.split(":")
        return sliding_window(q, rec, int(w), float(r))
    n = int(args)
    if name == "LEADING":
        return leading(q, rec, n)
    if name == "TRAILING":
        return trailing(q, rec, n)
    if name == "AVGQUAL":
        return avgqual(q, rec, n)
    if name == "CROP":
        return crop(rec, n)
    if name == "HEADCROP":
        return headcrop(rec, n)
    if name == "MINLEN":
        return minlen(rec, n)
    raise ValueError(f"step {step!r} is not restated")


def run_read(steps, seq, qual, rec=None, counts=None):
    """The steps in order on one read (bytes); ``rec`` is the entering record (default: the whole
    read).  ``counts`` = (changed, dropped) lists, one entry per step, counted among the records
    alive when the step runs."""
    q = zero_n(seq, qual)
    if rec is None:
        rec = (0, len(seq))
    for k, st in enumerate(steps):
        if rec is None:
            break
        new = apply_step(st, q, rec)
        if counts is not None:
            if new is None:
                counts[1][k] += 1
            elif new != rec:
                counts[0][k] += 1
        rec = new
    return rec


def split_steps(steps):
    if isinstance(steps, str):
        steps = steps.split()
    return list(steps)


def run_pairs(steps, pairs, single_end=False):
    """``pairs`` = (seq1, qual1, seq2, qual2) bytes tuples -> the records of both mates (read 2's
    are None in single-end mode).  An ILLUMINACLIP step at any position is applied to the pair's
    current records (which must then start at 0)."""
    steps = split_steps(steps)
    clips = {k: tmo.IlluminaClip(st[len("ILLUMINACLIP:"):]) for k, st in enumerate(steps)
             if st.startswith("ILLUMINACLIP:")}
    out1, out2 = [], []
    for s1, q1, s2, q2 in pairs:
        recs = [(0, len(s1)), None if single_end else (0, len(s2))]
        reads = [(s1, q1), (s2, q2)]
        zq = [zero_n(s1, q1), None if single_end else zero_n(s2, q2)]
        for k, st in enumerate(steps):
            if k in clips:
                ab = []
                for rec, (s, q) in zip(recs, reads):
                    if rec is None:
                        ab.append(None)
                    else:
                        assert rec[0] == 0, "ILLUMINACLIP on a window is not restated"
                        ab.append(("r", s[:rec[1]].decode(), q[:rec[1]].decode()))
                ca, cb = clips[k].process(ab[0], ab[1])
                recs = [None if c is None else (0, len(c[1])) for c in (ca, cb)]
            else:
                recs = [None if rec is None else apply_step(st, z, rec) for rec, z in zip(recs, zq)]
        out1.append(recs[0])
        out2.append(recs[1])
    return out1, out2


def windows(recs):
    """Records as the device reports them: int32 start and keep arrays, keep = -1 (start 0) for
    a dropped record."""
    start = np.array([0 if r is None else r[0] for r in recs], np.int32)
    keep = np.array([-1 if r is None else r[1] for r in recs], np.int32)
    return start, keep


def read_fastq(path):
    op = gzip.open if open(path, "rb").read(2) == b"\x1f\x8b" else open
    out = []
    with op(path, "rb") as f:
        while True:
            h = f.readline()
            if not h:
                return out
            s = f.readline().rstrip(b"\n")
            f.readline()
            q = f.readline().rstrip(b"\n")
            out.append((h.rstrip(b"\n")[1:], s, q))


def _open_out(path):
    return gzip.open(path, "wb", compresslevel=1) if path.endswith(".gz") else open(path, "wb")


def _write(f, name, s, q, rec):
    a, n = rec
    f.write(b"@%s\n%s\n+\n%s\n" % (name, s[a:a + n], q[a:a + n]))


def run_pe(r1, r2, outs, steps):
    """Trimmomatic PE's four files (forward paired, forward unpaired, reverse paired, reverse
    unpaired) and its summary counts."""
    a, b = read_fastq(r1), read_fastq(r2)
    n = min(len(a), len(b))
    o1, o2 = run_pairs(steps, [(a[i][1], a[i][2], b[i][1], b[i][2]) for i in range(n)])
    fp, fu, rp, ru = (_open_out(p) for p in outs)
    st = {"pairs": n, "both": 0, "fwd_only": 0, "rev_only": 0, "dropped": 0}
    for i in range(n):
        x, y = o1[i], o2[i]
        if x is not None and y is not None:
            _write(fp, a[i][0], a[i][1], a[i][2], x)
            _write(rp, b[i][0], b[i][1], b[i][2], y)
            st["both"] += 1
        elif x is not None:
            _write(fu, a[i][0], a[i][1], a[i][2], x)
            st["fwd_only"] += 1
        elif y is not None:
            _write(ru, b[i][0], b[i][1], b[i][2], y)
            st["rev_only"] += 1
        else:
            st["dropped"] += 1
    for f in (fp, fu, rp, ru):
        f.close()
    return st


def run_se(r1, out, steps):
    """Trimmomatic SE's one file and its counts."""
    a = read_fastq(r1)
    o1, _ = run_pairs(steps, [(x[1], x[2], b"", b"") for x in a], single_end=True)
    st = {"reads": len(a), "surviving": 0, "dropped": 0}
    with _open_out(out) as f:
        for x, rec in zip(a, o1):
            if rec is None:
                st["dropped"] += 1
            else:
                _write(f, x[0], x[1], x[2], rec)
                st["surviving"] += 1
    return st
