#!/usr/bin/env python3
"""The paired-end front end end to end (crispresso_amd/frontend.py: one upload, filter / clip /
steps / merge / pack on the device, the batch adopted in HBM) against the composed host path the
stages offer without it, on the same arrays in the same process, alternated:

    A  prepare_packed                                    + the resident pass
    B  trim_program_packed -> (cut the reads to their windows) -> merge_packed
       -> (gather the merged reads) -> pack_2bit -> upload_packed + the resident pass

Input: bench_trim.py's 1M synthetic 2 x 150 bp pairs (a 250 bp amplicon, 1 % substitution noise,
qualities 53..73, PCG64 seed 7, every 10th pair a 60-140 bp fragment read through into the Nextera
adapters), CRISPResso's default clip, MINLEN:40, FLASH 4 / 100 / outies.  Reads nothing outside
the repository.  Three warm-up passes of each path, then FRONT_BENCH_ROUNDS (9) alternated rounds; prints
one JSON line: medians and ranges of both, B's phases (the two numpy steps between the library
calls are listed apart: `b_calls_only` leaves them out), the front end's per-kernel device times,
the packer's bytes against the stream it writes, and whether both paths left the same batch and
the same alignments."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crispresso_amd import frontend  # noqa: E402
from crispresso_amd.aligner import GpuAligner, pack_2bit  # noqa: E402
from crispresso_amd.flash import FlashOptions, merge_packed  # noqa: E402
from crispresso_amd.trim import TrimProgram, trim_program_packed  # noqa: E402

N = int(os.environ.get("FRONT_BENCH_PAIRS", "1000000"))
ROUNDS = int(os.environ.get("FRONT_BENCH_ROUNDS", "9"))
L, AMP = 150, 250
FASTA = os.path.join(ROOT, "tests", "golden", "NexteraPE-PE.fa")
STEPS = "ILLUMINACLIP:" + FASTA + ":0:90:10:0:true MINLEN:40"
FLASH = FlashOptions(min_overlap=4, max_overlap=100, allow_outies=True)
A1 = np.frombuffer(b"CTGTCTCTTATACACATCTCCGAGCCCACGAGAC", np.uint8)   # what read 1 runs into
A2 = np.frombuffer(b"CTGTCTCTTATACACATCTGACGCTGCCGACGA", np.uint8)    # what read 2 runs into
rng = np.random.Generator(np.random.PCG64(7))
alpha = np.frombuffer(b"ACGT", np.uint8)
amp = rng.choice(alpha, AMP)
comp = np.zeros(256, np.uint8)
for a, b in zip(b"ACGT", b"TGCA"):
    comp[a] = b
r1 = np.tile(amp[:L], (N, 1))
r2 = np.tile(comp[amp[::-1]][:L], (N, 1))
for r in (r1, r2):
    m = rng.random(r.shape) < 0.01
    r[m] = rng.choice(alpha, int(m.sum()))
q1 = rng.integers(53, 74, (N, L)).astype(np.uint8)
q2 = rng.integers(53, 74, (N, L)).astype(np.uint8)
rows = np.arange(0, N, 10)
K = len(rows)
flen = rng.integers(60, 141, K)[:, None]
frag = rng.choice(alpha, (K, L))
pos = np.arange(L)[None, :]
rc_frag = comp[np.take_along_axis(frag, np.clip(flen - 1 - pos, 0, L - 1), axis=1)]
for dst, adapter, body in ((r1, A1, frag), (r2, A2, rc_frag)):
    tail = rng.choice(alpha, (K, L))
    in_adapter = (pos >= flen) & (pos < flen + len(adapter))
    tail = np.where(in_adapter, adapter[np.clip(pos - flen, 0, len(adapter) - 1)], tail)
    dst[rows] = np.where(pos < flen, body, tail)
off = np.arange(N + 1, dtype=np.int64) * L
s1, s2, q1, q2 = r1.ravel(), r2.ravel(), q1.ravel(), q2.ravel()
prog = TrimProgram.from_steps(STEPS)
amplicon = amp.tobytes().decode()
clock = time.perf_counter


def resident_pass(al, m):
    t = clock()
    al.run_async()
    dev_ms = al.sync()
    return clock() - t, dev_ms


def path_front(al, s1, q1, off1, s2, q2, off2):
    t0 = clock()
    pb = frontend.prepare_packed(al, s1, q1, off1, s2, q2, off2, trim=prog, flash=FLASH)
    t1 = clock()
    wall, dev_ms = resident_pass(al, len(pb))
    ph = {"prepare": t1 - t0, "pass": wall, "pass_device_ms": dev_ms}
    ph.update({k: v for k, v in pb.stats.items() if k.endswith("_ms")})
    return clock() - t0, ph, pb.buf, pb.offsets


def cut(seq, qual, off, start, keep, live):
    """The reads' windows, packed (the host step between the trim and the merge calls)."""
    lens = np.where(live, keep, 0).astype(np.int64)
    o = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=o[1:])
    idx = np.repeat(off[:-1] + start - o[:-1], lens) + np.arange(o[-1])
    return seq[idx], qual[idx], o


def path_composed(al, s1, q1, off1, s2, q2, off2):
    ph = {}
    t0 = t = clock()
    w = trim_program_packed(s1, q1, off1, s2, q2, off2, prog)
    ph["trim_program_packed"], t = clock() - t, clock()
    live = (w.keep1 >= 0) & (w.keep2 >= 0)   # Trimmomatic's fp / rp files
    c1, cq1, co1 = cut(s1, q1, off1, w.start1, w.keep1, live)
    c2, cq2, co2 = cut(s2, q2, off2, w.start2, w.keep2, live)
    ph["numpy_cut"], t = clock() - t, clock()
    mr = merge_packed(c1, cq1, co1, c2, cq2, co2, FLASH)
    ph["merge_packed"], t = clock() - t, clock()
    lens = mr.length.astype(np.int64)
    o = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=o[1:])
    buf = mr.seq[np.repeat(mr.base - o[:-1], lens) + np.arange(o[-1])]
    sel = np.flatnonzero(lens > 0)
    offsets = np.concatenate([o[sel], o[-1:]])
    ph["numpy_gather"], t = clock() - t, clock()
    pr = pack_2bit(buf, offsets)
    ph["pack_2bit"], t = clock() - t, clock()
    al.upload_packed(pr)
    ph["upload_packed"], t = clock() - t, clock()
    ph["pass"], ph["pass_device_ms"] = resident_pass(al, len(offsets) - 1)
    ph["clip_ms"], ph["steps_ms"], ph["merge_ms"] = w.kernel_ms_clip, w.kernel_ms_steps, mr.kernel_ms
    return clock() - t0, ph, buf, offsets


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    args = (s1, q1, off, s2, q2, off)
    small = (s1[:L * 2000], q1[:L * 2000], off[:2001], s2[:L * 2000], q2[:L * 2000], off[:2001])
    with GpuAligner(0) as a_front, GpuAligner(0) as a_comp:
        for al in (a_front, a_comp):
            al.set_reference(amplicon)
            al.set_phase_events(False)
        path_front(a_front, *small), path_composed(a_comp, *small)
        # warm-up at the timed size, three passes of each path (the pinned output pool hands out a
        # second block of the batch's size while the aligner still holds the previous batch's text);
        # then the two paths' results against each other
        for _ in range(2):
            path_front(a_front, *args), path_composed(a_comp, *args)
        _, _, fbuf, foff = path_front(a_front, *args)
        mf = len(foff) - 1
        of = a_front.download_ops(mf)
        _, _, cbuf, coff = path_composed(a_comp, *args)
        oc = a_comp.download_ops(len(coff) - 1)
        same_batch = bool(np.array_equal(fbuf, cbuf) and np.array_equal(foff, coff))
        same_ops = bool(np.array_equal(of.stats, oc.stats) and np.array_equal(of.ops, oc.ops)
                        and np.array_equal(of.ops_off, oc.ops_off))
        total = int(foff[-1])
        del fbuf, cbuf, of, oc
        tf, tc, pf, pc = [], [], [], []
        for _ in range(ROUNDS):
            t, ph, _, _ = path_front(a_front, *args)
            tf.append(t), pf.append(ph)
            t, ph, _, _ = path_composed(a_comp, *args)
            tc.append(t), pc.append(ph)
    calls = ("trim_program_packed", "merge_packed", "pack_2bit", "upload_packed", "pass")
    b_calls = [sum(p[k] for k in calls) for p in pc]
    med = lambda ps: {k: sorted(p[k] for p in ps)[len(ps) // 2] for k in ps[0]}   # noqa: E731
    # the packer: count reads the merged bytes once, scatter reads them and writes them dense,
    # words reads the dense bytes and writes the stream; per-pair metadata beside
    pack_read = 3 * total + N * (8 + 8 + 4 + 4 + 4 + 4 + 4)
    pack_write = total + (total + 3) // 4 + N * (1 + 4) + mf * (8 + 2 + 8)
    out = {
        "metric": "raw pairs to aligned resident batch, s", "pairs": N, "read_len": L, "rounds": ROUNDS,
        "merged_reads": mf, "merged_bases": total,
        "front_s": spread(tf), "composed_s": spread(tc), "composed_calls_only_s": spread(b_calls),
        "speedup_median": spread(tc)["median"] / spread(tf)["median"],
        "speedup_vs_calls_only_median": spread(b_calls)["median"] / spread(tf)["median"],
        "ranges_overlap": bool(max(tf) >= min(b_calls)),
        "front_rounds_s": tf, "composed_rounds_s": tc, "composed_calls_only_rounds_s": b_calls,
        "front_phases_median": med(pf), "composed_phases_median": med(pc),
        "packer_bytes_read": pack_read, "packer_bytes_written": pack_write, "stream_bytes": (total + 3) // 4,
        "same_batch": same_batch, "same_alignments": same_ops,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
