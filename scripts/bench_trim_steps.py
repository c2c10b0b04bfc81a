#!/usr/bin/env python3
"""The steps kernel (crispresso_amd/csrc/trim_steps.hip) beside the clip kernel on one batch:
bench_trim.py's pairs (a 250 bp amplicon, 2 x 150 bp reads, 1 % substitution noise, every 10th
pair a short fragment read through into the Nextera adapters, PCG64 seed 7) with qualities that
make the steps act (PCG64 seed 11): phred 20..40 uniform; in 30 % of the reads phred 2..12 from
a random position in the last third to the end; 1 % of the reads with one N.
Program: ILLUMINACLIP:NexteraPE-PE.fa:0:90:10:0:true LEADING:3 TRAILING:3 SLIDINGWINDOW:4:15
MINLEN:36 through trim_program_packed; beside it CRISPResso's default string
(ILLUMINACLIP:... MINLEN:40) through trim_packed on the same batch, the two calls alternating
in one process, the minimum of 3 each.
Prints one JSON line: both kernels' times, the steps kernel's input bytes over its time as a
fraction of 8 TB/s, the reads each step changed or dropped (among those alive when it runs;
from the device, by running the program's prefixes), the two call times, and whether the first
300 pairs equal the restatement tests/trim_steps_model.py."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crispresso_amd.trim import TrimOptions, TrimProgram, trim_packed, trim_program_packed  # noqa: E402

N = int(os.environ.get("TRIM_BENCH_PAIRS", "1000000"))
L, AMP = 150, 250
FASTA = os.path.join(ROOT, "tests", "golden", "NexteraPE-PE.fa")
CLIP = "ILLUMINACLIP:" + FASTA + ":0:90:10:0:true"
DEFAULT = CLIP + " MINLEN:40"
STEPS = ["LEADING:3", "TRAILING:3", "SLIDINGWINDOW:4:15", "MINLEN:36"]
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
rng.integers(53, 74, (N, L))   # bench_trim.py's qualities: drawn to keep its stream, replaced below
rng.integers(53, 74, (N, L))
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

qrng = np.random.Generator(np.random.PCG64(11))


def qualities(reads):
    q = qrng.integers(20, 41, (N, L)).astype(np.uint8)
    bad = qrng.random(N) < 0.3
    start = qrng.integers(2 * L // 3, L, N)
    low = qrng.integers(2, 13, (N, L)).astype(np.uint8)
    q = np.where(bad[:, None] & (pos >= start[:, None]), low, q)
    with_n = np.flatnonzero(qrng.random(N) < 0.01)
    reads[with_n, qrng.integers(0, L, len(with_n))] = ord("N")
    return (q + 33).astype(np.uint8)


q1 = qualities(r1)
q2 = qualities(r2)
off = np.arange(N + 1, dtype=np.int64) * L
batch = (r1.ravel(), q1.ravel(), off, r2.ravel(), q2.ravel(), off)
small = (r1[:1000].ravel(), q1[:1000].ravel(), off[:1001], r2[:1000].ravel(), q2[:1000].ravel(), off[:1001])
prog = TrimProgram.from_steps([CLIP] + STEPS)
opts = TrimOptions.from_steps(DEFAULT)
trim_program_packed(*small, prog)
trim_packed(*small, opts)
t_prog, t_def, res, base = [], [], None, None
for _ in range(3):
    t0 = time.perf_counter()
    res = trim_program_packed(*batch, prog)
    t_prog.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    base = trim_packed(*batch, opts)
    t_def.append(time.perf_counter() - t0)

# per step: the program's prefixes on the device; a record that a step changes or drops differs
# between two successive prefixes
per_step = {}
prev = trim_program_packed(*batch, TrimProgram(prog.clip, []))
entering = int((prev.keep1 >= 0).sum() + (prev.keep2 >= 0).sum())
for k, name in enumerate(STEPS):
    cur = trim_program_packed(*batch, TrimProgram(prog.clip, prog.steps[:k + 1]))
    changed = dropped = 0
    for ps, pk, cs, ck in ((prev.start1, prev.keep1, cur.start1, cur.keep1),
                           (prev.start2, prev.keep2, cur.start2, cur.keep2)):
        alive = pk >= 0
        dropped += int((alive & (ck < 0)).sum())
        changed += int((alive & (ck >= 0) & ((cs != ps) | (ck != pk))).sum())
    per_step[name] = {"changed": changed, "dropped": dropped}
    prev = cur
assert np.array_equal(prev.keep1, res.keep1) and np.array_equal(prev.start2, res.start2)

steps_bytes = 4 * N * L + 2 * 8 * (N + 1) + 2 * 4 * N   # bases, qualities, offsets, the clip's lengths
out = {"metric": "trimmed read pairs/s", "pairs": N, "read_len": L, "program": "ILLUMINACLIP(default) " + " ".join(STEPS),
       "kernel_ms_clip": res.kernel_ms_clip, "kernel_ms_steps": res.kernel_ms_steps,
       "kernel_ms_clip_default_string": base.kernel_ms,
       "steps_input_bytes": steps_bytes,
       "steps_fraction_of_8TBps": steps_bytes / (res.kernel_ms_steps / 1e3) / 8e12,
       "reads_entering_the_steps": entering, "per_step": per_step,
       "reads_surviving": int((res.keep1 >= 0).sum() + (res.keep2 >= 0).sum()),
       "call_s_program": min(t_prog), "call_s_default_string": min(t_def),
       "call_s_program_all": t_prog, "call_s_default_string_all": t_def,
       "extra_output_bytes": 2 * 2 * 4 * N}
if os.environ.get("TRIM_BENCH_CPU", "1") == "1":
    sys.path.insert(0, ROOT)
    from tests import trim_steps_model  # noqa: E402
    k = 300
    pairs = [(r1[i].tobytes(), q1[i].tobytes(), r2[i].tobytes(), q2[i].tobytes()) for i in range(k)]
    e1, e2 = trim_steps_model.run_pairs([CLIP] + STEPS, pairs)
    s1, k1 = trim_steps_model.windows(e1)
    s2, k2 = trim_steps_model.windows(e2)
    out["sample_equals_model"] = bool(np.array_equal(s1, res.start1[:k]) and np.array_equal(k1, res.keep1[:k])
                                      and np.array_equal(s2, res.start2[:k]) and np.array_equal(k2, res.keep2[:k]))
print(json.dumps(out))
