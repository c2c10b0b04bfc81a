#!/usr/bin/env python3
"""Throughput of the GPU adapter trimming (crispresso_amd/trim.py) on synthetic
CRISPResso-like pairs: a 250 bp amplicon, 2 x 150 bp reads, 1 % substitution noise per
read, qualities 53..73, PCG64 seed 7 (bench_flash.py's input), with 10 % of the pairs
replaced by short-fragment read-through pairs (a random 60-140 bp fragment, then the
Nextera adapters), so that the palindrome and the simple mode both do real work.
Options: CRISPResso's default ILLUMINACLIP:NexteraPE-PE.fa:0:90:10:0:true MINLEN:40.
Prints one JSON line: the kernel's time, pairs/s of the kernel (inputs resident) and of
the whole call (with PCIe), the clipped and dropped reads, the input bytes over the
kernel time as a fraction of 8 TB/s, and the CPU restatement
(oracle/trimmomatic_oracle.py, 1 thread) on a sample, for scale."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crispresso_amd.trim import TrimOptions, trim_packed  # noqa: E402

N = int(os.environ.get("TRIM_BENCH_PAIRS", "1000000"))
L, AMP = 150, 250
FASTA = os.path.join(ROOT, "tests", "golden", "NexteraPE-PE.fa")
STEPS = "ILLUMINACLIP:" + FASTA + ":0:90:10:0:true MINLEN:40"
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
# every 10th pair: a short fragment, both reads run through it into the adapters
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
opts = TrimOptions.from_steps(STEPS)
trim_packed(r1[:1000].ravel(), q1[:1000].ravel(), off[:1001], r2[:1000].ravel(), q2[:1000].ravel(), off[:1001], opts)
t0 = time.perf_counter()
res = trim_packed(r1.ravel(), q1.ravel(), off, r2.ravel(), q2.ravel(), off, opts)
wall = time.perf_counter() - t0
in_bytes = 4 * N * L + 2 * 8 * (N + 1)
out = {"metric": "trimmed read pairs/s", "pairs": N, "read_len": L, "kernel_ms": res.kernel_ms,
       "kernel_pairs_per_s": N / (res.kernel_ms / 1e3), "call_pairs_per_s": N / wall,
       "reads_clipped": int(((res.keep1 > 0) & (res.keep1 < L)).sum() + ((res.keep2 > 0) & (res.keep2 < L)).sum()),
       "reads_dropped": int((res.keep1 == 0).sum() + (res.keep2 == 0).sum()),
       "input_bytes": in_bytes, "fraction_of_8TBps": in_bytes / (res.kernel_ms / 1e3) / 8e12}
if os.environ.get("TRIM_BENCH_CPU", "1") == "1":
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import trimmomatic_oracle  # noqa: E402
    clip = trimmomatic_oracle.IlluminaClip(STEPS.split()[0][len("ILLUMINACLIP:"):])
    k = 300
    recs = [(("r", r1[i].tobytes().decode(), q1[i].tobytes().decode()),
             ("r", r2[i].tobytes().decode(), q2[i].tobytes().decode())) for i in range(k)]
    t0 = time.perf_counter()
    same = True
    for i, (a, b) in enumerate(recs):
        ca, cb = clip.process(a, b)
        la, lb = (0 if c is None or len(c[1]) < 40 else len(c[1]) for c in (ca, cb))
        same = same and la == res.keep1[i] and lb == res.keep2[i]
    out["cpu_restatement_pairs_per_s_1thread"] = k / (time.perf_counter() - t0)
    out["sample_equals_restatement"] = bool(same)
print(json.dumps(out))
