#!/usr/bin/env python3
"""sgRNA counting on the GPU against the per-read Python loop it replaces.

Input (seeded, tests/count_cases.mixed_batch): 1M reads of 50 bp -- a 20-base guide of a
1,000-guide library (Zipf-like weights), the default 20-base tracrRNA, flanks; 5 % of the reads
with one substitution in the guide, 2 % without the tracrRNA.  Reports, in one process, as the
minimum of ``--steps`` after a warm-up:

* the ``count_guides`` call from host arrays, without and with a whitelist (the library);
* its kernels by phase (HIP events, nwc_phase_times), and the bytes each phase has to move
  (computed from the shapes below) over its time, beside the HBM rate;
* the share of the call spent in the chunks' uploads and in the kernels;
* the restatement's loop (tests/count_model.fast_model: ``bytes.find``, a slice, a dict) over the
  same reads -- what a user of the reference runs today -- and the ratio of the two.

The results of both paths are compared before anything is reported.  The measuring process is a
child under a time limit of its own; one JSON document goes to ``--out`` (default
profiles/r01_count/bench_count.json) and to stdout.  The exit status is 1 when the call is not
faster than the loop (the ratio is written either way)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0      # MI355X: 8 TB/s


def phase_bytes(n, text_bytes, found, kw, whitelist):
    """The bytes each phase's algorithm reads and writes (no cache effects, the table's atomics
    counted as one 16-byte touch per found read at most: a lower bound on the traffic)."""
    key = 4 * kw
    out = {"find": text_bytes + 8 * (n + 1) + 16 * n + key * found}
    if whitelist:
        out["verify_or_lookup"] = 8 * n + 4 * n + found * (16 + 2 * key)
    else:
        out["insert"] = 8 * n + 4 * n + 16 * found
        out["publish"] = 4 * n + 4 * found
        out["verify_or_lookup"] = 4 * n + found * (12 + 2 * key)
    return out


def measure(n_reads: int, steps: int) -> dict:
    import numpy as np

    from crispresso_amd import count
    from tests import count_cases as cc
    from tests import count_model as cm

    reads, T, L, info = cc.mixed_batch(n_reads, 1000, 21)
    n = len(reads)
    text = np.frombuffer(b"".join(reads), np.uint8)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(np.fromiter((len(r) for r in reads), np.int64, n), out=offsets[1:])
    library = info["library"]
    clock = time.perf_counter
    out = {"workload": f"{n} reads of {len(reads[0])} bp, 1,000-guide library (Zipf), {info['sub']} reads with one "
                       f"substitution in the guide, {info['miss']} without the tracrRNA",
           "tracrRNA": T.decode(), "guide_length": L, "steps": steps, "statistic": "minimum over the steps",
           "hbm_peak_GBps": HBM_PEAK_GBS, "text_bytes": int(len(text))}
    with count.GpuGuideCounter(0) as c:
        for mode, guides in (("no_whitelist", None), ("whitelist", library)):
            want = cm.fast_model(reads, T, L, guides)
            got = count.count_guides(text, offsets, T.decode(), L, guides, c, want_pos=True, want_group_of_read=True)
            bad = cc.mismatches(got, want)                          # (the warm-up call, checked)
            if bad:
                raise SystemExit("the GPU result differs from the model:\n" + "\n".join(bad))
            call_s, kernel_ms, phases, loop_s, full_s = [], [], [], [], []
            for _ in range(steps):
                t0 = clock()
                res = count.count_guides(text, offsets, T.decode(), L, guides, c)
                call_s.append(clock() - t0)
                kernel_ms.append(res.kernel_ms)
                phases.append(c.phase_times())
                t0 = clock()
                count.count_guides(text, offsets, T.decode(), L, guides, c, want_pos=True, want_group_of_read=True)
                full_s.append(clock() - t0)
                t0 = clock()
                cm.fast_model(reads, T, L, guides)
                loop_s.append(clock() - t0)
            best = min
            ph = {k: best(p[k] for p in phases) for k in phases[0]}
            nbytes = phase_bytes(n, len(text), want["n_found"], (L + 3) // 4, guides is not None)
            call, loop = best(call_s), best(loop_s)
            out[mode] = {
                "groups": len(res), "n_found": res.n_found, "n_counted": res.n_counted, "collided": res.collided,
                "equal_to_model": True,
                "call_s": call, "call_with_per_read_arrays_s": best(full_s), "reads_per_s": n / call,
                "kernels_total_ms": best(kernel_ms), "phase_ms": ph,
                "phase_bytes": nbytes,
                "phase_GBps": {k: (v / (ph[k] * 1e-3) / 1e9 if ph[k] > 0 else None) for k, v in nbytes.items()},
                "upload_share_of_call": ph["upload_wall"] * 1e-3 / call,
                "kernel_share_of_call": best(kernel_ms) * 1e-3 / call,
                "kernels_over_upload": best(kernel_ms) / ph["upload_wall"] if ph["upload_wall"] > 0 else None,
                "python_loop_s": loop, "loop_over_call": loop / call, "call_faster_than_loop": call < loop,
            }
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=int(os.environ.get("COUNT_BENCH_READS", "1000000")))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=480, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r01_count", "bench_count.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.reads, a.steps)))
        return 0
    # the GPU step: a process of its own under its own time limit
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reads", str(a.reads), "--steps",
                        str(a.steps)], capture_output=True, text=True, timeout=a.timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:] + p.stdout[-2000:])
        return p.returncode or 1
    line = p.stdout.strip().splitlines()[-1]
    doc = json.loads(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(line)
    return 0 if all(doc[m]["call_faster_than_loop"] for m in ("no_whitelist", "whitelist")) else 1


if __name__ == "__main__":
    sys.exit(main())
