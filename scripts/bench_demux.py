#!/usr/bin/env python3
"""Pooled-amplicon demultiplexing on the GPU against a Python loop restating its rule.

Input (seeded): ``--reads`` reads (default 1M) of about 250 bp over ``synth.pooled_amplicons(96)``
(the C2 edit mix), every odd read reverse-complemented, the amplicons' reads interleaved.
Reports, in one process, as the median of ``--rounds`` alternated rounds after a warm-up round:

* the ``demultiplex`` call from host arrays (index build, assignment, gather, the copies);
* its assign kernel (HIP events, summed over the chunks), the index build, the gather kernel and
  the host's wall time in the chunks' uploads (nwd_phase_times);
* the restatement's loop (tests/demux_model.demultiplex: a dict of windows and a ``Counter``) on
  the first ``--loop-reads`` reads, its time per read, and that time scaled to all reads (the
  loop over all of them would take minutes per round; the scaled figure is marked as such).

The GPU result is compared with the model on the loop's reads, and with the reads' sources on all
of them, before anything is reported.  The measuring process is a child under a time limit of its
own; one JSON document goes to ``--out`` (default profiles/r01_demux/bench_demux.json) and to
stdout.  No ratio is required: the numbers are written as measured."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(n_reads: int):
    import numpy as np

    from crispresso_amd import synth
    from tests import demux_model as dm

    amps = synth.pooled_amplicons(96)
    per = -(-n_reads // len(amps))
    parts = [synth.reads_from(a, per, seed=700 + g) for g, a in enumerate(amps)]
    # interleave: read i comes from amplicon i % 96; odd reads reverse-complemented
    reads = []
    for g, (buf, off) in enumerate(parts):
        raw = buf.tobytes()
        reads.append([raw[off[i]:off[i + 1]] for i in range(per)])
    flat = [reads[i % len(amps)][i // len(amps)] for i in range(n_reads)]
    flat = [dm.revcomp(r) if i % 2 else r for i, r in enumerate(flat)]
    text = np.frombuffer(b"".join(flat), np.uint8)
    offsets = np.zeros(n_reads + 1, np.int64)
    np.cumsum(np.fromiter((len(r) for r in flat), np.int64, n_reads), out=offsets[1:])
    return amps, flat, text, offsets


def measure(n_reads: int, rounds: int, loop_reads: int) -> dict:
    import numpy as np

    from crispresso_amd import demux
    from tests import demux_cases as dc
    from tests import demux_model as dm

    amps, flat, text, offsets = workload(n_reads)
    amps_b = [a.encode() for a in amps]
    loop_reads = min(loop_reads, n_reads)
    clock = time.perf_counter
    out = {"workload": f"{n_reads} reads of {len(text) / n_reads:.1f} bp on average over {len(amps)} amplicons "
                       f"({sum(len(a) for a in amps)} bases), odd reads reverse-complemented",
           "k": 16, "min_hits": 2, "both_strands": True, "rounds": rounds,
           "statistic": "median of the alternated rounds after one warm-up round", "text_bytes": int(len(text)),
           "loop_reads": loop_reads}
    call_s, kernel_ms, upload_ms, index_ms, gather_ms, loop_s = [], [], [], [], [], []
    with demux.GpuDemultiplexer(0) as d:
        for rnd in range(rounds + 1):
            t0 = clock()
            res = demux.demultiplex(amps, (text, offsets), demultiplexer=d)       # (synchronous: ends in a device sync)
            t_call = clock() - t0
            ph = d.phase_times()
            t0 = clock()
            want = dm.demultiplex(amps_b, flat[:loop_reads])
            t_loop = clock() - t0
            if rnd == 0:        # the warm-up round, checked
                if res.which[:loop_reads].tolist() != want["which"] or res.strand[:loop_reads].tolist() != want["strand"] \
                        or res.votes[:loop_reads].tolist() != want["votes"] or res.rival[:loop_reads].tolist() != want["rival"]:
                    raise SystemExit("the GPU result differs from the model")
                head = demux.demultiplex(amps, (text, offsets[:loop_reads + 1]), demultiplexer=d)
                bad = dc.mismatches(head, want)
                if bad:
                    raise SystemExit("the GPU result differs from the model:\n" + "\n".join(bad))
                source = np.arange(n_reads) % len(amps)
                out["assigned_to_source"] = int((res.which == source).sum())
                out["n_assigned"], out["n_tie"], out["n_no_hit"] = res.n_assigned, res.n_tie, res.n_no_hit
                out["fallback"] = res.fallback
                out["n_windows"], out["n_ambiguous"] = res.n_windows, res.n_ambiguous
                out["equal_to_model_on_loop_reads"] = True
                continue
            call_s.append(t_call)
            kernel_ms.append(ph["assign"])
            upload_ms.append(ph["upload_wall"])
            index_ms.append(ph["index"])
            gather_ms.append(ph["gather"])
            loop_s.append(t_loop)
    med = statistics.median
    call, loop = med(call_s), med(loop_s)
    out.update({
        "demultiplex_call_s": call, "demultiplex_call_s_all_rounds": call_s, "reads_per_s": n_reads / call,
        "assign_kernel_ms": med(kernel_ms), "upload_wall_ms": med(upload_ms), "index_build_ms": med(index_ms),
        "gather_kernel_ms": med(gather_ms),
        "python_loop_s_on_loop_reads": loop, "python_loop_us_per_read": loop / loop_reads * 1e6,
        "python_loop_s_scaled_to_all_reads": loop / loop_reads * n_reads,
        "scaled_loop_over_call": loop / loop_reads * n_reads / call,
    })
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=int(os.environ.get("DEMUX_BENCH_READS", "1000000")))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-reads", type=int, default=20000, help="reads the Python loop is timed on")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r01_demux", "bench_demux.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.reads, a.rounds, a.loop_reads)))
        return 0
    # the GPU step: a process of its own under its own time limit
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reads", str(a.reads), "--rounds",
                        str(a.rounds), "--loop-reads", str(a.loop_reads)], capture_output=True, text=True,
                       timeout=a.timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:] + p.stdout[-2000:])
        return p.returncode or 1
    line = p.stdout.strip().splitlines()[-1]
    doc = json.loads(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
