#!/usr/bin/env python3
"""The pooled amplicon flow with the reads kept in HBM against the flow through the host.

Input (seeded): scripts/bench_demux.py's panel -- ``--reads`` reads (default 1M) of about 220 bp
over ``synth.pooled_amplicons(96)``, every odd read reverse-complemented, interleaved.
In one process, after a warm-up round in which the two results are compared, ``--rounds``
alternated rounds of

* ``demux.align_demultiplexed`` with the ops output (gather to the host, concatenate, pack and
  upload again, ``nw_align_multi_ops``, rows rebuilt on the host), and the same up to the runs
  (``demultiplex`` + ``align_multi_ops``, no rows), which is what the resident call returns;
* ``demux.align_demultiplexed_resident`` (assign, group and 2-bit pack in HBM, every group
  adopted where it lies, one synchronised pass per amplicon, runs back);
* the resident call's steps one by one, from the same public methods: index + assign, the packer
  (wall and, by HIP events, its kernels), and the per-group loop (wall, and split into
  set_reference / adoption / pass / download; the pass also in device ms).

Each figure is the median of the rounds with its range.  Host clocks surround work that ends in
a device synchronise.  No ratio is required: the numbers are written as measured, to ``--out``
(default profiles/r01_demux_resident/bench_demux_resident.json) and to stdout."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": list(xs)}


def measure(n_reads: int, rounds: int) -> dict:
    import numpy as np

    from bench_demux import workload
    from crispresso_amd import demux
    from crispresso_amd.aligner import GpuAligner

    amps, _, text, offsets = workload(n_reads)
    reads = (text, offsets)
    clock = time.perf_counter
    out = {"workload": f"{n_reads} reads of {len(text) / n_reads:.1f} bp on average over {len(amps)} amplicons, "
                       "odd reads reverse-complemented", "k": 16, "min_hits": 2, "rounds": rounds,
           "statistic": "median (min, max) of the alternated rounds after one warm-up round; seconds unless named ms",
           "text_bytes": int(len(text))}
    T = {k: [] for k in ("host_align_demultiplexed", "host_to_runs", "host_demultiplex", "host_align_multi_ops",
                         "resident_call", "steps_total", "steps_index_assign", "steps_pack", "steps_loop",
                         "loop_set_reference", "loop_adopt", "loop_pass", "loop_download", "pack_kernels_ms",
                         "loop_pass_device_ms")}

    def host_to_runs(d, al):
        t0 = clock()
        res = demux.demultiplex(amps, reads, demultiplexer=d)
        t1 = clock()
        which = np.repeat(np.arange(len(amps), dtype=np.int32), res.counts)
        ob = al.align_multi_ops(amps, res.text, res.text_offsets, which)
        return res, ob, t1 - t0, clock() - t1

    def steps(d, al):
        """align_demultiplexed_resident's own steps, timed one by one."""
        t = {}
        t0 = clock()
        abuf, aoff = demux.pack_amplicons(amps)
        d.set_amplicons(abuf, aoff, 16)
        got = d.assign(text, offsets, 2, True)
        t["steps_index_assign"] = clock() - t0
        t1 = clock()
        pk = d.pack(got[5])
        t["steps_pack"] = clock() - t1
        t["pack_kernels_ms"] = pk.kernel_ms
        acc = dict.fromkeys(("loop_set_reference", "loop_adopt", "loop_pass", "loop_download", "loop_pass_device_ms"), 0.0)
        al.set_output("ops")
        t2 = clock()
        for g in range(len(amps)):
            if int(got[4][g]) == 0:
                continue
            a = clock()
            al.set_reference(amps[g])
            b = clock()
            n = d.adopt(al, g)
            c = clock()
            al.run_async()
            acc["loop_pass_device_ms"] += al.sync()
            e = clock()
            al.download_ops(n)
            f = clock()
            acc["loop_set_reference"] += b - a
            acc["loop_adopt"] += c - b
            acc["loop_pass"] += e - c
            acc["loop_download"] += f - e
        t["steps_loop"] = clock() - t2
        t["steps_total"] = clock() - t0
        al.set_output("rows")
        t.update(acc)
        return t

    with demux.GpuDemultiplexer(0) as d, GpuAligner(0) as al:
        for rnd in range(rounds + 1):
            t0 = clock()
            demux.align_demultiplexed(amps, reads, al, demultiplexer=d)
            t_host = clock() - t0
            res, ob, t_dm, t_ops = host_to_runs(d, al)
            t0 = clock()
            obs, rres, skipped = demux.align_demultiplexed_resident(amps, reads, al, demultiplexer=d)
            t_res = clock() - t0
            st = steps(d, al)
            if rnd == 0:        # the warm-up round, checked: the resident runs are the host path's
                if skipped or not np.array_equal(rres.which, res.which) or not np.array_equal(rres.order, res.order):
                    raise SystemExit("the resident call's decisions differ from the host path's")
                for g in range(len(amps)):
                    lo, hi = int(res.group_offsets[g]), int(res.group_offsets[g + 1])
                    o0, o1 = int(ob.ops_off[lo]), int(ob.ops_off[hi])
                    if not (np.array_equal(obs[g].stats, ob.stats[lo:hi]) and np.array_equal(obs[g].ops, ob.ops[o0:o1])):
                        raise SystemExit(f"the resident call's runs differ from the host path's in group {g}")
                out["equal_to_host_path"] = True
                out["n_assigned"] = int(res.n_assigned)
                out["groups"] = int((res.counts > 0).sum())
                out["gathered_bytes"] = int(res.text_offsets[-1])
                out["n_exceptions"] = int(d._packed.n_exc) if d._packed is not None else None
                continue
            T["host_align_demultiplexed"].append(t_host)
            T["host_demultiplex"].append(t_dm)
            T["host_align_multi_ops"].append(t_ops)
            T["host_to_runs"].append(t_dm + t_ops)
            T["resident_call"].append(t_res)
            for k, v in st.items():
                T[k].append(v)
    out.update({k: summary(v) for k, v in T.items()})
    out["resident_over_host_to_runs"] = out["resident_call"]["median"] / out["host_to_runs"]["median"]
    out["resident_over_host_align_demultiplexed"] = out["resident_call"]["median"] / out["host_align_demultiplexed"]["median"]
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=int(os.environ.get("DEMUX_BENCH_READS", "1000000")))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r01_demux_resident", "bench_demux_resident.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.reads, a.rounds)))
        return 0
    # the GPU step: a process of its own under its own time limit
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reads", str(a.reads), "--rounds",
                        str(a.rounds)], capture_output=True, text=True, timeout=a.timeout)
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
