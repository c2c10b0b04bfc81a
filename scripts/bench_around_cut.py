#!/usr/bin/env python3
"""The allele table around a cut site from the resident batch against the path it replaces.

Input: the C2 workload of scripts/bench_alleles.py (synth.c2_workload: a 250 bp amplicon, 1M
reads), aligned and quantified resident.  For one cut point and for two, in one process on that
one batch:

* alleles.around_cut_tables (nwa_windows_device: window extract, grouping, unedited + gather by
  HIP events; the call; the strings and the frame);
* the path it replaces: alleles.group_reads + alleles.allele_table (the full-length table) followed
  by alleles.around_cut_from_alleles per cut point;
* that both give equal tables, the number of window groups beside the distinct reads, and the
  ratio of the two paths.

The measuring process is a child started under a time limit of its own; one JSON document goes to
``--out`` (default profiles/r01_around_cut/bench_around_cut.json) and to stdout."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(n_reads: int, steps: int, offset: int) -> dict:
    import numpy as np
    import pandas as pd

    from crispresso_amd import alleles, quantify, synth
    from crispresso_amd.aligner import GpuAligner
    from crispresso_amd.devmem import DeviceBuffer
    from crispresso_amd.needle import _printed_percents

    amp, buf, off = synth.c2_workload(n_reads)
    n = len(off) - 1
    args = argparse.Namespace(amplicon_seq=amp, guide_seq=amp[105:125], cleavage_offset=-3, window_around_sgrna=1,
                              exclude_bp_from_left=15, exclude_bp_from_right=15, coding_seq=None,
                              expected_hdr_amplicon_seq=None)
    cut = int(quantify.compute_cut_points(amp, args.guide_seq)[0])
    clock = time.perf_counter
    out = {}
    with GpuAligner(0) as al, quantify.GpuQuantifier(0) as q:
        al.set_reference(amp)
        al.set_output("ops")
        al.upload(buf, off)
        al.run_async()
        al.sync()
        dev = al.device_ops()
        ob = al.download_ops(n)
        score = _printed_percents(ob.stats["n_ident"], np.maximum(ob.stats["aln_len"], 1))
        keep = ((ob.stats["flags"] & 1) == 0) & (score > 60.0)
        q.set_params(quantify.globals_from_args(args), args)
        with DeviceBuffer.from_array(quantify.pre_flags(score == 100)) as d_pre, DeviceBuffer(16 * n) as d_out:
            q.run_device_ops(amp, dev, d_pre.ptr, n, d_out.ptr)
            rr = d_out.download(np.zeros((n, 4), np.int32))
        grouper = alleles.default_grouper(0)
        out["workload"] = f"C2: {n} reads of a 250 bp amplicon, {int(keep.sum())} kept (identity > 60), offset {offset}"
        for cuts in ([cut], [cut, cut + 60]):
            alleles.around_cut_tables(al, amp, buf, off, rr, cuts, offset, keep=keep)        # warm-up: buffers allocated
            new_s, phases, call_s = [], [], []
            for _ in range(steps):
                t0 = clock()
                got = alleles.around_cut_tables(al, amp, buf, off, rr, cuts, offset, keep=keep)
                new_s.append(clock() - t0)
                phases.append(grouper.window_times())
                t0 = clock()
                wins = grouper.windows(dev, n, ob.awidth, amp, cuts, offset, rr, keep=keep)
                call_s.append(clock() - t0)
            old = {"group_reads_s": [], "allele_table_s": [], "around_cut_from_alleles_s": []}
            for _ in range(steps):
                t0 = clock()
                groups = alleles.group_reads(al, buf, off, keep=keep)
                old["group_reads_s"].append(clock() - t0)
                t0 = clock()
                table = alleles.allele_table(amp, buf, off, ob, rr, groups)
                old["allele_table_s"].append(clock() - t0)
                t0 = clock()
                want = [alleles.around_cut_from_alleles(table, c, offset) for c in cuts]
                old["around_cut_from_alleles_s"].append(clock() - t0)
            for g, w in zip(got, want):
                pd.testing.assert_frame_equal(g, w)
            best = min
            old_s = sum(best(v) for v in old.values())
            out[f"cut_points_{len(cuts)}"] = {
                "cut_points": cuts, "distinct_reads": len(groups), "alleles": len(table),
                "window_groups": [len(w) for w in wins], "table_rows": [len(g) for g in got],
                "collided": wins[0].collided,
                "kernel_ms": {k: best(p[k] for p in phases) for k in phases[0]},
                "nwa_windows_device_call_s": best(call_s),
                "around_cut_tables_s": best(new_s),
                "replaced_path_s": {k: best(v) for k, v in old.items()},
                "replaced_path_total_s": old_s,
                "replaced_over_new": old_s / best(new_s),
                "tables_equal": True,
            }
    out["steps"], out["statistic"] = steps, "minimum over the steps"
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--offset", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=480, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r01_around_cut", "bench_around_cut.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.reads, a.steps, a.offset)))
        return 0
    # the GPU step: a process of its own under its own time limit
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reads", str(a.reads), "--steps",
                        str(a.steps), "--offset", str(a.offset)], capture_output=True, text=True, timeout=a.timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        return p.returncode or 1
    line = p.stdout.strip().splitlines()[-1]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(json.loads(line), indent=1) + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
