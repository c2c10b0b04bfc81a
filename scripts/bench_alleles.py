#!/usr/bin/env python3
"""The allele table from the resident batch against the per-read DataFrame path it replaces.

Input: the C2 workload (synth.c2_workload: a 250 bp amplicon, 1M reads), aligned and quantified
resident (upload -> run -> nw_batch_device_ops -> nwq_run_device_ops).  Reports, in one process on
that one batch:

* the grouping kernels by HIP events (hash / insert / verify / compaction) and the call's wall time
  (crispresso_amd.alleles.GpuAlleleGrouper.group: nwa_group_device);
* alleles.allele_table's wall time (strings of one read per group + the reference's last steps);
* the existing path: needle.ops_to_dataframe for every read, the class / count columns as
  quantify._result_tuple fills them, and quantify.run_summary's groupby (CORE:2923-2946);
* that both tables are equal, and the ratio of the two paths.

The measuring process is a child started under a time limit of its own; one JSON document goes to
``--out`` (default profiles/r01_alleles/bench_alleles.json) and to stdout."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(n_reads: int, steps: int) -> dict:
    import numpy as np
    import pandas as pd

    from crispresso_amd import alleles, quantify, synth
    from crispresso_amd.aligner import GpuAligner
    from crispresso_amd.devmem import DeviceBuffer
    from crispresso_amd.needle import _printed_percents, ops_to_dataframe

    amp, buf, off = synth.c2_workload(n_reads)
    n = len(off) - 1
    args = argparse.Namespace(amplicon_seq=amp, guide_seq=amp[105:125], cleavage_offset=-3, window_around_sgrna=1,
                              exclude_bp_from_left=15, exclude_bp_from_right=15, coding_seq=None,
                              expected_hdr_amplicon_seq=None)
    clock = time.perf_counter
    with GpuAligner(0) as al, quantify.GpuQuantifier(0) as q, alleles.GpuAlleleGrouper(0) as grouper:
        al.set_reference(amp)
        al.set_output("ops")
        al.upload(buf, off)
        al.run_async()
        align_ms = al.sync()
        dev = al.device_ops()
        ob = al.download_ops(n)
        score = _printed_percents(ob.stats["n_ident"], np.maximum(ob.stats["aln_len"], 1))
        keep = ((ob.stats["flags"] & 1) == 0) & (score > 60.0)
        g = quantify.globals_from_args(args)
        q.set_params(g, args)
        with DeviceBuffer.from_array(quantify.pre_flags(score == 100)) as d_pre, DeviceBuffer(16 * n) as d_out:
            q.run_device_ops(amp, dev, d_pre.ptr, n, d_out.ptr)
            rr = d_out.download(np.zeros((n, 4), np.int32))
        quant_ms = q.last_kernel_ms

        grouper.group(dev, n, keep=keep)                        # warm-up: buffers allocated
        phases, kernel_ms, call_s, table_s = [], [], [], []
        for _ in range(steps):
            t0 = clock()
            groups = grouper.group(dev, n, keep=keep)
            call_s.append(clock() - t0)
            kernel_ms.append(grouper.last_kernel_ms)
            phases.append(grouper.phase_times())
            t0 = clock()
            table = alleles.allele_table(amp, buf, off, ob, rr, groups)
            table_s.append(clock() - t0)

        # the path it replaces: one DataFrame row per read
        names = [f"r{i}" for i in range(n)]
        old = {"ops_to_dataframe_s": [], "column_fill_s": [], "groupby_s": []}
        for _ in range(steps):
            t0 = clock()
            df = ops_to_dataframe(ob, amp, buf, off, names, "ref")
            df = df.loc[(df.score_ref > 60.0).to_numpy()].copy()
            old["ops_to_dataframe_s"].append(clock() - t0)
            t0 = clock()
            res = rr[keep]
            cls = res[:, 0]
            df["UNMODIFIED"] = (df.score_ref == 100).to_numpy() | (cls == 0)
            df["NHEJ"] = cls == 1
            df["HDR"] = cls == 2
            df["MIXED"] = cls == 3
            df["n_mutated"] = res[:, 1].astype(np.int64)
            df["n_inserted"] = res[:, 2].astype(np.int64)
            df["n_deleted"] = res[:, 3].astype(np.int64)
            old["column_fill_s"].append(clock() - t0)
            t0 = clock()
            a = df.groupby(["align_seq", "ref_seq", "NHEJ", "UNMODIFIED", "HDR", "n_deleted", "n_inserted",
                            "n_mutated"]).size().reset_index()
            a = a.rename(columns={0: "#Reads", "align_seq": "Aligned_Sequence", "ref_seq": "Reference_Sequence"})
            a["%Reads"] = a["#Reads"] / a["#Reads"].sum() * 100.0
            a = a.sort_values(by="#Reads", ascending=False)
            old["groupby_s"].append(clock() - t0)
        pd.testing.assert_frame_equal(table.reset_index(drop=True), a.reset_index(drop=True))

    best = min
    new_s = best(call_s) + best(table_s)
    old_s = sum(best(v) for v in old.values())
    return {
        "workload": f"C2: {n} reads of a 250 bp amplicon, {int(keep.sum())} kept (identity > 60)",
        "groups": len(groups), "alleles": len(table), "collided": groups.collided,
        "aligner_resident_ms": align_ms, "quantification_kernel_ms": quant_ms,
        "grouping_kernel_ms": {k: best(p[k] for p in phases) for k in phases[0]},
        "grouping_kernels_total_ms": best(kernel_ms),
        "grouping_call_s": best(call_s),
        "allele_table_s": best(table_s),
        "new_path_s": new_s,
        "existing_path_s": {k: best(v) for k, v in old.items()},
        "existing_path_total_s": old_s,
        "existing_over_new": old_s / new_s,
        "tables_equal": True,
        "steps": steps, "statistic": "minimum over the steps",
    }


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=int(os.environ.get("ALLELES_BENCH_READS", "1000000")))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=480, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r01_alleles", "bench_alleles.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.reads, a.steps)))
        return 0
    # the GPU step: a process of its own under its own time limit
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reads", str(a.reads), "--steps",
                        str(a.steps)], capture_output=True, text=True, timeout=a.timeout)
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
