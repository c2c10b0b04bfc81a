#!/usr/bin/env python3
"""Raw reads to the per-amplicon summary in HBM against today's round trip per group.

Input (seeded): scripts/bench_demux.py's panel -- ``--reads`` reads (default 1M) of about 220 bp
over ``synth.pooled_amplicons(96)``, every odd read reverse-complemented, interleaved; as pairs,
R1 = a read's first 150 bases and R2 = the reverse complement of its last 150, constant quality.
In one process, after a warm-up round in which the results are compared, ``--rounds`` alternated
rounds of

* ``demux.summarize_pooled`` on the host reads, against ``demux.align_demultiplexed_resident``
  with an ``on_group`` that does what a caller had to do before: ``download_ops``, the printed
  identities and the ``> 60`` filter on the host, ``pre_flags`` uploaded, ``run_device_ops``, the
  per-read results downloaded and counted with pandas (the consumer of
  tests/test_gpu_demux_resident.py without the allele table).  That baseline uses nothing this
  stage adds;
* from pairs: ``frontend.prepare_packed_resident`` -> ``summarize_pooled`` on the resident reads,
  against ``frontend.prepare_packed`` -> the baseline on the fetched text;
* the two new kernels by HIP events, summed over the groups of a call.

Each figure is the median of the rounds with its range; host clocks surround work that ends in a
device synchronise.  No ratio is required: the numbers are written as measured, to ``--out``
(default profiles/r01_pooled_summary/bench_pooled_summary.json) and to stdout."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

MIN_READS, SCORE = 1000, 60.0


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": list(xs)}


def measure(n_reads: int, rounds: int) -> dict:
    import numpy as np
    import pandas as pd

    from bench_demux import workload
    from crispresso_amd import _lib, demux, frontend, quantify
    from crispresso_amd.aligner import GpuAligner
    from crispresso_amd.devmem import DeviceBuffer
    from crispresso_amd.needle import _printed_percents
    from tests import demux_model as dm

    amps, flat, text, offsets = workload(n_reads)
    reads = (text, offsets)
    rows = [{"Name": "A%d" % g, "Amplicon_Sequence": a, "sgRNA": "", "Expected_HDR": "", "Coding_sequence": ""}
            for g, a in enumerate(amps)]
    r1 = [r[:150] for r in flat]
    r2 = [dm.revcomp(r[-150:]) for r in flat]
    s1 = np.frombuffer(b"".join(r1), np.uint8)
    s2 = np.frombuffer(b"".join(r2), np.uint8)
    off1, off2 = np.zeros(n_reads + 1, np.int64), np.zeros(n_reads + 1, np.int64)
    np.cumsum(np.fromiter((len(r) for r in r1), np.int64, n_reads), out=off1[1:])
    np.cumsum(np.fromiter((len(r) for r in r2), np.int64, n_reads), out=off2[1:])
    q1, q2 = np.full(len(s1), ord("I"), np.uint8), np.full(len(s2), ord("I"), np.uint8)
    pairs = (s1, q1, off1, s2, q2, off2)
    del flat, r1, r2
    print("workload made", file=sys.stderr, flush=True)
    clock = time.perf_counter
    out = {"workload": f"{n_reads} reads of {len(text) / n_reads:.1f} bp on average over {len(amps)} amplicons, odd "
                       "reads reverse-complemented; as pairs: 150 + 150 bases, constant quality",
           "min_reads": MIN_READS, "min_identity_score": SCORE, "rounds": rounds,
           "statistic": "median (min, max) of the alternated rounds after one checked warm-up round; seconds unless named ms",
           "text_bytes": int(len(text)), "pair_bytes": int(2 * (len(s1) + len(s2)))}

    def quant_args(amp):
        return types.SimpleNamespace(
            amplicon_seq=amp, guide_seq=None, cleavage_offset=-3, window_around_sgrna=1, exclude_bp_from_left=15,
            exclude_bp_from_right=15, coding_seq=None, ignore_substitutions=False, ignore_insertions=False,
            ignore_deletions=False, hide_mutations_outside_window_NHEJ=False, expected_hdr_amplicon_seq=None)

    def baseline(gq, d, al, host_reads):
        """The round trip per group; returns ({g: the counts a summary needs}, seconds inside on_group)."""
        counts, spent = {}, [0.0]

        def on_group(g, a, n):
            t0 = clock()
            dev = a.device_ops()
            ob = a.download_ops(n)
            score = _printed_percents(ob.stats["n_ident"], np.maximum(ob.stats["aln_len"], 1))
            keep = ((ob.stats["flags"] & _lib.NW_FLAG_EMPTY) == 0) & (score > SCORE)
            args = quant_args(amps[g])
            gq.set_params(quantify.globals_from_args(args), args)
            um = score == 100
            with DeviceBuffer.from_array(quantify.pre_flags(um)) as d_pre, DeviceBuffer(16 * n) as d_out:
                gq.run_device_ops(amps[g], dev, d_pre.ptr, n, d_out.ptr)
                rr = d_out.download(np.zeros((n, 4), np.int32))
            df = pd.DataFrame({"keep": keep, "UNMODIFIED": um | (rr[:, 0] == 0), "NHEJ": rr[:, 0] == 1,
                               "HDR": rr[:, 0] == 2, "MIXED": rr[:, 0] == 3})
            df = df[df["keep"]]
            counts[g] = [n, int(df.shape[0]), int(df["UNMODIFIED"].sum()), int(df["NHEJ"].sum()), int(df["HDR"].sum()),
                         int(df["MIXED"].sum())]
            spent[0] += clock() - t0

        demux.align_demultiplexed_resident(amps, host_reads, al, min_reads=MIN_READS, on_group=on_group,
                                           demultiplexer=d)
        return counts, spent[0]

    def same(ps, counts):
        return all(ps.counts[g, :6].tolist() == c for g, c in counts.items()) and \
            sorted(counts) == [g for g in range(len(amps)) if g not in ps.skipped]

    T = {k: [] for k in ("summarize_pooled", "baseline_round_trip", "baseline_on_group", "pairs_resident_total",
                         "pairs_resident_prepare", "pairs_resident_summarize", "pairs_host_total", "pairs_host_prepare",
                         "pairs_host_baseline", "flags_kernel_ms", "summary_kernel_ms", "quantify_kernel_ms")}
    with demux.GpuDemultiplexer(0) as d, GpuAligner(0) as al, quantify.GpuQuantifier(0) as gq, \
            demux.GpuSummarizer(0) as gs:
        kw = dict(min_reads=MIN_READS, min_identity_score=SCORE, demultiplexer=d, quantifier=gq, summarizer=gs)
        for rnd in range(rounds + 1):
            print(f"round {rnd} of {rounds}", file=sys.stderr, flush=True)
            t0 = clock()
            ps = demux.summarize_pooled(rows, reads, al, **kw)
            t_new = clock() - t0
            t0 = clock()
            counts, t_group = baseline(gq, d, al, reads)
            t_old = clock() - t0
            # from pairs
            al.set_reference(amps[0])
            t0 = clock()
            with frontend.prepare_packed_resident(al, *pairs) as rr:
                t1 = clock()
                pps = demux.summarize_pooled(rows, rr, al, **kw)
                m = len(rr)
            t2 = clock()
            al.set_reference(amps[0])
            t3 = clock()
            pb = frontend.prepare_packed(al, *pairs)
            t4 = clock()
            pcounts, _ = baseline(gq, d, al, (pb.buf, pb.offsets))
            t5 = clock()
            if rnd == 0:        # the warm-up round, checked
                if not same(ps, counts):
                    raise SystemExit("summarize_pooled's counts differ from the round trip's")
                if not same(pps, pcounts):
                    raise SystemExit("from pairs: summarize_pooled's counts differ from the round trip's")
                out["equal_to_round_trip"] = True
                out["groups"] = len(counts)
                out["reads_kept"] = int(ps.counts[:, 1].sum())
                out["pairs_merged"] = int(m)
                out["pairs_groups"] = len(pcounts)
                out["merged_text_bytes"] = int(pb.offsets[-1])
                continue
            T["summarize_pooled"].append(t_new)
            T["baseline_round_trip"].append(t_old)
            T["baseline_on_group"].append(t_group)
            T["pairs_resident_total"].append(t2 - t0)
            T["pairs_resident_prepare"].append(t1 - t0)
            T["pairs_resident_summarize"].append(t2 - t1)
            T["pairs_host_total"].append(t5 - t3)
            T["pairs_host_prepare"].append(t4 - t3)
            T["pairs_host_baseline"].append(t5 - t4)
            T["flags_kernel_ms"].append(ps.kernel_ms["flags"])
            T["summary_kernel_ms"].append(ps.kernel_ms["summary"])
            T["quantify_kernel_ms"].append(ps.kernel_ms["quantify"])
    out.update({k: summary(v) for k, v in T.items()})
    out["summarize_over_round_trip"] = out["summarize_pooled"]["median"] / out["baseline_round_trip"]["median"]
    out["pairs_resident_over_host"] = out["pairs_resident_total"]["median"] / out["pairs_host_total"]["median"]
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=int(os.environ.get("DEMUX_BENCH_READS", "1000000")))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r01_pooled_summary", "bench_pooled_summary.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.reads, a.rounds)))
        return 0
    # the GPU step: a process of its own under its own time limit
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reads", str(a.reads), "--rounds",
                        str(a.rounds)], stdout=subprocess.PIPE, text=True, timeout=a.timeout)   # (its progress: stderr)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:])
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
