#!/usr/bin/env python3
"""Allele tables of the per-amplicon result folders from HBM: ``summarize_pooled(reports=...,
alleles=True)`` against the host path that yields the same tables, and the call without
``alleles`` (the figure to hold against an earlier tree).

Input (seeded): scripts/bench_pooled_reports.py's panel -- ``--reads`` reads (default 1M) of
about 220 bp over ``synth.pooled_amplicons(96)``, every odd read reverse-complemented,
interleaved; here every amplicon also gets an sgRNA (20 bases around its middle), so that every
folder has a table around a cut site.  In one process, after a warm-up round in which the tables
are compared (``assert_frame_equal``), ``--rounds`` alternated rounds of

* ``demux.summarize_pooled`` with a ``reports`` callback and no ``alleles`` (``--plain-only``
  times nothing else, gives the rows no sgRNA and uses no new keyword, so that the same script
  measures an earlier tree: ``--root`` names the tree whose package is imported);
* the same with ``alleles=True``;
* the host path to the same tables: ``demux.align_demultiplexed`` (rows on the host), per
  amplicon the printed identities and the ``> 60`` filter (``needle.batch_to_dataframe``),
  ``quantify.quantify_alignments``, ``quantify.run_summary`` (its ``df_alleles``) and
  ``alleles.around_cut_from_alleles`` per cut point.

Also the new kernels' time by events, summed over the groups of a call (``alleles``: grouping and
the representative rows; ``around_cut``: windows, their grouping, gather), and the host's wall
time of the two steps.  Each figure is the median of the rounds with its range.  No time is a pass
condition: the numbers are written as measured, to ``--out`` (default
profiles/r01_pooled_alleles/bench_pooled_alleles.json) and to stdout."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIN_READS, SCORE, OFFSET = 1000, 60.0, 20


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": list(xs)}


def measure(n_reads: int, rounds: int, plain_only: bool) -> dict:
    import numpy as np

    from bench_demux import workload
    from crispresso_amd import demux, needle, quantify
    from crispresso_amd.aligner import GpuAligner

    amps, flat, text, offsets = workload(n_reads)
    reads = (text, offsets)
    rows = [{"Name": "A%d" % g, "Amplicon_Sequence": a, "Expected_HDR": "", "Coding_sequence": "",
             "sgRNA": "" if plain_only else a[len(a) // 2 - 10:len(a) // 2 + 10]} for g, a in enumerate(amps)]
    print("workload made", file=sys.stderr, flush=True)
    clock = time.perf_counter
    out = {"workload": f"{n_reads} reads of {len(text) / n_reads:.1f} bp on average over {len(amps)} amplicons, odd "
                       "reads reverse-complemented" + ("" if plain_only else ", an sgRNA around every amplicon's middle"),
           "min_reads": MIN_READS, "min_identity_score": SCORE, "rounds": rounds, "plain_only": plain_only,
           "offset_around_cut": OFFSET,
           "statistic": "median (min, max) of the alternated rounds after one checked warm-up round; seconds unless named ms"}
    opts = dict(window_around_sgrna=1, cleavage_offset=-3, exclude_bp_from_left=15, exclude_bp_from_right=15)

    def host_path(gq, d, al):
        """{g: (df_alleles, [around-cut frames])} by the earlier API."""
        from crispresso_amd import alleles

        batches, _, skipped = demux.align_demultiplexed(amps, reads, al, min_reads=MIN_READS, demultiplexer=d)
        got = {}
        for g, (row, batch) in enumerate(zip(rows, batches)):
            if g in skipped:
                continue
            amp = row["Amplicon_Sequence"]
            df = needle.batch_to_dataframe(batch, [str(i) for i in range(len(batch))], "ref")
            df = df[df["score_ref"] > SCORE]
            args = types.SimpleNamespace(
                amplicon_seq=amp, guide_seq=row["sgRNA"] or None, coding_seq=None, ignore_substitutions=False,
                ignore_insertions=False, ignore_deletions=False, hide_mutations_outside_window_NHEJ=False,
                expected_hdr_amplicon_seq=None, **opts)
            res = quantify.quantify_alignments(df.copy(), args, quantifier=gq, globals_=quantify.globals_from_args(args))
            cuts = quantify.compute_cut_points(amp, args.guide_seq, args.cleavage_offset)
            table = quantify.run_summary(res[0], len(amp), cuts)["df_alleles"]
            pairs = list(zip(args.guide_seq.split(","), cuts)) if args.guide_seq else []
            got[g] = (table, [alleles.around_cut_from_alleles(table, c, OFFSET) for _, c in pairs])
        return got

    names = ["summarize_pooled_reports"] if plain_only else \
        ["summarize_pooled_reports", "summarize_pooled_alleles", "host_path_alleles", "alleles_kernel_ms",
         "around_cut_kernel_ms", "alleles_wall_ms", "around_cut_wall_ms"]
    T = {k: [] for k in names}
    with demux.GpuDemultiplexer(0) as d, GpuAligner(0) as al, quantify.GpuQuantifier(0) as gq, \
            demux.GpuSummarizer(0) as gs:
        kw = dict(min_reads=MIN_READS, min_identity_score=SCORE, demultiplexer=d, quantifier=gq, summarizer=gs)
        for rnd in range(rounds + 1):
            print(f"round {rnd} of {rounds}", file=sys.stderr, flush=True)
            plain_reports = {}
            t0 = clock()
            plain = demux.summarize_pooled(rows, reads, al, reports=lambda g, rep: plain_reports.__setitem__(g, rep), **kw)
            t_plain = clock() - t0
            if not plain_only:
                reports = {}
                t0 = clock()
                with_alleles = demux.summarize_pooled(rows, reads, al, reports=lambda g, rep: reports.__setitem__(g, rep),
                                                      alleles=True, offset_around_cut=OFFSET, **kw)
                t_alleles = clock() - t0
                t0 = clock()
                host = host_path(gq, d, al)
                t_host = clock() - t0
            if rnd == 0:        # the warm-up round, checked
                out["reads_kept"] = int(plain.counts[:, 1].sum())
                out["counts_digest"] = int((plain.counts[:, :6] * np.arange(1, 7)).sum())
                if not plain_only:
                    from pandas.testing import assert_frame_equal

                    if not np.array_equal(with_alleles.counts, plain.counts):
                        raise SystemExit("the counts with alleles differ from the counts without")
                    if sorted(host) != sorted(reports):
                        raise SystemExit("the host path and the reports cover different amplicons")
                    for g, (table, around) in host.items():
                        assert_frame_equal(reports[g].alleles, table)
                        if len(around) != len(reports[g].around_cut):
                            raise SystemExit(f"amplicon {g}: {len(reports[g].around_cut)} around-cut tables")
                        for (_, _, frame), want in zip(reports[g].around_cut, around):
                            assert_frame_equal(frame, want)
                    out["equal_to_host_path"] = True
                    out["groups"] = len(reports)
                    out["alleles"] = int(sum(len(r.alleles) for r in reports.values()))
                    out["around_cut_tables"] = int(sum(len(r.around_cut) for r in reports.values()))
                continue
            T["summarize_pooled_reports"].append(t_plain)
            if not plain_only:
                T["summarize_pooled_alleles"].append(t_alleles)
                T["host_path_alleles"].append(t_host)
                T["alleles_kernel_ms"].append(with_alleles.kernel_ms["alleles"])
                T["around_cut_kernel_ms"].append(with_alleles.kernel_ms["around_cut"])
                T["alleles_wall_ms"].append(with_alleles.kernel_ms["alleles_wall"])
                T["around_cut_wall_ms"].append(with_alleles.kernel_ms["around_cut_wall"])
    out.update({k: summary(v) for k, v in T.items()})
    if not plain_only:
        out["alleles_over_host_path"] = out["summarize_pooled_alleles"]["median"] / out["host_path_alleles"]["median"]
        out["alleles_over_reports"] = out["summarize_pooled_alleles"]["median"] / out["summarize_pooled_reports"]["median"]
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=int(os.environ.get("DEMUX_BENCH_READS", "1000000")))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true", help="time only the call without alleles")
    ap.add_argument("--root", default=ROOT, help="the tree whose crispresso_amd and scripts are measured")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r01_pooled_alleles", "bench_pooled_alleles.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    if a.child:
        sys.path.insert(0, root)
        sys.path.insert(0, os.path.join(root, "scripts"))
        print(json.dumps(measure(a.reads, a.rounds, a.plain_only)))
        return 0
    # the GPU step: a process of its own under its own time limit
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reads", str(a.reads), "--rounds", str(a.rounds),
           "--root", root]
    p = subprocess.run(cmd + (["--plain-only"] if a.plain_only else []), stdout=subprocess.PIPE, text=True,
                       timeout=a.timeout)   # (its progress: stderr)
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
