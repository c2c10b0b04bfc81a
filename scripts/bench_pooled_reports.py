#!/usr/bin/env python3
"""Per-amplicon result folders from HBM: ``summarize_pooled(reports=...)`` against the call without
reports and against the host path that yields the same tables.

Input (seeded): scripts/bench_demux.py's panel -- ``--reads`` reads (default 1M) of about 220 bp
over ``synth.pooled_amplicons(96)``, every odd read reverse-complemented, interleaved; the panel
of scripts/bench_pooled_summary.py.  In one process, after a warm-up round in which the results
are compared, ``--rounds`` alternated rounds of

* ``demux.summarize_pooled`` without ``reports`` (``--plain-only`` times nothing else and uses no
  new keyword, so that the same script measures an earlier tree);
* the same with a ``reports`` callback that builds the four histogram tables of every amplicon
  (``report.tables``);
* the same with a callback that also writes every amplicon's folder (``report.write_report``)
  into a fresh temporary directory;
* the host path that yields the same tables: ``demux.align_demultiplexed`` (rows on the host),
  then per amplicon the printed identities and the ``> 60`` filter
  (``needle.batch_to_dataframe``), ``quantify.quantify_alignments`` and ``quantify.run_summary``.

Also the two new kernels' time by events, summed over the groups of a call.  Each figure is the
median of the rounds with its range; host clocks surround work that ends in a device synchronise.
No time is a pass condition: the numbers are written as measured, to ``--out`` (default
profiles/r01_pooled_reports/bench_pooled_reports.json) and to stdout."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

MIN_READS, SCORE = 1000, 60.0
TABLES = ("df_indels", "df_insertion", "df_deletion", "df_substitution")


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": list(xs)}


def measure(n_reads: int, rounds: int, plain_only: bool) -> dict:
    import numpy as np

    from bench_demux import workload
    from crispresso_amd import demux, needle, quantify
    from crispresso_amd.aligner import GpuAligner

    amps, flat, text, offsets = workload(n_reads)
    reads = (text, offsets)
    rows = [{"Name": "A%d" % g, "Amplicon_Sequence": a, "sgRNA": "", "Expected_HDR": "", "Coding_sequence": ""}
            for g, a in enumerate(amps)]
    print("workload made", file=sys.stderr, flush=True)
    clock = time.perf_counter
    out = {"workload": f"{n_reads} reads of {len(text) / n_reads:.1f} bp on average over {len(amps)} amplicons, odd "
                       "reads reverse-complemented",
           "min_reads": MIN_READS, "min_identity_score": SCORE, "rounds": rounds, "plain_only": plain_only,
           "statistic": "median (min, max) of the alternated rounds after one checked warm-up round; seconds unless named ms",
           "text_bytes": int(len(text))}
    opts = dict(window_around_sgrna=1, cleavage_offset=-3, exclude_bp_from_left=15, exclude_bp_from_right=15)

    def host_path(gq, d, al):
        """{g: run_summary's output} by the earlier API."""
        batches, _, skipped = demux.align_demultiplexed(amps, reads, al, min_reads=MIN_READS, demultiplexer=d)
        got = {}
        for g, (amp, batch) in enumerate(zip(amps, batches)):
            if g in skipped:
                continue
            df = needle.batch_to_dataframe(batch, [str(i) for i in range(len(batch))], "ref")
            df = df[df["score_ref"] > SCORE]
            args = types.SimpleNamespace(
                amplicon_seq=amp, guide_seq=None, coding_seq=None, ignore_substitutions=False, ignore_insertions=False,
                ignore_deletions=False, hide_mutations_outside_window_NHEJ=False, expected_hdr_amplicon_seq=None, **opts)
            res = quantify.quantify_alignments(df.copy(), args, quantifier=gq, globals_=quantify.globals_from_args(args))
            got[g] = (quantify.run_summary(res[0], len(amp), []), res)
        return got

    names = ["summarize_pooled_plain"] if plain_only else \
        ["summarize_pooled_plain", "summarize_pooled_tables", "summarize_pooled_folders", "host_path_tables",
         "mask_kernel_ms", "histograms_kernel_ms", "quantify_kernel_ms", "summary_kernel_ms"]
    T = {k: [] for k in names}
    with demux.GpuDemultiplexer(0) as d, GpuAligner(0) as al, quantify.GpuQuantifier(0) as gq, \
            demux.GpuSummarizer(0) as gs:
        kw = dict(min_reads=MIN_READS, min_identity_score=SCORE, demultiplexer=d, quantifier=gq, summarizer=gs)
        for rnd in range(rounds + 1):
            print(f"round {rnd} of {rounds}", file=sys.stderr, flush=True)
            t0 = clock()
            plain = demux.summarize_pooled(rows, reads, al, **kw)
            t_plain = clock() - t0
            if not plain_only:
                from crispresso_amd import report

                tables, reports = {}, {}

                def build(g, rep):
                    reports[g] = rep
                    tables[g] = report.tables(rep)

                t0 = clock()
                with_tables = demux.summarize_pooled(rows, reads, al, reports=build, **kw)
                t_tables = clock() - t0
                folder = tempfile.mkdtemp(prefix="pooled_reports_")
                try:
                    def write(g, rep):
                        report.write_report(os.path.join(folder, report.folder_name(rep.name)), rep)

                    t0 = clock()
                    demux.summarize_pooled(rows, reads, al, reports=write, **kw)
                    t_folders = clock() - t0
                    n_folders = len(os.listdir(folder))
                finally:
                    shutil.rmtree(folder, ignore_errors=True)
                t0 = clock()
                host = host_path(gq, d, al)
                t_host = clock() - t0
            if rnd == 0:        # the warm-up round, checked
                out["plain_reads_kept"] = int(plain.counts[:, 1].sum())
                out["plain_counts_digest"] = int((plain.counts[:, :6] * np.arange(1, 7)).sum())
                if not plain_only:
                    if not np.array_equal(with_tables.counts, plain.counts):
                        raise SystemExit("the counts with reports differ from the counts without")
                    if sorted(host) != sorted(tables) or n_folders != len(tables):
                        raise SystemExit("the host path and the reports cover different amplicons")
                    for g, (s, res) in host.items():
                        for key in TABLES:
                            if not tables[g][key].equals(s[key]):
                                raise SystemExit(f"amplicon {g}: {key} differs from the host path's")
                        v = reports[g].totals["vectors"]
                        for k, name in enumerate(quantify.VECTOR_NAMES[:13]):
                            if not np.array_equal(v[name], res[1 + k]):
                                raise SystemExit(f"amplicon {g}: {name} differs from the host path's")
                    out["equal_to_host_path"] = True
                    out["groups"] = len(tables)
                    out["reads_modified"] = int(plain.counts[:, 3].sum())
                continue
            T["summarize_pooled_plain"].append(t_plain)
            if not plain_only:
                T["summarize_pooled_tables"].append(t_tables)
                T["summarize_pooled_folders"].append(t_folders)
                T["host_path_tables"].append(t_host)
                T["mask_kernel_ms"].append(with_tables.kernel_ms["mask"])
                T["histograms_kernel_ms"].append(with_tables.kernel_ms["histograms"])
                T["quantify_kernel_ms"].append(with_tables.kernel_ms["quantify"])
                T["summary_kernel_ms"].append(with_tables.kernel_ms["summary"])
    out.update({k: summary(v) for k, v in T.items()})
    if not plain_only:
        out["tables_over_host_path"] = out["summarize_pooled_tables"]["median"] / out["host_path_tables"]["median"]
        out["tables_over_plain"] = out["summarize_pooled_tables"]["median"] / out["summarize_pooled_plain"]["median"]
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=int(os.environ.get("DEMUX_BENCH_READS", "1000000")))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true", help="time only the call without reports")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r01_pooled_reports", "bench_pooled_reports.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.reads, a.rounds, a.plain_only)))
        return 0
    # the GPU step: a process of its own under its own time limit
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reads", str(a.reads), "--rounds", str(a.rounds)]
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
