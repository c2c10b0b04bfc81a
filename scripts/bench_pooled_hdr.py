#!/usr/bin/env python3
"""Expected_HDR rows in the pooled summary: ``summarize_pooled(allow_hdr=True)`` against what a
caller had to write before it.

Input (seeded): scripts/bench_demux.py's panel -- ``--reads`` reads (default 1M) of about 220 bp
over ``synth.pooled_amplicons(96)``, every odd read reverse-complemented, interleaved.  Every
second amplicon has an ``Expected_HDR`` that replaces a 10-base block in its middle, and every
fifth read of those amplicons is a copy of it.  In one process, after a warm-up round in which
the counts are compared, ``--rounds`` alternated rounds of

* ``demux.summarize_pooled(allow_hdr=True)`` on the host reads;
* the yardstick, which uses nothing this stage adds: ``demux.align_demultiplexed_resident`` once
  per reference.  The first call has the Expected_HDR amplicons as references (the amplicon where
  a row has none; its ``on_group`` downloads the records and prints the repaired identity), the
  second the amplicons (``on_group``: ``download_ops``, both printed identities, the filter and
  ``pre_flags`` on the host, ``pre`` uploaded, ``run_device_ops``, the per-read results downloaded
  and counted with pandas).  The first call demultiplexes against the Expected_HDR amplicons and
  aligns the rows without one a second time: the earlier API offers no way round either;
* the unchanged call: ``summarize_pooled`` on the same reads with the ``Expected_HDR`` column
  blank.  ``--plain-only`` times nothing else and uses no new keyword, so that the same script
  measures an earlier tree.

Each figure is the median of the rounds with its range; host clocks surround work that ends in a
device synchronise.  No time is a pass condition: the numbers are written as measured, to
``--out`` (default profiles/r01_pooled_hdr/bench_pooled_hdr.json) and to stdout."""
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

MIN_READS, SCORE, THRESHOLD = 1000, 60.0, 98.0


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": list(xs)}


def hdr_workload(n_reads: int):
    """(rows, text, offsets): the panel with the Expected_HDR alleles put in."""
    import numpy as np

    from bench_demux import workload
    from tests import demux_model as dm

    amps, flat, _, _ = workload(n_reads)
    swap = str.maketrans("ACGT", "GTAC")
    rows = []
    for g, a in enumerate(amps):
        mid = len(a) // 2
        hdr = a[:mid] + a[mid:mid + 10].translate(swap) + a[mid + 10:] if g % 2 == 0 else ""
        rows.append({"Name": "A%d" % g, "Amplicon_Sequence": a, "sgRNA": "", "Expected_HDR": hdr, "Coding_sequence": ""})
    for i in range(n_reads):
        g = i % len(amps)
        if g % 2 == 0 and (i // len(amps)) % 5 == 0:
            h = rows[g]["Expected_HDR"].encode()
            flat[i] = dm.revcomp(h) if i % 2 else h
    text = np.frombuffer(b"".join(flat), np.uint8)
    offsets = np.zeros(n_reads + 1, np.int64)
    np.cumsum(np.fromiter((len(r) for r in flat), np.int64, n_reads), out=offsets[1:])
    return rows, text, offsets


def measure(n_reads: int, rounds: int, plain_only: bool) -> dict:
    import numpy as np
    import pandas as pd

    from crispresso_amd import _lib, demux, quantify
    from crispresso_amd.aligner import GpuAligner
    from crispresso_amd.devmem import DeviceBuffer
    from crispresso_amd.needle import _printed_percents

    rows, text, offsets = hdr_workload(n_reads)
    reads = (text, offsets)
    amps = [r["Amplicon_Sequence"] for r in rows]
    hdrs = [r["Expected_HDR"] or None for r in rows]
    plain_rows = [dict(r, Expected_HDR="") for r in rows]
    print("workload made", file=sys.stderr, flush=True)
    clock = time.perf_counter
    out = {"workload": f"{n_reads} reads of {len(text) / n_reads:.1f} bp on average over {len(amps)} amplicons, odd reads "
                       f"reverse-complemented; {sum(h is not None for h in hdrs)} amplicons with an Expected_HDR that "
                       "replaces 10 bases, a fifth of their reads copies of it",
           "min_reads": MIN_READS, "min_identity_score": SCORE, "hdr_perfect_alignment_threshold": THRESHOLD,
           "rounds": rounds, "plain_only": plain_only,
           "statistic": "median (min, max) of the alternated rounds after one checked warm-up round; seconds unless named ms",
           "text_bytes": int(len(text))}

    def quant_args(g):
        return types.SimpleNamespace(
            amplicon_seq=amps[g], guide_seq=None, cleavage_offset=-3, window_around_sgrna=1, exclude_bp_from_left=15,
            exclude_bp_from_right=15, coding_seq=None, ignore_substitutions=False, ignore_insertions=False,
            ignore_deletions=False, hide_mutations_outside_window_NHEJ=False, expected_hdr_amplicon_seq=hdrs[g],
            hdr_perfect_alignment_threshold=THRESHOLD)

    def printed(stats):
        return _printed_percents(stats["n_ident"], np.maximum(stats["aln_len"], 1))

    def yardstick(gq, d, al):
        """Two calls of the earlier API; returns ({g: the counts a summary needs}, seconds inside on_group)."""
        repaired, counts, spent = {}, {}, [0.0]

        def on_hdr_group(g, a, n):
            t0 = clock()
            if hdrs[g] is not None:
                repaired[g] = printed(a.download_ops(n).stats)
            spent[0] += clock() - t0

        def on_group(g, a, n):
            t0 = clock()
            dev = a.device_ops()
            ob = a.download_ops(n)
            score = printed(ob.stats)
            live = (ob.stats["flags"] & _lib.NW_FLAG_EMPTY) == 0
            um = score == 100
            if hdrs[g] is not None:
                rep = repaired[g]
                keep = live & ((score > SCORE) | (rep > SCORE))
                pre = quantify.pre_flags(um, score - rep, rep, THRESHOLD)
            else:
                keep = live & (score > SCORE)
                pre = quantify.pre_flags(um)
            args = quant_args(g)
            gq.set_params(quantify.globals_from_args(args), args)
            with DeviceBuffer.from_array(pre) as d_pre, DeviceBuffer(16 * n) as d_out:
                gq.run_device_ops(amps[g], dev, d_pre.ptr, n, d_out.ptr)
                rr = d_out.download(np.zeros((n, 4), np.int32))
            df = pd.DataFrame({"keep": keep, "UNMODIFIED": um | (rr[:, 0] == 0), "NHEJ": rr[:, 0] == 1,
                               "HDR": rr[:, 0] == 2, "MIXED": rr[:, 0] == 3})
            df = df[df["keep"]]
            counts[g] = [n, int(df.shape[0]), int(df["UNMODIFIED"].sum()), int(df["NHEJ"].sum()), int(df["HDR"].sum()),
                         int(df["MIXED"].sum())]
            spent[0] += clock() - t0

        _, first, _ = demux.align_demultiplexed_resident([h or a for h, a in zip(hdrs, amps)], reads, al,
                                                         min_reads=MIN_READS, on_group=on_hdr_group, demultiplexer=d)
        _, second, _ = demux.align_demultiplexed_resident(amps, reads, al, min_reads=MIN_READS, on_group=on_group,
                                                          demultiplexer=d)
        if not np.array_equal(first.which, second.which):
            raise SystemExit("the yardstick's two calls assign the reads differently")
        return counts, spent[0]

    def same(ps, counts):
        return all(ps.counts[g, :6].tolist() == c for g, c in counts.items()) and \
            sorted(counts) == [g for g in range(len(amps)) if g not in ps.skipped]

    names = ["summarize_pooled_plain"] if plain_only else \
        ["summarize_pooled_hdr", "yardstick_two_calls", "yardstick_on_group", "summarize_pooled_plain", "flags_kernel_ms",
         "printed_kernel_ms", "summary_kernel_ms", "quantify_kernel_ms", "hdr_pass_ms"]
    T = {k: [] for k in names}
    with demux.GpuDemultiplexer(0) as d, GpuAligner(0) as al, quantify.GpuQuantifier(0) as gq, \
            demux.GpuSummarizer(0) as gs:
        kw = dict(min_reads=MIN_READS, min_identity_score=SCORE, demultiplexer=d, quantifier=gq, summarizer=gs)
        for rnd in range(rounds + 1):
            print(f"round {rnd} of {rounds}", file=sys.stderr, flush=True)
            if not plain_only:
                t0 = clock()
                ps = demux.summarize_pooled(rows, reads, al, allow_hdr=True, hdr_perfect_alignment_threshold=THRESHOLD, **kw)
                t_new = clock() - t0
                t0 = clock()
                counts, t_group = yardstick(gq, d, al)
                t_old = clock() - t0
            t0 = clock()
            plain = demux.summarize_pooled(plain_rows, reads, al, **kw)
            t_plain = clock() - t0
            if rnd == 0:        # the warm-up round, checked
                out["plain_reads_kept"] = int(plain.counts[:, 1].sum())
                out["plain_counts_digest"] = int((plain.counts[:, :6] * np.arange(1, 7)).sum())
                if not plain_only:
                    if not same(ps, counts):
                        raise SystemExit("summarize_pooled(allow_hdr=True)'s counts differ from the yardstick's")
                    if not (ps.counts[::2, 4] > 0).all() or ps.counts[1::2, 4:6].any():
                        raise SystemExit("the HDR counts are not where the panel puts them")
                    out["equal_to_yardstick"] = True
                    out["groups"] = len(counts)
                    out["reads_kept"] = int(ps.counts[:, 1].sum())
                    out["reads_hdr"] = int(ps.counts[:, 4].sum())
                    out["reads_mixed"] = int(ps.counts[:, 5].sum())
                continue
            T["summarize_pooled_plain"].append(t_plain)
            if not plain_only:
                T["summarize_pooled_hdr"].append(t_new)
                T["yardstick_two_calls"].append(t_old)
                T["yardstick_on_group"].append(t_group)
                T["flags_kernel_ms"].append(ps.kernel_ms["flags"])
                T["printed_kernel_ms"].append(ps.kernel_ms["printed"])
                T["summary_kernel_ms"].append(ps.kernel_ms["summary"])
                T["quantify_kernel_ms"].append(ps.kernel_ms["quantify"])
                T["hdr_pass_ms"].append(ps.kernel_ms["hdr_pass"])
    out.update({k: summary(v) for k, v in T.items()})
    if not plain_only:
        out["hdr_over_yardstick"] = out["summarize_pooled_hdr"]["median"] / out["yardstick_two_calls"]["median"]
        out["hdr_over_plain"] = out["summarize_pooled_hdr"]["median"] / out["summarize_pooled_plain"]["median"]
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=int(os.environ.get("DEMUX_BENCH_READS", "1000000")))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true", help="time only the call without Expected_HDR rows")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r01_pooled_hdr", "bench_pooled_hdr.json"))
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
