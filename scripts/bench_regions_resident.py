#!/usr/bin/env python3
"""A BAM's region reads to the summary inside HBM against the path a caller had before.

Input (seeded): the 1M records of 150 bp and 100 regions of scripts/bench_regions.py (WGS mode)
and the same records with the positions of scripts/bench_discover.py (genome mode, ``min_reads``
1000), with the bases rewritten so that every record reads the genome at its position through its
CIGAR (a random genome per reference; inserted bases random; 1 % ``N``; 0.2 % substitutions), and
that genome as the FASTA's content: the amplicon of a region is its stretch of it.  In one
process, after a warm-up round in which the two results are compared, ``--rounds`` alternated
rounds of

* ``extract_regions_resident`` / ``discover_regions_resident`` -> ``summarize_regions``;
* what a caller had: ``extract_regions`` / ``discover_regions`` (bases and qualities to the host),
  ``pooled.align_pooled`` on the regions that run, the printed identities and the ``> 60`` filter
  on the host (``needle.batch_to_dataframe``), ``quantify.quantify_alignments`` on the kept rows,
  ``quantify.run_summary``.

Each figure is the median of the rounds with its range; host clocks surround work that ends in a
device synchronise.  Also reported: the packer's kernels (HIP events), the extraction call alone
either way, and the share of ``summarize_regions`` that is its per-region loop.  No ratio is
required: the numbers are written as measured, to ``--out`` (default
profiles/r01_regions_resident/bench_regions_resident.json) and to stdout."""
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
SCORE = 60.0
SEQ_AT, READ = 57, 150          # where bench_regions.synthetic's records keep their bases


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": list(xs)}


def with_genome(plain, refs, f, n, seed=21):
    """The records of bench_regions.synthetic with their bases read off a random genome through
    their CIGARs; returns (plain, the genome's letters per reference)."""
    import numpy as np

    from tests import regions_cases as rc

    rng = np.random.Generator(np.random.PCG64(seed))
    codes = np.array([1, 2, 4, 8], np.uint8)
    genome = [codes[rng.integers(0, 4, length + 2 * READ)] for _, length in refs]
    head = len(rc.bam_plain(refs, []))
    size = (len(plain) - head) // n
    recs = np.frombuffer(plain, np.uint8, n * size, head).reshape(n, size).copy()
    j = np.arange(READ, dtype=np.int32)[None, :]
    for lo in range(0, n, 100000):
        hi = min(n, lo + 100000)
        p = (np.asarray(f["pos"][lo:hi], np.int64) - 1).astype(np.int32)[:, None]
        a, b = (np.asarray(f[k][lo:hi], np.int32)[:, None] for k in ("a", "b"))
        kind, ref = np.asarray(f["kind"][lo:hi])[:, None], np.asarray(f["ref"][lo:hi])[:, None]
        idx = p + j + np.where((kind == 1) & (j >= a), b, 0) - np.where((kind == 2) & (j >= a + b), b, 0)
        nib = np.where(ref == 0, genome[0][np.minimum(idx, len(genome[0]) - 1)], genome[1][np.minimum(idx, len(genome[1]) - 1)])
        ins = (kind == 2) & (j >= a) & (j < a + b)
        nib = np.where(ins | (rng.random(nib.shape) < 0.002), codes[rng.integers(0, 4, nib.shape)], nib)
        nib = np.where(rng.random(nib.shape) < 0.01, np.uint8(15), nib).astype(np.uint8)
        recs[lo:hi, SEQ_AT:SEQ_AT + READ // 2] = (nib[:, 0::2] << 4) | nib[:, 1::2]
    letters = np.frombuffer(rc.NIBBLES.encode(), np.uint8)
    return plain[:head] + recs.tobytes(), [letters[g].tobytes().decode() for g in genome]


def measure(n, rounds):
    import bench_discover as bd
    import bench_regions as br
    from crispresso_amd import needle, quantify
    from crispresso_amd import regions as rg
    from crispresso_amd.aligner import GpuAligner
    from crispresso_amd.pooled import align_pooled

    clock = time.perf_counter
    opts = dict(window_around_sgrna=1, cleavage_offset=-3, exclude_bp_from_left=15, exclude_bp_from_right=15)

    def host_path(bam, x, al, gq, regs, rows_of, min_reads, discover):
        """What a caller had: returns ({g: [reads, kept, unmodified, modified]}, seconds of the extraction)."""
        t0 = clock()
        res = rg.discover_regions(bam, min_reads, extractor=x) if discover else rg.extract_regions(bam, regs, extractor=x)
        t_extract = clock() - t0
        rows = rows_of(res)
        keep = [g for g in range(len(res)) if int(res.n_reads[g]) >= max(min_reads, 1) and rows[g]["Amplicon_Sequence"]]
        amps = [rows[g]["Amplicon_Sequence"] for g in keep]
        batches = align_pooled(amps, [res.reads(g) for g in keep], al)
        counts = {}
        for g, amp, batch in zip(keep, amps, batches):
            df = needle.batch_to_dataframe(batch, [str(i) for i in range(len(batch))], "ref")
            df = df[df["score_ref"] > SCORE]
            n_reads = int(res.n_reads[g])
            if df.shape[0] == 0:
                counts[g] = [n_reads, 0, 0, 0]
                continue
            args = types.SimpleNamespace(
                amplicon_seq=amp, guide_seq=None, coding_seq=None, ignore_substitutions=False, ignore_insertions=False,
                ignore_deletions=False, hide_mutations_outside_window_NHEJ=False, expected_hdr_amplicon_seq=None, **opts)
            out = quantify.quantify_alignments(df.copy(), args, quantifier=gq, globals_=quantify.globals_from_args(args))
            s = quantify.run_summary(out[0], len(amp), [])
            counts[g] = [n_reads, int(s["n_total"]), int(s["n_unmodified"]), int(s["n_modified"])]
        return counts, t_extract

    def resident_path(bam, x, al, gq, regs, rows_of, min_reads, discover):
        t0 = clock()
        res = rg.discover_regions_resident(bam, min_reads, extractor=x) if discover else \
            rg.extract_regions_resident(bam, regs, extractor=x)
        t1 = clock()
        with res:
            rows = rows_of(res)
            t2 = clock()
            rs = rg.summarize_regions(rows, res, al, min_reads=min_reads, min_identity_score=SCORE, quantifier=gq, **opts)
            t3 = clock()
            return rs, {"extract": t1 - t0, "rows": t2 - t1, "summarize": t3 - t2, "pack_ms": res.pack_ms,
                        "hits": len(res.src), "bases": int(res.text_offsets[-1]), "n_exc": res.n_exc}

    doc = {"rounds": rounds, "min_identity_score": SCORE,
           "statistic": "median (min, max) of the alternated rounds after one checked warm-up round; seconds unless named ms"}
    for mode in ("wgs", "genome"):
        discover = mode == "genome"
        if discover:
            plain, refs, regs, f = bd.synthetic(n)
        else:
            plain, refs, regs, f = br.synthetic(n, 100)
        plain, genome = with_genome(plain, refs, f, n)
        bam = rg.read_bam(plain)
        min_reads = 1000 if discover else 10
        print(f"{mode}: workload made", file=sys.stderr, flush=True)

        def seq(ref_id, s, e):
            return genome[ref_id][max(s, 1) - 1:max(e - 1, 0)]

        if discover:
            def rows_of(res):
                return [{"Name": name, "Amplicon_Sequence": seq(int(t["ref_id"]), int(t["bpstart"]), int(t["bpend"]))
                         if int(res.n_reads[g]) else "", "sgRNA": "", "Expected_HDR": "", "Coding_sequence": ""}
                        for g, (name, t) in enumerate(zip(res.target_names, res.region_table))]
        else:
            fixed = [{"Name": "R%d" % g, "Amplicon_Sequence": seq(*r), "sgRNA": "", "Expected_HDR": "", "Coding_sequence": ""}
                     for g, r in enumerate(regs)]

            def rows_of(res):
                return fixed

        T = {k: [] for k in ("resident_total", "resident_extract", "resident_summarize", "pack_kernel_ms", "host_total",
                             "host_extract", "flags_kernel_ms", "summary_kernel_ms", "quantify_kernel_ms")}
        out = {"workload": f"{n} records of {READ} bp; " + ("bench_discover.py's positions, min_reads 1000" if discover else
                                                          "bench_regions.py's 100 regions of 100 bp, min_reads 10"),
               "record_bytes": len(plain), "min_reads": min_reads}
        with rg.GpuRegionExtractor(0) as x, GpuAligner(0) as al, quantify.GpuQuantifier(0) as gq:
            for rnd in range(rounds + 1):
                print(f"{mode}: round {rnd} of {rounds}", file=sys.stderr, flush=True)
                t0 = clock()
                rs, parts = resident_path(bam, x, al, gq, regs, rows_of, min_reads, discover)
                t_new = clock() - t0
                t0 = clock()
                counts, t_extract = host_path(bam, x, al, gq, regs, rows_of, min_reads, discover)
                t_old = clock() - t0
                if rnd == 0:        # the warm-up round, checked
                    ran = [g for g in range(len(rs.counts)) if g not in rs.skipped]
                    if sorted(counts) != ran or any(rs.counts[g, :4].tolist() != counts[g] for g in ran):
                        raise SystemExit(f"{mode}: summarize_regions' counts differ from the host path's")
                    out.update(equal_to_host_path=True, regions_run=len(ran), hits=parts["hits"], bases=parts["bases"],
                               exceptions=parts["n_exc"], reads_kept=int(rs.counts[:, 1].sum()),
                               reads_modified=int(rs.counts[:, 3].sum()))
                    continue
                T["resident_total"].append(t_new)
                T["resident_extract"].append(parts["extract"])
                T["resident_summarize"].append(parts["summarize"])
                T["pack_kernel_ms"].append(parts["pack_ms"])
                T["host_total"].append(t_old)
                T["host_extract"].append(t_extract)
                for k in ("flags", "summary", "quantify"):
                    T[k + "_kernel_ms"].append(rs.kernel_ms[k])
        out.update({k: summary(v) for k, v in T.items()})
        out["resident_over_host"] = out["resident_total"]["median"] / out["host_total"]["median"]
        out["summarize_share_of_resident"] = out["resident_summarize"]["median"] / out["resident_total"]["median"]
        doc[mode] = out
        bam.close()
    return doc


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--records", type=int, default=int(os.environ.get("REGIONS_BENCH_RECORDS", "1000000")))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r01_regions_resident", "bench_regions_resident.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.records, a.rounds)))
        return 0
    # the GPU step: a process of its own under its own time limit
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--records", str(a.records), "--rounds",
                        str(a.rounds)], stdout=subprocess.PIPE, text=True, timeout=a.timeout)   # (its progress: stderr)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:])
        return p.returncode or 1
    line = p.stdout.strip().splitlines()[-1]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(json.loads(line), indent=1) + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
