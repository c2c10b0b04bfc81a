#!/usr/bin/env python3
"""Region discovery on the GPU (CRISPRessoPooled's genome mode) against its restatement in Python
and against extract_regions on the same records.

Input (seeded): the 1M-record BAM of scripts/bench_regions.py (150 bp, three CIGAR ops each, 2 %
unmapped) with the positions rewritten: 95 % of the records sit within 4 bases of one of 100 sites
(with the CIGARs' deletions and insertions that is a few thousand distinct spans), 5 % anywhere
on their reference (a tail of mostly singleton regions).  Reports, in one process, as the minimum
of ``--steps`` after a warm-up call:

* ``discover_regions`` from the resident :class:`BamRecords` at ``min_reads`` 0 and 1000: the
  call (host wall, it ends synchronised), its kernels (HIP events) and its uploads (host wall);
  at the default chunk size (this BAM is two chunks) and again as one chunk, where the records are
  uploaded once;
* ``extract_regions`` on the same records with the 100 sites as its region table (the call
  that is handed the regions);
* the Python model (tests/genome_regions_model.py: span per record, a dict by key, the sort, the
  FASTQ text of the emitted regions) over the same records, once per ``min_reads``.

The GPU result is compared with the model before anything is reported: keys in order, counts,
n_aligned, and the FASTQ bytes of every emitted region.  The measuring process is a child under
a time limit of its own; one JSON document goes to ``--out`` (default
profiles/r01_discover/bench_discover.json) and to stdout."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
SITES, JITTER, TAIL = 100, 4, 0.05


def synthetic(n, seed=12):
    """(plain BAM stream, refs, the sites as regions, per-record fields) with the rewritten positions."""
    import numpy as np

    import bench_regions as br
    from tests import regions_cases as rc

    plain, refs, regions, f = br.synthetic(n, SITES)
    head = len(rc.bam_plain(refs, []))
    size = (len(plain) - head) // n
    recs = np.frombuffer(plain, np.uint8, n * size, head).reshape(n, size).copy()
    rng = np.random.Generator(np.random.PCG64(seed))
    site = (f["pos"].astype(np.int64) + br.SPACING // 2) // br.SPACING * br.SPACING
    pos = site - rng.integers(0, JITTER, n)
    tail = rng.random(n) < TAIL
    pos[tail] = rng.integers(1, refs[0][1] - 400, int(tail.sum()))
    recs[:, 8:12] = (pos - 1).astype("<i4").view(np.uint8).reshape(n, 4)
    f = dict(f, pos=pos)
    return plain[:head] + recs.tobytes(), refs, regions, f


def model(f, n, refs, min_reads):
    """The discovery in Python: (keys in order, counts, n_aligned, {key: FASTQ bytes} of the emitted)."""
    from tests import genome_regions_model as gm

    op = "MDI"
    by_key, aligned = {}, 0
    ref, pos, flag, a, b, c, kind = (f[k].tolist() for k in ("ref", "pos", "flag", "a", "b", "c", "kind"))
    br_read = len(f["seq"]) // n
    for i in range(n):
        aligned += (flag[i] & 0x904) == 0
        if flag[i] & 4:
            continue
        span = gm.span_ops(pos[i], "%dM%d%s%dM" % (a[i], b[i], op[kind[i]], c[i]))
        by_key.setdefault((ref[i],) + span, []).append(i)
    keys = sorted(by_key)
    fastq = {}
    for k in keys:
        if len(by_key[k]) >= min_reads:
            fastq[k] = b"".join(b"@r%07d\n%s\n+\n%s\n" % (i, f["seq"][i * br_read:(i + 1) * br_read],
                                                        f["qual"][i * br_read:(i + 1) * br_read]) for i in by_key[k])
    return keys, [len(by_key[k]) for k in keys], aligned, fastq


def measure(n, steps):
    import numpy as np

    from crispresso_amd import regions as rg

    clock = time.perf_counter
    plain, refs, sites, f = synthetic(n)
    bam = rg.read_bam(plain)
    assert len(bam) == n
    out = {"workload": f"{n} records of 150 bp (three CIGAR ops, 2 % unmapped): {100 - int(TAIL * 100)} % within {JITTER} bases "
                       f"of {SITES} sites, {int(TAIL * 100)} % anywhere on their reference",
           "steps": steps, "statistic": "minimum over the steps, after one warm-up call", "record_bytes": len(plain)}
    with rg.GpuRegionExtractor(0) as x:
        for min_reads in (0, 1000):
            res = rg.discover_regions(bam, min_reads, extractor=x)              # the warm-up call, checked below
            call_s, kernel_ms, upload_ms = [], [], []
            for _ in range(steps):
                t0 = clock()
                r = rg.discover_regions(bam, min_reads, extractor=x)
                call_s.append(clock() - t0)
                kernel_ms.append(r.kernel_ms)
                upload_ms.append(r.upload_ms)
            t0 = clock()
            keys, counts, aligned, fastq = model(f, n, refs, min_reads)
            model_s = clock() - t0
            got_keys = [tuple(int(v) for v in (t["ref_id"], t["bpstart"], t["bpend"])) for t in res.region_table]
            if got_keys != keys or res.n_records.tolist() != counts or res.n_aligned != aligned:
                raise SystemExit(f"min_reads {min_reads}: the GPU's regions differ from the model's")
            for g, k in enumerate(keys):
                if (res.fastq_bytes(g) if counts[g] >= min_reads else None) != fastq.get(k):
                    raise SystemExit(f"min_reads {min_reads}: the reads of region {k} differ from the model's")
            call = min(call_s)
            out["min_reads_%d" % min_reads] = {
                "regions": len(keys), "regions_emitted": res.n_emitted, "singleton_regions": counts.count(1),
                "records_kept": res.n_kept, "records_emitted": int(len(res.src)), "output_bytes": int(len(res.text)),
                "equal_to_model": True, "call_s": call, "records_per_s": n / call, "kernels_total_ms": min(kernel_ms),
                "upload_wall_ms": min(upload_ms), "kernel_share_of_call": min(kernel_ms) * 1e-3 / call,
                "upload_share_of_call": min(upload_ms) * 1e-3 / call, "python_model_s": model_s, "model_over_call": model_s / call}
        table = [(ref_id, s, e) for ref_id, s, e in sites]
        rg.extract_regions(bam, table, extractor=x)
        call_s, kernel_ms = [], []
        for _ in range(steps):
            t0 = clock()
            r = rg.extract_regions(bam, table, extractor=x)
            call_s.append(clock() - t0)
            kernel_ms.append(r.kernel_ms)
        out["extract_regions_same_records"] = {"regions": len(table), "hits": int(len(r.src)), "output_bytes": int(len(r.text)),
                                               "call_s": min(call_s), "kernels_total_ms": min(kernel_ms)}
    # the same calls with the BAM as one chunk: the records stay in HBM between the two passes
    os.environ["CRISPR_NWR_CHUNK"] = str(n)
    with rg.GpuRegionExtractor(0) as x:
        for min_reads in (0, 1000):
            first = rg.discover_regions(bam, min_reads, extractor=x)
            if not (np.array_equal(first.n_records, res.n_records) and np.array_equal(first.region_table, res.region_table)):
                raise SystemExit("one chunk: other regions than in two chunks")
            if min_reads == 1000 and not (np.array_equal(first.text, res.text) and np.array_equal(first.src, res.src)):
                raise SystemExit("one chunk: other reads than in two chunks")
            call_s, kernel_ms, upload_ms = [], [], []
            for _ in range(steps):
                t0 = clock()
                r = rg.discover_regions(bam, min_reads, extractor=x)
                call_s.append(clock() - t0)
                kernel_ms.append(r.kernel_ms)
                upload_ms.append(r.upload_ms)
            out["one_chunk_min_reads_%d" % min_reads] = {"call_s": min(call_s), "kernels_total_ms": min(kernel_ms),
                                                         "upload_wall_ms": min(upload_ms)}
    del os.environ["CRISPR_NWR_CHUNK"]
    out["not_measured"] = ["per-kernel times (no profiler run)", "the reference's own awk | sort | awk pipe on this input",
                           "read_bam (see profiles/r01_regions/bench_regions.json)"]
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--records", type=int, default=int(os.environ.get("DISCOVER_BENCH_RECORDS", "1000000")))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r01_discover", "bench_discover.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.records, a.steps)))
        return 0
    # the GPU step: a process of its own under its own time limit
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--records", str(a.records), "--steps",
                        str(a.steps)], capture_output=True, text=True, timeout=a.timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:] + p.stdout[-2000:])
        return p.returncode or 1
    line = p.stdout.strip().splitlines()[-1]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(json.loads(line), indent=1) + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
