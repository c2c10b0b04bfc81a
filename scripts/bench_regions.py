#!/usr/bin/env python3
"""BAM records to per-region reads on the GPU against the per-read Python loop it replaces.

Input (seeded): a coordinate-sorted BAM of 1M records of 150 bp over 100 regions of 100 bp on two
references; every record overlaps one region, 10 % carry a deletion and 10 % an insertion (three
CIGAR ops each), 2 % are unmapped.  Reports, in one process, as the minimum of ``--steps`` after
a warm-up:

* ``read_bam`` of the BGZF bytes (inflate, index, validation; host only);
* the ``extract_regions`` call from the resident :class:`BamRecords` (wall), its kernels (HIP
  events) and its uploads (host wall), and the share of the call each takes;
* the reference's per-read procedure restated here (a per-base position list, ``in``, ``index``,
  the two slices and the FASTQ record; per region only the records that overlap it, which is
  what ``samtools view chr:start-end`` hands the reference) over the same records, once -- what a
  user of the reference runs today after samtools has done its part -- and the ratio of the two.

The results of both paths are compared before anything is reported.  The measuring process is a
child under a time limit of its own; one JSON document goes to ``--out`` (default
profiles/r01_regions/bench_regions.json) and to stdout."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READ, WIDTH, SPACING = 150, 100, 10000


def synthetic(n, n_regions, seed=11):
    """(plain BAM stream, refs, regions, per-record fields for the loop), coordinate-sorted."""
    import numpy as np

    from tests import regions_cases as rc

    rng = np.random.Generator(np.random.PCG64(seed))
    per_ref = (n_regions + 1) // 2
    refs = [("chrA", SPACING * (per_ref + 2)), ("chrB", SPACING * (per_ref + 2))]
    regions = [(g % 2, SPACING * (g // 2 + 1), SPACING * (g // 2 + 1) + WIDTH) for g in range(n_regions)]
    g = rng.integers(0, n_regions, n)
    ref = (g % 2).astype(np.int32)
    pos = (SPACING * (g // 2 + 1) - rng.integers(0, READ - WIDTH, n)).astype(np.int32)       # 1-based
    order = np.lexsort((pos, ref))
    ref, pos = ref[order], pos[order]
    kind = rng.choice(3, n, p=[0.8, 0.1, 0.1])             # 0: M M M, 1: M D M, 2: M I M
    a = rng.integers(20, 100, n)
    b = rng.integers(1, 6, n)
    mid_op = np.array([0, 2, 1])[kind]
    c = np.where(kind == 1, READ - a, READ - a - b)
    flag = np.where(rng.random(n) < 0.02, 4, np.where(rng.random(n) < 0.5, 16, 0)).astype(np.uint16)
    nib = rng.choice(np.array([1, 2, 4, 8, 15], np.uint8), (n, READ), p=[0.2475, 0.2475, 0.2475, 0.2475, 0.01])
    qual = rng.integers(2, 41, (n, READ)).astype(np.uint8)
    name = np.frombuffer(b"".join(b"r%07d\0" % i for i in range(n)), np.uint8).reshape(n, 9)
    dt = np.dtype([("bs", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("ln", "u1"), ("mq", "u1"), ("bin", "<u2"), ("nc", "<u2"),
                   ("flag", "<u2"), ("ls", "<i4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4"), ("name", "u1", 9),
                   ("cig", "<u4", 3), ("seq", "u1", READ // 2), ("qual", "u1", READ)])
    r = np.zeros(n, dt)
    r["bs"], r["ref"], r["pos"], r["ln"], r["mq"], r["nc"], r["flag"], r["ls"] = dt.itemsize - 4, ref, pos - 1, 9, 30, 3, flag, READ
    r["bin"] = 4681 + ((pos - 1) >> 14)
    r["nref"], r["npos"], r["name"] = -1, -1, name
    r["cig"] = np.stack([a << 4, (b << 4) | mid_op, c << 4], 1)
    r["seq"] = (nib[:, 0::2] << 4) | nib[:, 1::2]
    r["qual"] = qual
    plain = rc.bam_plain(refs, []) + r.tobytes()
    letters = np.frombuffer(rc.NIBBLES.encode(), np.uint8)[nib]
    fields = {"ref": ref, "pos": pos, "flag": flag, "a": a, "b": b, "c": c, "kind": kind,
              "seq": letters.tobytes(), "qual": (qual + 33).tobytes()}
    return plain, refs, regions, fields


def reference_loop(fields, regions, selected):
    """The reference's loop per region over the records samtools would hand it; returns the
    FASTQ bytes of every region."""
    op = "MDI"
    seqs, quals, pos, a, b, c, kind = (fields[k] for k in ("seq", "qual", "pos", "a", "b", "c", "kind"))
    out = []
    for (ref_id, bpstart, bpend), sel in zip(regions, selected):
        parts, n_reads = [], 0
        for i in sel:
            cigar = "%dM%d%s%dM" % (a[i], b[i], op[kind[i]], c[i])
            seq, qual, name = seqs[i * READ:(i + 1) * READ], quals[i * READ:(i + 1) * READ], b"r%07d" % i
            positions, p = [], pos[i]
            num = 0
            for ch in cigar:                      # (the reference: a regular expression, then this walk)
                if ch.isdigit():
                    num = num * 10 + int(ch)
                    continue
                if ch == "S" or ch == "I":
                    positions.extend([None] * num)
                elif ch == "M":
                    positions.extend(range(p, p + num))
                    p += num
                elif ch == "D" or ch == "N":
                    p += num
                num = 0
            if bpstart in positions and bpend in positions:
                st = positions.index(bpstart)
                en = len(positions) - positions[::-1].index(bpend) - 1
                n_reads += 1
                parts.append(b"@%s_%d\n%s\n+\n%s\n" % (name, n_reads, seq[st:en], qual[st:en]))
        out.append(b"".join(parts))
    return out


def measure(n, n_regions, steps):
    import numpy as np

    from crispresso_amd import regions as rg
    from tests import regions_cases as rc

    clock = time.perf_counter
    plain, refs, regs, fields = synthetic(n, n_regions)
    z = rc.bgzf(plain)
    read_s = []
    for _ in range(steps + 1):
        t0 = clock()
        bam = rg.read_bam(z)
        read_s.append(clock() - t0)
    assert len(bam) == n
    out = {"workload": f"{n} records of {READ} bp, coordinate-sorted, {n_regions} regions of {WIDTH} bp on 2 references; "
                       "10 % with a deletion, 10 % with an insertion, 2 % unmapped",
           "steps": steps, "statistic": "minimum over the steps", "bam_bytes": len(z), "record_bytes": len(plain),
           "read_bam_s": min(read_s[1:]), "read_bam_GBps_uncompressed": len(plain) / min(read_s[1:]) / 1e9}
    with rg.GpuRegionExtractor(0) as x:
        res = rg.extract_regions(bam, regs, extractor=x)                  # the warm-up call, checked below
        call_s, kernel_ms, upload_ms = [], [], []
        for _ in range(steps):
            t0 = clock()
            r = rg.extract_regions(bam, regs, extractor=x)
            call_s.append(clock() - t0)
            kernel_ms.append(r.kernel_ms)
            upload_ms.append(r.upload_ms)
        t0 = clock()
        fq = [res.fastq_bytes(g) for g in range(len(regs))]
        fastq_s = clock() - t0
    # per region, the records that overlap it: samtools' part, not timed
    mapped = (fields["flag"] & 4) == 0
    selected = []
    for ref_id, s, e in regs:
        lo = np.searchsorted(fields["pos"][fields["ref"] == ref_id], s - READ - 8)
        base = int(np.searchsorted(fields["ref"], ref_id))
        idx = np.arange(base + lo, base + np.searchsorted(fields["pos"][fields["ref"] == ref_id], e + 1))
        selected.append([int(i) for i in idx[mapped[idx]]])
    small = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in fields.items()}
    t0 = clock()
    want = reference_loop(small, regs, selected)
    loop_s = clock() - t0
    if fq != want:
        bad = [g for g in range(len(regs)) if fq[g] != want[g]]
        raise SystemExit(f"the GPU result differs from the loop in regions {bad[:10]}")
    call = min(call_s)
    out.update({
        "hits": int(len(res.src)), "output_bytes": int(len(res.text)), "n_no_seq": res.n_no_seq, "equal_to_loop": True,
        "call_s": call, "records_per_s": n / call, "kernels_total_ms": min(kernel_ms), "upload_wall_ms": min(upload_ms),
        "kernel_share_of_call": min(kernel_ms) * 1e-3 / call, "upload_share_of_call": min(upload_ms) * 1e-3 / call,
        "fastq_text_on_host_s": fastq_s, "python_loop_s": loop_s, "loop_over_call": loop_s / call,
        "loop_over_call_and_read_bam": loop_s / (call + min(read_s[1:])),
    })
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--records", type=int, default=int(os.environ.get("REGIONS_BENCH_RECORDS", "1000000")))
    ap.add_argument("--regions", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r01_regions", "bench_regions.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.records, a.regions, a.steps)))
        return 0
    # the GPU step: a process of its own under its own time limit
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--records", str(a.records), "--regions",
                        str(a.regions), "--steps", str(a.steps)], capture_output=True, text=True, timeout=a.timeout)
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
