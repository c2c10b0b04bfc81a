#!/usr/bin/env python3
"""The FASTQ ingest with qualities (crispresso_amd/ingest.py, fastq_parse.hip) and the front end
on files, against the interpreter's reader the front end started from, in one process:

    read_fastq_pack      flash.read_fastq + flash._pack of the bases and the qualities, per mate
    parse_fastq_bytes    the text in memory to resident records: upload / kernels (events), the
                         call's wall time, and the fetch of every array apart
    read_fastq_records   the .gz file to resident records, with the inflate's share
    prepare_fastq        (reader + upload) against prepare_fastq_device (ingest + hand-off),
                         alternated, on the plain files and on the .gz files

Input: bench_front.py's 1M synthetic 2 x 150 bp pairs (same generator and seed), written as FASTQ
text (names "@M7:<8 digits>/1") in memory, as plain files and as .gz files (level 1) in a
temporary directory.  Before timing, the two readers' records and the two paths' batches and names
are compared for equality.  Warm-up first; host clock around work that ends in a synchronising
copy; kernels by events.  Prints one JSON line."""
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("FRONT_BENCH_PAIRS", os.environ.get("INGEST_BENCH_PAIRS", "1000000"))
import bench_front as bf  # noqa: E402  (the generator: builds the pairs at import)
from crispresso_amd import flash, frontend, ingest  # noqa: E402
from crispresso_amd.aligner import GpuAligner  # noqa: E402

N, L = bf.N, bf.L
ROUNDS = int(os.environ.get("INGEST_BENCH_ROUNDS", "5"))
clock = time.perf_counter


def say(msg):
    print(f"[bench_ingest] {msg}", file=sys.stderr, flush=True)


def fastq_text(seq, qual, mate):
    """The mate's FASTQ text as one uint8 array (fixed-width records)."""
    name = np.frombuffer(b"".join(b"@M7:%08d/%d\n" % (k, mate) for k in range(N)), np.uint8).reshape(N, -1)
    nl = np.full((N, 1), 10, np.uint8)
    plus = np.tile(np.frombuffer(b"\n+\n", np.uint8), (N, 1))
    return np.concatenate([name, seq.reshape(N, L), plus, qual.reshape(N, L), nl], axis=1).ravel()


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "rounds": list(xs)}


def timed(fn):
    t = clock()
    out = fn()
    return clock() - t, out


def read_and_pack(path):
    names, seqs, quals = flash.read_fastq(path)
    return names, flash._pack(seqs), flash._pack(quals)


def same_batches(a, b):
    (pa, na), (pb, nb) = a, b
    return bool(na == nb and all(np.array_equal(getattr(pa, k), getattr(pb, k))
                                 for k in ("status", "src", "buf", "offsets", "lens")))


def main():
    texts = [fastq_text(bf.s1, bf.q1, 1), fastq_text(bf.s2, bf.q2, 2)]
    out = {"metric": "FASTQ files to records / to a prepared resident batch, s", "pairs": N, "read_len": L,
           "rounds": ROUNDS, "text_bytes_per_mate": int(texts[0].size)}
    with tempfile.TemporaryDirectory() as tmp, GpuAligner(0) as a_host, GpuAligner(0) as a_dev:
        plain = [os.path.join(tmp, f"r{m}.fastq") for m in (1, 2)]
        gz = [p + ".gz" for p in plain]
        for t, p, g in zip(texts, plain, gz):
            t.tofile(p)
            with open(g, "wb") as f:
                f.write(gzip.compress(t.tobytes(), compresslevel=1))
        out["gz_bytes_per_mate"] = os.path.getsize(gz[0])
        say("files written")
        for al in (a_host, a_dev):
            al.set_reference(bf.amplicon)
            al.set_phase_events(False)

        # equality first: the records of both readers, then both paths' batches and names
        names, (sb, so), (qb, _) = read_and_pack(plain[0])
        with ingest.read_fastq_records(gz[0]) as rec:
            out["same_records"] = bool(
                np.array_equal(rec.seq, sb) and np.array_equal(rec.qual, qb) and np.array_equal(rec.off, so)
                and rec.qual_off is None and rec.lists()[0] == names and rec.info["first_bad"] == -1)
        del names, sb, so, qb, rec
        kw = dict(trim=bf.prog, flash=bf.FLASH)
        out["same_batch_plain"] = same_batches(frontend.prepare_fastq_device(a_dev, *plain, **kw),
                                               frontend.prepare_fastq(a_host, *plain, **kw))
        out["same_batch_gz"] = same_batches(frontend.prepare_fastq_device(a_dev, *gz, **kw),
                                            frontend.prepare_fastq(a_host, *gz, **kw))
        say(f"equality: {out['same_records']} {out['same_batch_plain']} {out['same_batch_gz']}")

        # the readers, mate 1
        host, parse, fetch, gzrec, info_t, info_g = [], [], [], [], [], []
        for r in range(ROUNDS + 1):   # the first round is the warm-up
            th, _ = timed(lambda: read_and_pack(plain[0]))
            tp, rec = timed(lambda: ingest.parse_fastq_bytes(texts[0], fetch=False))
            tf, _ = timed(rec.fetch)
            it = dict(rec.info)
            rec.close()
            tg, rec = timed(lambda: ingest.read_fastq_records(gz[0], fetch=False))
            ig = dict(rec.info)
            rec.close()
            if r:
                host.append(th), parse.append(tp), fetch.append(tf), gzrec.append(tg)
                info_t.append(it), info_g.append(ig)
            say(f"readers round {r}: host {th:.3f} parse {tp:.3f} fetch {tf:.3f} gz {tg:.3f}")
        med = lambda ds, k: sorted(d[k] for d in ds)[len(ds) // 2]   # noqa: E731
        out["read_fastq_pack_s"] = spread(host)
        out["parse_fastq_bytes_s"] = spread(parse)
        out["parse_fastq_bytes_upload_ms"] = med(info_t, "upload_ms")
        out["parse_fastq_bytes_kernel_ms"] = med(info_t, "kernel_ms")
        out["fetch_all_s"] = spread(fetch)
        out["read_fastq_records_gz_s"] = spread(gzrec)
        out["read_fastq_records_gz_inflate_ms"] = med(info_g, "inflate_ms")
        out["read_fastq_records_gz_upload_ms"] = med(info_g, "upload_ms")
        out["read_fastq_records_gz_kernel_ms"] = med(info_g, "kernel_ms")

        # the two paths from files to the prepared batch, alternated
        for label, files in (("plain", plain), ("gz", gz)):
            td, th = [], []
            for r in range(ROUNDS + 1):
                a, _ = timed(lambda: frontend.prepare_fastq_device(a_dev, *files, **kw))
                b, _ = timed(lambda: frontend.prepare_fastq(a_host, *files, **kw))
                if r:
                    td.append(a), th.append(b)
                say(f"{label} round {r}: device {a:.3f} host {b:.3f}")
            out[f"prepare_fastq_device_{label}_s"] = spread(td)
            out[f"prepare_fastq_{label}_s"] = spread(th)
            out[f"speedup_median_{label}"] = spread(th)["median"] / spread(td)["median"]
            out[f"ranges_overlap_{label}"] = bool(max(td) >= min(th))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
