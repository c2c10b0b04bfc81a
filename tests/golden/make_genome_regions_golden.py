"""Writes tests/golden/genome_regions.json.gz: per case the SAM lines and every file (name and
text) that the reference's genome-mode demultiplex makes of them.

    python tests/golden/make_genome_regions_golden.py <path to CRISPResso/CRISPRessoPooledCORE.py>

The two shell strings of the reference (``s1`` and ``s2``, CRISPRessoPooledCORE.py:1045-1075) are
taken out of that file as text and evaluated here, at generation time only; none of their text
is kept.  ``samtools view -F 4 <bam>`` at the head of the pipe is replaced by ``cat`` of the case's
SAM lines with ``flag & 4 == 0`` (all lines are recorded), and the pipe runs with the local
``awk`` and ``sort`` under ``LC_ALL=C``.  The golden in the tree was made with mawk 1.3.4 and GNU
coreutils' sort.  Mapped records without reference (``*``) and records without sequence are left
out: there discover_regions differs from the reference on purpose.  The tests that read the file
are tests/test_genome_regions_model.py and tests/test_gpu_genome_regions.py.
"""
import glob
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def seq_of(n, salt):
    return "".join("ACGT"[(i * 7 + salt + i // 5) % 4] for i in range(n))


def qual_of(n, salt):
    return "".join(chr(33 + (i * 11 + salt) % 42) for i in range(n))


def line(name, flag, ref, pos, cigar, n=None, seq=None, qual=None):
    if n is None and seq is None:
        import re

        n = sum(int(k) for k, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MIS=X") or 8
    seq = seq if seq is not None else seq_of(n, len(name))
    qual = qual if qual is not None else qual_of(len(seq), pos)
    return "\t".join(map(str, (name, flag, ref, pos, 30, cigar, "*", 0, 0, seq, qual)))


CIGARS = ["50M", "3S47M", "47M3S", "2H3S40M2I5M3D2M4S1H", "2I3S10M", "3S3S10M", "10M2S3M", "40M10N10M", "40M10P10M",
          "5=3X2M", "10M5=", "3S5=2M", "5=3S", "*", "15=", "12X3M2=4M", "2S3M1I2=1X1D2M1N3M", "4M2P4M", "1M", "3I4M",
          "5H10M", "10M5H", "2=2X2=3S4M", "0M5S10M"]


def cases():
    out = {}
    # every CIGAR at its own position, both strands; 5S10M at position 2 reaches below zero
    rows = [line("c%02d" % k, 16 if k % 3 == 0 else 0, "chr1", 100 + 1000 * k, c) for k, c in enumerate(CIGARS)]
    rows.append(line("low", 0, "chr1", 2, "5S10M"))
    rows.append(line("unmapped", 4, "chr1", 100, "50M"))
    out["cigars"] = rows
    # one file's order: strands, names that differ in their last byte, a name that another
    # begins with, equal names with different sequences and qualities, flags whose bit 16 is
    # set among others
    rows = []
    names = ["r10", "r1", "r1a", "r1b", "R1", "r2", "r1.x", "r1-x", "r1_x", "q9", "r1", "r1", "r1", "zz", "a", "r1A"]
    flags = [0, 16, 0, 16, 0, 83, 99, 16, 0, 147, 0, 0, 16, 1024, 2048 | 16, 0]
    for k, (nm, fl) in enumerate(zip(names, flags)):
        seq = seq_of(20, k % 5)
        rows.append(line(nm, fl, "chr2", 500, "20M", seq=seq, qual=qual_of(20, 0 if k % 2 else 3)))
    rows.append(line("r1", 0, "chr2", 500, "20M", seq=seq_of(20, 0), qual="I" * 20))
    rows.append(line("r1", 0, "chr2", 500, "20M", seq=seq_of(20, 0), qual="!" * 20))
    out["order"] = rows
    # references chr1 / chr10 / chr2 (the BAM's order: first appearance), the same span on two
    # references, equal starts with different ends (1005 before 101 as text), equal ends with
    # different starts, starts that sort differently as text and as numbers
    rows = []
    for k, (ref, pos, cigar) in enumerate([
            ("chr1", 100, "1M"), ("chr10", 100, "1M"), ("chr2", 100, "1M"), ("chr1", 100, "905M"), ("chr1", 100, "20M"),
            ("chr10", 100, "20M"), ("chr1", 90, "30M"), ("chr1", 1000, "20M"), ("chr1", 99, "21M"), ("chr2", 9, "5M"),
            ("chr2", 10, "4M"), ("chr1", 100, "20M"), ("chr1", 100, "1M"), ("chr10", 100, "1M"), ("chr1", 3, "5S2M"),
            ("chr1", 5, "5S2M"), ("chr1", 4, "5S2M"), ("chr2", 100, "1M"), ("chr1", 100, "905M"), ("chr1", 90, "30M")]):
        rows.append(line("m%d" % k, 16 * (k % 2), ref, pos, cigar, n=12 if cigar == "905M" else None))
    out["references"] = rows
    return out


def shell_strings(path, sam, outdir):
    """The reference's pipe for this SAM file and output directory."""
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.strip() == "s1 = (")
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("cmd = s1 + s2"))
    ns = {"bam_filename_genome": sam, "log_filename": os.devnull}
    exec("if True:\n" + "\n".join(lines[start:end]) + "\n", ns)
    cmd = ns["s1"] + ns["s2"].replace("__OUTPUTPATH__", outdir + os.sep)
    return "cat %s |" % sam + cmd.split("|", 1)[1]


def main(path):
    golden = []
    for name, rows in cases().items():
        with tempfile.TemporaryDirectory() as tmp:
            sam, outdir = os.path.join(tmp, "in.sam"), os.path.join(tmp, "out")
            os.mkdir(outdir)
            with open(sam, "w") as f:
                f.write("".join(r + "\n" for r in rows if not int(r.split("\t")[1]) & 4))
            subprocess.run(shell_strings(path, sam, outdir), shell=True, check=True, env=dict(os.environ, LC_ALL="C"))
            files = {}
            for p in sorted(glob.glob(os.path.join(outdir, "*"))):
                text = gzip.open(p).read() if p.endswith(".gz") else open(p, "rb").read()
                key = os.path.basename(p)[:-3] if p.endswith(".gz") else os.path.basename(p)
                assert key not in files
                files[key] = text.decode("latin-1")
        golden.append({"name": name, "sam": rows, "files": files})
        print("%s: %d lines -> %d files" % (name, len(rows), len(files)))
    out = os.path.join(HERE, "genome_regions.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as f:
        f.write(json.dumps({"cases": golden}, sort_keys=True).encode())
    print(out)


if __name__ == "__main__":
    main(sys.argv[1])
