"""The synthetic WGS case of tests/test_gpu_regions_resident.py: two references, four regions of
120 to 200 bases, about 200 records each (the last region fewer than ``MIN_READS``), with exact
copies, substitutions, an insertion and a deletion near the cut, reads with ``N``, junk that fails
the 60 % filter, soft clips and ``I`` / ``D`` in the CIGAR so that the slice matters, and one row
whose guide occurs nowhere.  Also the model's reads per region and the check of the CPU oracles'
slots (``oracle_check``), which needs no GPU: the choice of inputs is held before any GPU call.
"""
import numpy as np

from crispresso_amd import synth
from tests import regions_cases as rc
from tests import regions_model as rm

MIN_READS = 10
SIZES = (120, 150, 180, 200)
N_RECORDS = (200, 190, 210, 6)


def revcomp(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def genome():
    """(FASTA contigs {name: bases}, amplicons, region rows of the reference's seven columns)."""
    amps = [synth.random_amplicon(n, 40 + g) for g, n in enumerate(SIZES)]
    pad = [synth.random_amplicon(60, 90 + k) for k in range(6)]
    contigs = {"chrA": pad[0] + amps[0] + pad[1] + amps[1] + pad[2], "chrB": pad[3] + amps[2] + pad[4] + amps[3] + pad[5]}
    rows = []
    for g, a in enumerate(amps):
        chrom = "chrA" if g < 2 else "chrB"
        s = contigs[chrom].index(a) + 1
        rows.append({"chr_id": chrom, "bpstart": s, "bpend": s + len(a), "Name": "region %d" % g, "sgRNA": "",
                     "Expected_HDR": "", "Coding_sequence": ""})
    mid = SIZES[0] // 2
    rows[0]["sgRNA"] = revcomp(amps[0][mid - 10:mid + 10])        # found as its reverse complement only
    rows[1]["sgRNA"] = "ACGTTGCAACGTTGCAACGT"                      # occurs nowhere: blanked
    rows[2]["Coding_sequence"] = amps[2][40:130]
    assert rows[1]["sgRNA"] not in contigs["chrA"] and revcomp(rows[1]["sgRNA"]) not in contigs["chrA"]
    return contigs, amps, rows


def records():
    """(refs, records) of the BAM: record k of region g is one of eight kinds, in turn."""
    contigs, amps, rows = genome()
    refs = [("chrA", len(contigs["chrA"])), ("chrB", len(contigs["chrB"]))]
    rng = np.random.Generator(np.random.PCG64(7))
    out = []
    for g, (a, row) in enumerate(zip(amps, rows)):
        chrom, s = contigs[row["chr_id"]], row["bpstart"]
        ref_id = 0 if row["chr_id"] == "chrA" else 1
        cut = len(a) // 2 - (8 if g == 0 else 0)      # region 0's guide lies reversed: its cut is offset_rc from its start
        for k in range(N_RECORDS[g]):
            lead, tail = 3 + k % 9, 2 + k % 6
            lo = s - 1 - lead
            body = chrom[lo:s - 1 + len(a) + tail]
            kind = k % 8
            seq, cigar = body, "%dM" % len(body)
            if kind == 1:        # two substitutions away from the cut
                p, q = lead + 20 + k % 10, lead + len(a) - 25
                seq = body[:p] + "ACGT"[("ACGT".index(body[p]) + 1) % 4] + body[p + 1:q] + "ACGT"[("ACGT".index(body[q]) + 2) % 4] \
                    + body[q + 1:]
            elif kind == 2:      # a 2-base insertion at the cut
                at = lead + cut + 1
                seq, cigar = body[:at] + "GA" + body[at:], "%dM2I%dM" % (at, len(body) - at)
            elif kind == 3:      # a deletion of 3 to 6 bases over the cut
                d = 3 + k % 4
                at = lead + cut - 2
                seq, cigar = body[:at] + body[at + d:], "%dM%dD%dM" % (at, d, len(body) - at - d)
            elif kind == 4:      # an N in an exact copy
                p = lead + 30 + k % 40
                seq = body[:p] + "N" + body[p + 1:]
            elif kind == 5:      # junk of the same length, mapped as if it matched
                seq = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, len(body)))
            elif kind == 6:      # a soft clip in front
                seq, cigar = "ACG" + body, "3S%dM" % len(body)
            elif kind == 7:      # substitutions on both sides of the cut
                p = lead + cut
                seq = body[:p] + "".join("ACGT"[("ACGT".index(c) + 3) % 4] for c in body[p:p + 2]) + body[p + 2:]
            out.append(rc.rec("r%d_%d" % (g, k), ref_id, lo + 1, cigar, seq=seq))
    out.append(rc.rec("unmapped", 0, rows[0]["bpstart"], "100M", flag=4))
    return refs, out


def model_reads():
    """The reads of every region by tests/regions_model.py, as bytes."""
    _, _, rows = genome()
    refs, recs = records()
    ref_id = {"chrA": 0, "chrB": 1}
    want = rm.extract(recs, [(ref_id[r["chr_id"]], r["bpstart"], r["bpend"]) for r in rows])
    return [[h[3] for h in hits] for hits in want["hits"]]


def write_inputs(tmp_path):
    """(bam path, region file path, FASTA path) under tmp_path."""
    contigs, _, rows = genome()
    refs, recs = records()
    bam = tmp_path / "wgs.bam"
    bam.write_bytes(rc.bgzf(rc.bam_plain(refs, recs), [30000]))
    fasta = tmp_path / "genome.fa"
    fasta.write_text("".join(">%s\n%s\n" % (name, "\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)))
                             for name, seq in contigs.items()))
    table = tmp_path / "regions.txt"
    table.write_text("".join("\t".join(str(r[c]) for c in ("chr_id", "bpstart", "bpend", "Name", "sgRNA", "Expected_HDR",
                                                            "Coding_sequence")).rstrip("\t") + "\n" for r in rows))
    return str(bam), str(table), str(fasta)


def oracle_check(rows, oracle_slots):
    """The choice of inputs, on the oracles' result: every analysed region has a filtered read,
    an UNMODIFIED one and an NHEJ one, and no kept read that is not an alignment."""
    reads = model_reads()
    slots = {}
    for g, row in enumerate(rows):
        if len(reads[g]) < MIN_READS:
            continue
        s = slots[g] = oracle_slots(row, reads[g])
        assert s[0] == len(reads[g]) and s[0] - s[1] >= 1 and s[2] >= 1 and s[3] >= 1 and s[15] == 0, (g, s)
    assert sorted(slots) == [0, 1, 2] and [len(r) for r in reads] == list(N_RECORDS)
    return slots
