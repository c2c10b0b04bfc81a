"""Plain-Python restatements of the Expected_HDR half of include/crispr_summary.h for
tests/test_hdr_summary_model.py and tests/test_gpu_hdr_summary.py: the printed identity in tenths
by integers, nws_printed and nws_flags_dual record by record, the reference's rule on printed
floats, the four-amplicon panel of the whole-call tests and its 16 slots from the CPU oracles
alone (needle, the printed identities, quant_oracle)."""
import numpy as np

from crispresso_amd import _lib, synth
from crispresso_amd.aligner import printed_percent
from oracle import quant_oracle as qo
from tests import pooled_summary_model as psm
from tests.alleles_cases import pack
from tests.helpers import oracle_batch

NO_TENTHS = 0xFFFF
MAX_COLS = 1 << 20
OPTS = dict(window_around_sgrna=1, cleavage_offset=-3, exclude_bp_from_left=15, exclude_bp_from_right=15)
SCORE, THRESHOLD = 60.0, 98.0


def tenths(n, L, tie_up):
    """printed_percent(n, L) * 10 by integers: the rule of the header."""
    n, L = int(n), int(L)
    if L == 0:
        return 0
    t, r = divmod(1000 * n, L)
    if 2 * r < L:
        return t
    if 2 * r > L:
        return t + 1
    return t + int(tie_up[t])


def record_tenths(L, n, tie_up):
    """(tenths, out of range) of one record, the EMPTY flag aside."""
    L, n = int(L), int(n)
    if not 0 <= L <= MAX_COLS or not 0 <= n <= L:
        return NO_TENTHS, True
    return tenths(n, L, tie_up), False


def printed(aln_len, n_ident, stat_flags, tie_up):
    """(uint16 tenths, n_out_of_range) of nws_printed."""
    out, bad = [], 0
    for L, n, f in zip(aln_len, n_ident, stat_flags):
        t, outside = record_tenths(L, n, tie_up)
        bad += outside
        out.append(NO_TENTHS if int(f) & _lib.NW_FLAG_EMPTY else t)
    return np.array(out, np.uint16), bad


def flags_dual(aln_len, n_ident, stat_flags, rep, tie_up, keep_tenths, hdr_tenths):
    """(pre, keep, n_out_of_range) of nws_flags_dual."""
    pre, keep, bad = [], [], 0
    for L, n, f, p in zip(aln_len, n_ident, stat_flags, rep):
        ref, outside = record_tenths(L, n, tie_up)
        p = int(p)
        has_rep = p <= 1000
        if outside or (not has_rep and p != NO_TENTHS):
            bad += 1
            pre.append(0)
            keep.append(0)
            continue
        empty = bool(int(f) & _lib.NW_FLAG_EMPTY)
        keep.append(int(not empty and (ref >= keep_tenths or (has_rep and p >= keep_tenths))))
        b = _lib.NWQ_PRE_UNMODIFIED if ref == 1000 else 0
        if has_rep and ref < p:
            b |= _lib.NWQ_PRE_HDR if p >= hdr_tenths else _lib.NWQ_PRE_MIXED
        pre.append(b)
    return np.array(pre, np.uint8), np.array(keep, np.uint8), bad


def reference_rule(score_ref, score_repaired, min_identity_score, threshold):
    """(kept, pre) as the reference computes them from the two printed floats
    (CRISPRessoCORE.py:1849-1856, 2014, 536-548 through quantify.pre_flags)."""
    from crispresso_amd import quantify

    sr, sp = np.asarray(score_ref, np.float64), np.asarray(score_repaired, np.float64)
    kept = (sr > min_identity_score) | (sp > min_identity_score)
    return kept, quantify.pre_flags(sr == 100, sr - sp, sp, threshold)


# ---- the four-amplicon panel --------------------------------------------------------------------

EDIT_AT = 70          # the first base of the edit: inside the first 115 bases, far from both ends


def _other(base):
    return "ACGT"[("ACGT".index(base) + 2) % 4]


def _substituted(seq, positions):
    s = list(seq)
    for p in positions:
        s[p] = _other(s[p])
    return "".join(s)


def panel():
    """(rows, reads as bytes, the amplicon each read was made from).  Four amplicons of 200
    random bases: 0 with a 10-base block replaced in Expected_HDR, 1 with 6 bases inserted
    (another length), 2 like 0 with an sgRNA over the edit, 3 without Expected_HDR.  Every second
    read is reverse-complemented."""
    amps = [synth.random_amplicon(200, 310 + g) for g in range(4)]
    rows, reads, origin = [], [], []
    for g, a in enumerate(amps):
        if g == 1:
            h = a[:EDIT_AT] + "".join(_other(c) for c in a[EDIT_AT - 6:EDIT_AT]) + a[EDIT_AT:]
        elif g < 3:
            h = a[:EDIT_AT] + "".join(_other(c) for c in a[EDIT_AT:EDIT_AT + 10]) + a[EDIT_AT + 10:]
        else:
            h = ""
        rows.append({"Name": "AMP_%d" % g, "Amplicon_Sequence": a, "sgRNA": a[EDIT_AT - 8:EDIT_AT + 12] if g == 2 else "",
                     "Expected_HDR": h, "Coding_sequence": ""})
        nhej = a[:100] + a[103:]
        if h:
            far = [20, 40, 130, 150, 170]                      # substitutions outside the edit
            mine = [a] * 8 + [h] * 6 + [_substituted(h, far[:4])] * 3 + [_substituted(h, far)] * 3 + [nhej] * 4 \
                + [a[:EDIT_AT] + a[EDIT_AT + 10:]] * 2 + [h[:121]] * 2 + [h[:115]] * 2
            if len(h) != len(a):
                mine += [h[:125]] * 2      # 121 of 206 columns print 58.7: the prefix that prints above 60 there
        else:
            mine = [a] * 12 + [nhej] * 6 + [_substituted(a, [30, 160])] * 6
        reads += mine
        origin += [g] * len(mine)
    reads = [r.encode() for r in reads]
    reads = [r.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1] if j % 2 else r for j, r in enumerate(reads)]
    return rows, reads, origin


# ---- two regions of a BAM, one with Expected_HDR -------------------------------------------------

REGION_SIZES = (160, 180)
REGION_RECORDS = (24, 20)
REGION_EDIT_AT = 60


def region_case():
    """(contigs, refs, records, region-file rows): built like tests/regions_summary_cases.py.
    Region 0 has an Expected_HDR with a 10-base block replaced; its records are, in turn, an exact
    copy, a copy of the Expected_HDR allele, that with 3 substitutions (prints 98.1: HDR) and with
    5 (96.9: MIXED), a 3-base deletion in the CIGAR, and junk both identities drop.  Region 1 has
    none: exact copies, substitutions, the deletion, junk."""
    from tests import regions_cases as rc

    amps = [synth.random_amplicon(n, 330 + g) for g, n in enumerate(REGION_SIZES)]
    pad = [synth.random_amplicon(50, 340 + k) for k in range(3)]
    contig = pad[0] + amps[0] + pad[1] + amps[1] + pad[2]
    rows = []
    for g, a in enumerate(amps):
        s = contig.index(a) + 1
        rows.append({"chr_id": "chrH", "bpstart": s, "bpend": s + len(a), "Name": "hdr region %d" % g, "sgRNA": "",
                     "Expected_HDR": "", "Coding_sequence": ""})
    e = REGION_EDIT_AT
    rows[0]["Expected_HDR"] = amps[0][:e] + "".join(_other(c) for c in amps[0][e:e + 10]) + amps[0][e + 10:]
    rng = np.random.Generator(np.random.PCG64(17))
    records = []
    for g, (a, row) in enumerate(zip(amps, rows)):
        s = row["bpstart"]
        for k in range(REGION_RECORDS[g]):
            lead, tail = 3 + k % 5, 2 + k % 4
            lo = s - 1 - lead
            body = contig[lo:s - 1 + len(a) + tail]
            seq, cigar = body, "%dM" % len(body)
            kind = k % 6 if g == 0 else (0, 4, 6, 5)[k % 4]
            if kind in (1, 2, 3):        # the Expected_HDR allele, mapped as if it matched
                p = lead + e
                seq = body[:p] + "".join(_other(c) for c in body[p:p + 10]) + body[p + 10:]
                seq = _substituted(seq, [lead + q for q in ([], [], [20, 100, 140], [20, 40, 100, 120, 140])[kind]])
            elif kind == 4:              # a deletion of 3 bases
                at = lead + len(a) // 2
                seq, cigar = body[:at] + body[at + 3:], "%dM3D%dM" % (at, len(body) - at - 3)
            elif kind == 5:              # junk of the same length
                seq = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, len(body)))
            elif kind == 6:              # two substitutions
                seq = _substituted(body, [lead + 25, lead + 130])
            records.append(rc.rec("h%d_%d" % (g, k), 0, lo + 1, cigar, seq=seq))
    return {"chrH": contig}, [("chrH", len(contig))], records, rows


def region_model_reads():
    """The reads of both regions by tests/regions_model.py."""
    from tests import regions_model as rm

    _, _, records, rows = region_case()
    want = rm.extract(records, [(0, r["bpstart"], r["bpend"]) for r in rows])
    return [[h[3] for h in hits] for hits in want["hits"]]


def write_region_inputs(tmp_path):
    """(bam path, region file path, FASTA path) under tmp_path."""
    from tests import regions_cases as rc

    contigs, refs, records, rows = region_case()
    bam = tmp_path / "hdr.bam"
    bam.write_bytes(rc.bgzf(rc.bam_plain(refs, records), [20000]))
    fasta = tmp_path / "genome.fa"
    fasta.write_text("".join(">%s\n%s\n" % (name, "\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)))
                             for name, seq in contigs.items()))
    table = tmp_path / "regions.txt"
    table.write_text("".join("\t".join(str(r[c]) for c in ("chr_id", "bpstart", "bpend", "Name", "sgRNA", "Expected_HDR",
                                                            "Coding_sequence")).rstrip("\t") + "\n" for r in rows))
    return str(bam), str(table), str(fasta)


def printed_pairs(amp, hdr, group_reads):
    """(batch against amp, score_ref, score_repaired) of the oriented reads by the CPU aligner
    oracle; NaN where there is no repaired score."""
    buf, off = pack(group_reads)
    ba = oracle_batch(amp, buf, off)
    sr = np.array([printed_percent(int(n), int(L)) for n, L in zip(ba.stats["n_ident"], ba.stats["aln_len"])])
    if not hdr:
        return ba, sr, np.full(len(sr), np.nan)
    bh = oracle_batch(hdr, buf, off)
    sp = np.array([printed_percent(int(n), int(L)) for n, L in zip(bh.stats["n_ident"], bh.stats["aln_len"])])
    return ba, sr, sp


def oracle_slots(row, group_reads, min_identity_score=SCORE, threshold=THRESHOLD):
    """The 16 slots of one amplicon from the CPU oracles alone: needle against the amplicon and
    the Expected_HDR amplicon, the filter and the flags on the printed floats, quant_oracle with
    expected_hdr, the slot model.  Also returns the two printed scores."""
    amp, hdr = row["Amplicon_Sequence"], row.get("Expected_HDR") or None
    ba, sr, sp = printed_pairs(amp, hdr, group_reads)
    empty = np.array([ba.empty(i) for i in range(len(ba))])
    with np.errstate(invalid="ignore"):
        kept = ~empty & ((sr > min_identity_score) | (sp > min_identity_score))
    sel = np.flatnonzero(kept)
    cuts = qo.cut_points(amp, row["sgRNA"] or None, OPTS["cleavage_offset"])
    exon, spl = qo.exon_splicing_positions(amp, row["Coding_sequence"] or None)
    prm = qo.QuantParams(len(amp), qo.include_idxs(len(amp), cuts, OPTS["window_around_sgrna"],
                                                   OPTS["exclude_bp_from_left"], OPTS["exclude_bp_from_right"]),
                         exon, spl, window_around_sgrna=OPTS["window_around_sgrna"], expected_hdr=bool(hdr),
                         hdr_perfect_alignment_threshold=threshold)
    um = sr[sel] == 100
    res = qo.process_rows([ba.ref_seq(i) for i in sel], [ba.align_str(i) for i in sel], [ba.align_seq(i) for i in sel],
                          um, (sr - sp)[sel] if hdr else None, sp[sel] if hdr else None, prm)
    got = psm.slots(res["cls"], res["n_mutated"], res["n_inserted"], res["n_deleted"],
                    um.astype(np.uint8) * _lib.NWQ_PRE_UNMODIFIED, np.ones(len(sel), np.uint8))
    return [len(group_reads)] + got[1:], sr, sp
