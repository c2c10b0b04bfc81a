"""Every launch geometry of the quantifier (nw_quant.hip: geometry(), the lane kernel's and
expand_rows' block sizes in nwq_run_device_ops) against the CPU oracle, 400 to 4,952 bp, on the
batches of tests/quant_geometry_cases.py.  Each case names the regime it is there for and
GpuQuantifier.last_plan() must report it; every class, count, vector entry, counter and histogram
entry is compared exactly with oracle/quant_oracle.py on the rows the host expands from the same
runs.  Then the limit (4,952 bp runs, 4,953 is refused and the context goes on), one context across
regimes against fresh ones, host rows through nwq_run, and summarize_pooled / summarize_regions
over amplicons and a region that take different regimes.

DESIGN.md 4d has the table of regimes.  A library whose row kernel dropped the slab offset of the
list path failed every case here in which quant_lanes is on (profiles/r01_quant_geometry/NOTE.md)."""
from __future__ import annotations

import os
import types

import numpy as np
import pytest

from crispresso_amd import _lib, quantify, synth
from crispresso_amd.aligner import GpuAligner
from crispresso_amd.devmem import DeviceBuffer
from oracle import quant_oracle as qo
from tests import quant_geometry_cases as qc
from tests.test_gpu_quant import PARAMS, args_for, globals_for, make_params

pytestmark = pytest.mark.gpu

SHAPES = {"full": qc.full, "short": qc.short}
MAX_LDS = 160 * 1024

# (row kernel's waves a block, its totals in HBM, quant_lanes' waves a block or 0, expand_rows' waves a block)
REGIME = {
    ("full", 400): (4, False, 8, 4),
    ("full", 520): (2, False, 8, 4),
    ("full", 580): (2, False, 4, 4),
    ("full", 640): (1, False, 4, 4),       # (between the issue's rows: one wave from 589, quant_lanes at 4 to 695)
    ("full", 730): (1, False, 2, 4),
    ("full", 1000): (1, False, 1, 4),
    ("full", 1393): (1, False, 1, 4),      # the last length with the totals in LDS: close to all 160 KB
    ("full", 1394): (2, True, 1, 4),       # the first with the totals in HBM; the row kernel over the list
    ("full", 1532): (2, True, 1, 4),
    ("full", 1533): (1, True, 1, 4),
    ("full", 1633): (1, True, 1, 4),       # the last length with quant_lanes on
    ("full", 1634): (1, True, 0, 4),       # every read through the rows, 64 reads a wave
    ("full", 2709): (1, True, 0, 2),
    ("full", 4952): (1, True, 0, 2),       # the last length the row kernel takes
    ("short", 1000): (1, False, 1, 4),
    ("short", 1572): (1, False, 1, 4),
    ("short", 1573): (2, True, 1, 4),
    ("short", 1755): (2, True, 1, 4),
    ("short", 1756): (2, True, 0, 4),
    ("short", 2083): (1, True, 0, 4),
    ("short", 3000): (1, True, 0, 4),
}
CASES = [("full", La) for La in qc.FULL] + [("short", La) for La in qc.SHORT]


@pytest.fixture(scope="module")
def gq():
    with quantify.GpuQuantifier(0) as q:
        yield q


@pytest.fixture(scope="module")
def gq_rows():
    """A quantifier that sends every read through the rows (CRISPR_NWQ_ROWS=1 at create)."""
    old = os.environ.get("CRISPR_NWQ_ROWS")
    os.environ["CRISPR_NWQ_ROWS"] = "1"
    try:
        q = quantify.GpuQuantifier(0)
    finally:
        if old is None:
            os.environ.pop("CRISPR_NWQ_ROWS", None)
        else:
            os.environ["CRISPR_NWQ_ROWS"] = old
    yield q
    q.close()


@pytest.fixture(scope="module")
def aligned():
    """get(shape, La, n) -> the case aligned on the resident ops path, with the rows the host expands
    from the same runs.  One aligner alive at a time (the cases come in order)."""
    held = {}

    def get(shape, La, n=0):
        key = (shape, La, n)
        if key not in held:
            for a in held.values():
                a.al.close()
            held.clear()
            case = SHAPES[shape](La, n)
            buf, off = case.packed()
            al = GpuAligner(0)
            al.set_reference(case.amp)
            al.set_output("ops")
            al.upload(buf, off)
            al.run_async()
            al.sync()
            dev = al.device_ops()
            rows = al.download_ops(case.n).expand(case.amp, buf, off)
            assert (rows.stats["aln_len"] > 0).all()
            held[key] = types.SimpleNamespace(
                al=al, dev=dev, case=case, fn=SHAPES[shape], La=La, n=n, stride=int(dev["max_cols"]),
                rows=qc.rows_of(rows.aln, rows.stats["aln_len"], rows.stats["n_ident"], La + 5, case.sr_fixed))
        return held[key]

    yield get
    for a in held.values():
        a.al.close()


def reference(a, pname):
    """(params, oracle results, the batch's figures): the conditions on the batch from the CPU
    oracles alone, then quant_oracle on the rows the host expanded -- the cached results when those
    rows are the CPU aligner's, byte for byte."""
    ora = qc.oracle_rows(a.fn, a.La, a.n)
    prm, ref = qc.oracle_reference(a.fn, a.La, pname, a.n)
    fig = qc.conditions(a.case, ora, {pname: ref})
    r = a.rows
    if not ((r.R, r.M, r.S) == (ora.R, ora.M, ora.S) and np.array_equal(r.score, ora.score)):
        prm, ref = qc.reference(a.case, r, pname)
    return prm, ref, fig


def pre_of(a, prm):
    r = a.rows
    return quantify.pre_flags(r.um, r.sd if prm.expected_hdr else None, r.sr if prm.expected_hdr else None,
                              prm.hdr_perfect_alignment_threshold)


def run_ops(q, a, prm):
    q.set_params(globals_for(prm), args_for(prm, prm.exon_positions is not None))
    n = a.case.n
    with DeviceBuffer.from_array(pre_of(a, prm)) as d_pre, DeviceBuffer(16 * n) as d_out:
        totals = q.run_device_ops(a.case.amp, a.dev, d_pre.ptr, n, d_out.ptr)
        reads = d_out.download(np.zeros((n, 4), np.int32))
    return totals, reads


def assert_equals_oracle(tot, reads, ref):
    assert np.array_equal(reads[:, 0].astype(np.int8), ref["cls"])
    for c, k in ((1, "n_mutated"), (2, "n_inserted"), (3, "n_deleted")):
        assert np.array_equal(reads[:, c], ref[k]), k
    for k in qo.VECTORS:
        assert np.array_equal(tot["vectors"][k], ref["vectors"][k]), k
    assert tot["counters"] == ref["counters"]
    assert tot["hist_inframe"] == ref["hist_inframe"]
    assert tot["hist_frameshift"] == ref["hist_frameshift"]


def assert_regime(plan, shape, La, lanes, n):
    waves, hbm, lane_waves, expand_waves = REGIME[(shape, La)]
    if not lanes:
        lane_waves = 0
    print(shape, La, "lanes" if lanes else "rows", plan)
    assert (plan["row_waves"], plan["row_totals_hbm"]) == (waves, hbm)
    assert plan["lane_waves"] == lane_waves and (plan["lane_lds"] > 0) == (lane_waves > 0)
    assert plan["expand_waves"] == expand_waves
    assert plan["row_list"] == (lane_waves > 0)
    assert 0 < plan["row_lds"] <= MAX_LDS and plan["lane_lds"] <= MAX_LDS
    assert 1 <= plan["row_grid"] <= max(1, -(-n // waves))
    # a one-wave block is chosen only when two waves no longer fit in half of LDS
    if not hbm and waves == 1:
        assert plan["row_lds"] > MAX_LDS // 4


def check_case(gq, gq_rows, a, shape, La, pname):
    prm, ref, fig = reference(a, pname)
    assert a.stride == (qc.full_stride(La) if shape == "full" else qc.short_stride(La))
    n = a.case.n
    for q, lanes in ((gq, True), (gq_rows, False)):
        totals, reads = run_ops(q, a, prm)
        assert_equals_oracle(q.unpack_totals(totals, a.stride), reads, ref)
        plan = q.last_plan()
        assert_regime(plan, shape, La, lanes, n)
        if plan["lane_waves"]:
            # what quant_lanes must leave to the rows under these parameters (an ignored kind of edit
            # is not listed, so it cannot overflow its list)
            kinds = [k for k, off in (("subs_over", prm.ignore_substitutions), ("dels_3", prm.ignore_deletions),
                                      ("ins_3", prm.ignore_insertions), ("dash", False)) if not off]
            planted = {i for k in kinds for i in fig["over"][k]}
            print("lane fallbacks", q.last_lane_fallbacks, "planted", len(planted), "of", n)
            assert len(planted) >= qc.KIND_MIN
            assert len(planted) <= q.last_lane_fallbacks < n / 2
        else:
            assert q.last_lane_fallbacks == -1
    return ref


# ---- (a) every regime ---------------------------------------------------------------------------

@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("shape,La", CASES, ids=["%s_%d" % c for c in CASES])
def test_every_regime_vs_oracle(gq, gq_rows, aligned, shape, La, pname):
    check_case(gq, gq_rows, aligned(shape, La), shape, La, pname)


def test_every_regime_of_the_table_is_named():
    """Each (row kernel, lane kernel, expand_rows) shape the selection has for a stride >= the
    amplicon length is some case's regime."""
    seen = set(REGIME.values())
    for want in [(4, False, 8, 4), (2, False, 8, 4), (2, False, 4, 4), (1, False, 4, 4), (1, False, 2, 4), (1, False, 1, 4),
                 (2, True, 1, 4), (1, True, 1, 4), (1, True, 0, 4), (1, True, 0, 2), (2, True, 0, 4)]:
        assert want in seen, want
    assert all(c in REGIME for c in CASES)


# ---- (b) the limit ------------------------------------------------------------------------------

def test_the_longest_amplicon_and_the_refusal_after_it(gq, gq_rows, aligned):
    """4,952 bp is the last length a one-wave block fits in LDS beside the prefix tables; one base
    more is refused, and the context then runs the 400 bp case as before."""
    for pname in ("coding_guide", "coding_nowin_hdr"):
        check_case(gq, gq_rows, aligned("full", 4952, 32), "full", 4952, pname)
    a = aligned("full", 4953, 32)
    prm = make_params(a.case.amp, PARAMS["coding_guide"])
    for q in (gq, gq_rows):
        refused = False
        try:
            run_ops(q, a, prm)
        except quantify.QuantificationError as e:
            refused = True
            assert "(%d)" % _lib.NW_E_UNSUPPORTED in str(e) and "exceeds LDS" in str(e)
        assert refused, "4,953 bp was not refused"
        assert q.last_plan()["row_waves"] == 0
    check_case(gq, gq_rows, aligned("full", 400), "full", 400, "coding_guide")


# ---- (c) one context across regimes -------------------------------------------------------------

def test_one_context_across_regimes(aligned):
    """1394, 400, 2709, 730, 1533 and 400 again on one quantifier: each bit for bit what a fresh
    context gives (d_partial's growth and reuse, the amplicon tables' key, the pinned totals
    buffer, the occupancy cache)."""
    pname = "coding_nowin_hdr"
    with quantify.GpuQuantifier(0) as shared:
        for La in (1394, 400, 2709, 730, 1533, 400):
            a = aligned("full", La)
            prm, ref, _ = reference(a, pname)
            totals, reads = run_ops(shared, a, prm)
            plan = shared.last_plan()
            with quantify.GpuQuantifier(0) as fresh:
                totals1, reads1 = run_ops(fresh, a, prm)
                assert fresh.last_plan() == plan
            assert np.array_equal(totals, totals1) and np.array_equal(reads, reads1), La
            assert_equals_oracle(shared.unpack_totals(totals, a.stride), reads, ref)
            assert_regime(plan, "full", La, True, a.case.n)


# ---- (d) host rows through nwq_run --------------------------------------------------------------

@pytest.mark.parametrize("pname", ["coding_guide", "guide_w30_hide"])
@pytest.mark.parametrize("shape,La,waves", [("full", 2100, 2), ("short", 3000, 1)])
def test_host_rows_long(gq, shape, La, waves, pname):
    """quant_kernel_long over reads [0, n) with host-packed strides: the oracle's alignments, no
    aligner.  The host's stride is the longest alignment, about half the aligner's at 2,100 bp,
    so two waves fit there beside the prefix tables."""
    fn = SHAPES[shape]
    case, rows = fn(La), qc.oracle_rows(fn, La)
    prm, ref = qc.oracle_reference(fn, La, pname)
    qc.conditions(case, rows, {pname: ref})
    gq.set_params(globals_for(prm), args_for(prm, prm.exon_positions is not None))
    aln, lens = quantify.pack_rows(rows.R, rows.M, rows.S)
    pre = quantify.pre_flags(rows.um, None, None, prm.hdr_perfect_alignment_threshold)
    reads, totals = gq.run(aln, lens, pre)
    got = np.stack([reads["cls"], reads["n_mutated"], reads["n_inserted"], reads["n_deleted"]], axis=1)
    assert_equals_oracle(gq.unpack_totals(totals, aln.shape[2]), got, ref)
    plan = gq.last_plan()
    print(shape, La, plan)
    assert plan["row_totals_hbm"] and plan["row_waves"] == waves and not plan["row_list"]
    assert plan["lane_waves"] == 0 and plan["expand_waves"] == 0


# ---- (e) the summary calls across regimes -------------------------------------------------------

PANEL = (400, 730, 1450, 1700)
REGION, REGION_READ, REGION_SCORE = 1800, 150, 5.0


def panel():
    """(rows, reads) of a pooled panel over four regimes, 120 reads an amplicon, interleaved: the
    parity mix, and four reads an amplicon with more edits than a lane holds, so that the row
    kernel's list is not empty where quant_lanes is on, and four exact copies.  An sgRNA at the mix's
    indels on the 730 and 1,700 bp rows, a coding
    sequence over the mix's indels on the 1,450 bp row."""
    rng = np.random.Generator(np.random.PCG64(17))
    amps = [synth.random_amplicon(La, 3000 + La) for La in PANEL]
    groups = []
    for g, amp in enumerate(amps):
        buf, off = synth.reads_from(amp, 112, 500 + g, synth.PARITY_MIX)
        groups.append([r.encode() for r in synth.unpack(buf, off)] + [amp.encode()] * 4 +
                      [qc.kind_read(amp, 0, {"subs": 12, "dels": 3, "ins": 3}, rng).encode() for _ in range(4)])
    reads = [groups[j % 4][j // 4] for j in range(4 * 120)]
    rows = [{"Name": "AMP_%d" % La, "Amplicon_Sequence": a, "sgRNA": "", "Expected_HDR": "", "Coding_sequence": ""}
            for La, a in zip(PANEL, amps)]
    for g in (1, 3):             # (without a guide the window is the amplicon: only the exact copies are UNMODIFIED)
        mid = PANEL[g] // 2
        rows[g]["sgRNA"] = amps[g][mid - 10:mid + 10]
    rows[2]["Coding_sequence"] = amps[2][600:850]
    return rows, reads


def bytes_of(packed):
    buf, off = packed
    return [buf[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(off) - 1)]


def test_summarize_pooled_across_regimes(gpu_aligner_factory):
    """The 16 slots and the GroupReport integers of one panel whose amplicons take the row kernel
    with 4 waves and with 1 (totals in LDS), with the totals in HBM over quant_lanes' list, and
    with the totals in HBM over every read -- against the host path and the oracles."""
    from crispresso_amd import demux
    from crispresso_amd.pooled import align_pooled
    from tests.alleles_cases import pack
    from tests.test_gpu_reports import check_report
    from tests.test_gpu_summary import OPTS, SCORE, host_slots, oracle_slots

    rows, reads = panel()
    amps = [r["Amplicon_Sequence"] for r in rows]
    al = gpu_aligner_factory()
    got, plans = {}, {}
    with demux.GpuDemultiplexer(0) as d, quantify.GpuQuantifier(0) as q, quantify.GpuQuantifier(0) as gq:
        res = demux.demultiplex(amps, pack(reads), demultiplexer=d)
        counts = res.counts.tolist()
        assert sum(counts) >= 4 * 115 and min(counts) >= 115
        groups = res.reads_per_amplicon()
        batches = align_pooled(amps, groups, al)

        def on_report(g, rep):
            got[g] = rep
            plans[g] = q.last_plan()

        ps = demux.summarize_pooled(rows, pack(reads), al, min_reads=5, min_identity_score=SCORE, demultiplexer=d,
                                    quantifier=q, reports=on_report, **OPTS)
        plain = demux.summarize_pooled(rows, pack(reads), al, min_reads=5, min_identity_score=SCORE, demultiplexer=d,
                                       quantifier=q, **OPTS)
        assert np.array_equal(ps.counts, plain.counts) and ps.skipped == plain.skipped == [] and sorted(got) == [0, 1, 2, 3]
        for g in range(4):
            print(PANEL[g], plans[g])
            slots = ps.counts[g].tolist()
            assert slots == host_slots(batches[g], rows[g], gq) == oracle_slots(rows[g], bytes_of(groups[g])), g
            assert slots[0] == counts[g] and slots[2] > 0 and slots[3] > 0
            ref, _ = check_report(got[g], rows[g], counts[g], batches[g], None, slots, gq)
            v = ref["vectors"]
            assert v["effect_vector_any"].sum() > 0
            if not rows[g]["sgRNA"]:
                assert v["effect_vector_deletion"].sum() > 0 and v["effect_vector_insertion"].sum() > 0
                assert v["effect_vector_mutation"].sum() > 100
        assert sum(got[2].totals["counters"].values()) > 0 and got[2].totals["hist_frameshift"] and got[1].cut_points
    # full-length reads: the stride is at least twice the amplicon
    assert [plans[g]["row_totals_hbm"] for g in range(4)] == [False, False, True, True]
    assert [plans[g]["lane_waves"] > 0 for g in range(4)] == [True, True, True, False]
    assert [plans[g]["row_list"] for g in range(4)] == [True, True, True, False]
    assert plans[0]["row_waves"] > 1 and plans[1]["row_waves"] == 1


def region_inputs(tmp_path):
    """One region of 1,800 bases inside a contig and 160 records of about 150 bases over it.  A
    record is a hit of a region only if it covers both of its ends (CRISPRessoWGSCORE.py's
    rule), so each record is two pieces, one at either end of the region, with a deletion or a
    skipped stretch (D / N) of about 1,650 bases between them: exact copies, two substitutions,
    a 2-base insertion, a deletion of 3 to 6 bases, an N, junk, a soft clip; every record starts
    before the region and ends after it (the slice cuts it)."""
    from tests import regions_cases as rc

    rng = np.random.Generator(np.random.PCG64(23))
    region = synth.random_amplicon(REGION, 77)
    contig = synth.random_amplicon(200, 78) + region + synth.random_amplicon(200, 79)
    s = 201                                                  # 1-based start of the region
    recs = []
    for k in range(160):
        lead, tail = 3 + k % 9, 2 + k % 6
        a_in = 40 + (k * 7) % 70                             # bases of the region's start; the rest from its end
        a, b = lead + a_in, REGION_READ - a_in + tail
        gap = REGION - REGION_READ
        p0 = s - 1 - lead                                    # 0-based position in the contig
        first, second = contig[p0:p0 + a], contig[p0 + a + gap:p0 + a + gap + b]
        assert len(second) == b and b >= 40
        skip = "%d%s" % (gap, "DN"[k % 2])
        kind, seq, cigar = k % 8, first + second, "%dM%s%dM" % (a, skip, b)
        if kind == 1:
            i, j = lead + 15, a + 20
            seq = seq[:i] + "ACGT"[("ACGT".index(seq[i]) + 1) % 4] + seq[i + 1:j] + "ACGT"[("ACGT".index(seq[j]) + 2) % 4] + \
                seq[j + 1:]
        elif kind == 2:
            i = lead + 20
            seq, cigar = seq[:i] + "GA" + seq[i:], "%dM2I%dM%s%dM" % (i, a - i, skip, b)
        elif kind == 3:
            i, dd = lead + 25, 3 + k % 4
            seq, cigar = seq[:i] + seq[i + dd:], "%dM%dD%dM%s%dM" % (i, dd, a - i - dd, skip, b)
        elif kind == 4:
            i = lead + 12
            seq = seq[:i] + "N" + seq[i + 1:]
        elif kind == 5 and k % 16 == 5:
            seq = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, len(seq)))
        elif kind == 6:
            seq, cigar = "ACG" + seq, "3S" + cigar
        recs.append(rc.rec("r%d" % k, 0, p0 + 1, cigar, seq=seq))
    bam = tmp_path / "one.bam"
    bam.write_bytes(rc.bgzf(rc.bam_plain([("chrL", len(contig))], recs), [20000]))
    fasta = tmp_path / "one.fa"
    fasta.write_text(">chrL\n" + "\n".join(contig[i:i + 70] for i in range(0, len(contig), 70)) + "\n")
    table = tmp_path / "one.txt"
    table.write_text("chrL\t%d\t%d\tlong region\t%s\t\t%s\n" % (s, s + REGION, region[50:70], region[30:130]))
    return str(bam), str(table), str(fasta), len(recs)


def test_summarize_regions_on_a_long_region(gpu_aligner_factory, tmp_path):
    """The WGS shape through the whole call: the region file, the FASTA and the BAM to the 16
    slots and the report, against the host path (the region's reads on the host, align_pooled,
    the printed identity, quant_oracle, run_summary).  A 150-base read prints about 8 % against
    1,800 bases, so the filter is at 5."""
    from crispresso_amd import regions
    from crispresso_amd.pooled import align_pooled
    from tests.test_gpu_reports import check_report
    from tests.test_gpu_summary import OPTS, host_slots, oracle_slots

    bam_path, table, fasta, n_records = region_inputs(tmp_path)
    rows = regions.wgs_rows(regions.read_wgs_region_file(table), fasta)
    assert len(rows) == 1 and len(rows[0]["Amplicon_Sequence"]) == REGION and rows[0]["sgRNA"] and rows[0]["Coding_sequence"]
    bam = regions.read_bam(bam_path)
    targets = [(r["chr_id"], r["bpstart"], r["bpend"], r["Name"]) for r in rows]
    plain = regions.extract_regions(bam, targets)
    host_reads = bytes_of(plain.reads(0))
    assert len(host_reads) == n_records and max(map(len, host_reads)) == REGION_READ + 2 and min(map(len, host_reads)) >= 144
    al = gpu_aligner_factory()
    batches = align_pooled([rows[0]["Amplicon_Sequence"]], [plain.reads(0)], al)
    got, plans = {}, {}
    with quantify.GpuQuantifier(0) as q, quantify.GpuQuantifier(0) as gq:
        def on_report(g, rep):
            got[g] = rep
            plans[g] = q.last_plan()

        with regions.extract_regions_resident(bam, targets) as res:
            rs = regions.summarize_regions(rows, res, al, min_reads=10, min_identity_score=REGION_SCORE, quantifier=q,
                                           reports=on_report, **OPTS)
            without = regions.summarize_regions(rows, res, al, min_reads=10, min_identity_score=REGION_SCORE,
                                                quantifier=q, **OPTS)
        assert np.array_equal(rs.counts, without.counts) and rs.skipped == [] and sorted(got) == [0]
        slots = rs.counts[0].tolist()
        print(REGION, plans[0], slots)
        assert slots == host_slots(batches[0], rows[0], gq, REGION_SCORE) == oracle_slots(rows[0], host_reads, REGION_SCORE)
        assert slots[0] == n_records and slots[0] >= slots[1] > 100 and slots[2] > 10 and slots[3] > 10
        ref, _ = check_report(got[0], rows[0], n_records, batches[0], None, slots, gq, REGION_SCORE)
    assert ref["vectors"]["effect_vector_deletion"].max() > 50           # the end deletions of a short read
    assert sum(ref["counters"].values()) > 0 and got[0].cut_points
    assert plans[0]["row_totals_hbm"] and plans[0]["lane_waves"] == 0 and not plans[0]["row_list"]
