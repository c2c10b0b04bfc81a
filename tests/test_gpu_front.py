"""The read front end on the GPU (crispresso_amd/frontend.py, nwp_prepare, front_pack.hip)
against its CPU restatement (tests/front_model.py): status, batch text, offsets, lengths, the
2-bit stream and its exceptions byte for byte; the aligner, the quantification and the allele
grouping on the adopted batch against the same calls on an uploaded batch; the reference's pinned
runs from the raw pairs with no file between the stages; the refusals."""
import os

import numpy as np
import pytest

from crispresso_amd import _lib, alleles, frontend, quantify
from crispresso_amd.aligner import pack_2bit
from crispresso_amd.flash import FlashOptions
from crispresso_amd.trim import UnsupportedTrimStep
from tests import front_model as fm
from tests.test_e2e_pin import CASES, HERE, check_rows, expected, quant_args, summary_values
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu
FLASH = FlashOptions(min_overlap=4, max_overlap=100, allow_outies=True)


def prepare(al, pairs, single_end=False, **kw):
    kw.setdefault("flash", FLASH)
    return frontend.prepare_packed(al, *fm.packed_inputs(pairs, single_end), with_quals=True, with_packed=True, **kw)


def assert_equals_model(pb, e, what=""):
    assert np.array_equal(pb.status, e.status), (what, np.flatnonzero(pb.status != e.status)[:10])
    assert np.array_equal(pb.src, e.src), what
    assert np.array_equal(pb.offsets, e.offsets), what
    assert pb.offsets.dtype == np.int64 and pb.lens.dtype == np.uint16
    assert np.array_equal(pb.lens, e.lens), what
    assert np.array_equal(pb.buf, e.buf), (what, np.flatnonzero(pb.buf != e.buf)[:10])
    assert np.array_equal(pb.quals, e.qbuf), what
    nb = (int(e.offsets[-1]) + 3) // 4
    assert np.array_equal(pb.packed.packed[:nb], e.packed.packed[:nb]), \
        (what, np.flatnonzero(pb.packed.packed[:nb] != e.packed.packed[:nb])[:10])
    assert np.array_equal(pb.packed.exc_pos, e.packed.exc_pos), what
    assert np.array_equal(pb.packed.exc_byte, e.packed.exc_byte), what
    st = pb.stats
    assert st["combined"] == len(e.src) and st["pairs"] == len(e.status)
    for k, name in enumerate(("filtered", "trimmed", "not_combined", "innies", "outies")):
        assert st[name] == int(np.sum(e.status == k)), (what, name)


def run_ops(al, m):
    al.run_async()
    al.sync()
    return al.download_ops(m)


def assert_same_ops(a, b):
    assert np.array_equal(a.stats, b.stats)
    assert np.array_equal(a.ops_off, b.ops_off)
    assert np.array_equal(a.ops, b.ops)


def uploaded(factory, amp, e):
    """A second context holding the model's batch through the host path."""
    al = factory()
    al.set_reference(amp)
    al.upload_packed(pack_2bit(e.buf, e.offsets))
    return al


def simple_pairs(m, seed, extra=()):
    """m pairs that merge (60-99 bp fragments read whole from both ends) and `extra`."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for _ in range(m):
        f = fm._bases(rng, int(rng.integers(60, 100)))
        out.append((f, b"I" * len(f), fm.rc(f), b"H" * len(f)))
    return out + list(extra)


UNRELATED = (b"ACGTTGCAAC" * 5, b"I" * 50, b"GATTACAGGA" * 5, b"I" * 50)


# ---- the packer and the status against the model --------------------------------------------

def test_packer_against_model(gpu_aligner_factory):
    pairs, e = fm.packer_case()
    al = gpu_aligner_factory()
    al.set_reference("ACGT" * 50)
    pb = prepare(al, pairs, trim=fm.PACKER_TRIM, **fm.PACKER_FILTER)
    assert_equals_model(pb, e, "packer")
    assert {k: pb.stats[k] for k in e.trim} == e.trim
    assert pb.stats["trim_pairs"] == sum(e.trim.values())


# ---- edges, small batches -------------------------------------------------------------------

def test_no_survivor_keeps_the_previous_batch(gpu_aligner_factory):
    amp = fm._bases(np.random.Generator(np.random.PCG64(5)), 90).decode()
    al = gpu_aligner_factory()
    al.set_reference(amp)
    first = simple_pairs(40, 11)
    pb = prepare(al, first)
    before = run_ops(al, len(pb))
    off_before = al._off
    empty = prepare(al, [UNRELATED] * 3)
    assert len(empty) == 0 and empty.offsets.tolist() == [0] and len(empty.buf) == 0 and len(empty.src) == 0
    assert empty.status.tolist() == [fm.NOT_COMBINED] * 3
    assert al._off is off_before
    assert_same_ops(run_ops(al, len(pb)), before)


@pytest.mark.parametrize("m", [1, 256, 257, 1024, 1025])
def test_batch_sizes(gpu_aligner_factory, oracle, m):
    """One read; the classify kernel's offset-rebuild block (256 reads) and the length group
    (1024 reads) exactly full and one over."""
    pairs = simple_pairs(m, 100 + m, extra=[UNRELATED])
    pairs.insert(m // 2, UNRELATED)
    e = fm.expected(pairs)
    assert len(e.src) == m
    amp = pairs[0][0].decode()
    al = gpu_aligner_factory()
    al.set_reference(amp)
    pb = prepare(al, pairs)
    assert_equals_model(pb, e, f"m={m}")
    ob = run_ops(al, m)
    assert_same_ops(ob, run_ops(uploaded(gpu_aligner_factory, amp, e), m))
    if m <= 257:
        assert_same(oracle, amp, e.buf, e.offsets, ob.expand(amp, pb.buf, pb.offsets), f"m={m}")


def test_all_n_read_and_one_base_mates(gpu_aligner_factory):
    pairs = [(b"N" * 50, b"I" * 50, b"N" * 50, b"I" * 50)] + simple_pairs(3, 7)
    e = fm.expected(pairs)
    assert e.reads[0] == b"N" * 50
    al = gpu_aligner_factory()
    al.set_reference("ACGT" * 20)
    assert_equals_model(prepare(al, pairs), e, "all N")
    ob = run_ops(al, 4)
    assert_same_ops(ob, run_ops(uploaded(gpu_aligner_factory, "ACGT" * 20, e), 4))
    pairs = [(b"A", b"I", b"T", b"I"), (b"A", b"I", b"A", b"I"), (b"C", b"5", b"G", b"I")]
    e = fm.expected(pairs, min_overlap=1)
    assert e.reads == [b"A", b"C"]
    assert_equals_model(prepare(al, pairs, flash=FlashOptions(min_overlap=1, max_overlap=100)), e, "one base")


def test_empty_mates_with_the_filter_off(gpu_aligner_factory):
    pairs = [(b"", b"", b"", b""), (b"ACGT", b"IIII", b"", b"")] + simple_pairs(2, 9) + [(b"", b"", b"ACGT", b"IIII")]
    e = fm.expected(pairs)
    assert e.status.tolist() == [2, 2, 3, 3, 2]
    al = gpu_aligner_factory()
    al.set_reference("ACGT" * 20)
    assert_equals_model(prepare(al, pairs), e, "empty mates")
    with pytest.raises(ValueError):
        prepare(al, pairs, min_bp_quality=20)


@pytest.mark.parametrize("tail", [0, 1, 2, 3])
def test_last_read_ends_on_and_off_a_byte_boundary(gpu_aligner_factory, tail):
    pairs = simple_pairs(5, 21)
    total = sum(len(p[0]) for p in pairs)
    f = b"ACGTTGCATGCAGGCTTAAC" * 3 + b"ACG"[:(tail - total) % 4]
    pairs.append((f, b"I" * len(f), fm.rc(f), b"I" * len(f)))
    e = fm.expected(pairs)
    assert int(e.offsets[-1]) % 4 == tail and len(e.src) == 6
    al = gpu_aligner_factory()
    al.set_reference(f.decode())
    assert_equals_model(prepare(al, pairs), e, f"tail {tail}")
    assert_same_ops(run_ops(al, 6), run_ops(uploaded(gpu_aligner_factory, f.decode(), e), 6))


def test_smaller_batch_after_a_larger_one(gpu_aligner_factory):
    big, small = simple_pairs(1500, 31), simple_pairs(300, 32, extra=[UNRELATED])
    amp = small[0][0].decode()
    al = gpu_aligner_factory()
    al.set_reference(amp)
    prepare(al, big)
    run_ops(al, 1500)
    pb = prepare(al, small)
    assert_equals_model(pb, fm.expected(small), "second call")
    fresh = gpu_aligner_factory()
    fresh.set_reference(amp)
    pf = prepare(fresh, small)
    assert_same_ops(run_ops(al, len(pb)), run_ops(fresh, len(pf)))
    assert al.path_counts() == fresh.path_counts()


def test_single_end_against_model(gpu_aligner_factory, oracle):
    pairs, _ = fm.packer_case()
    reads = [(p[0], p[1], b"", b"") for p in pairs[:700]]
    reads[3] = (reads[3][0][:20] + b"acgtn" + reads[3][0][25:], reads[3][1], b"", b"")   # lower case
    reads[4] = (reads[4][0][:30] + b"RYK-" + reads[4][0][34:], reads[4][1], b"", b"")    # IUPAC codes, a dash
    steps = ["SLIDINGWINDOW:4:15", "LEADING:5", "MINLEN:40"]
    e = fm.expected(reads, single_end=True, trim=steps, **fm.PACKER_FILTER)
    assert e.status[3] == fm.COMBINED and e.status[4] == fm.COMBINED
    assert {ord("n"), ord("R"), ord("Y"), ord("K"), ord("-")} <= set(e.packed.exc_byte.tolist())
    assert ord("a") not in set(e.packed.exc_byte.tolist()) and ord("a") in set(e.buf.tolist())
    assert len(set(e.status.tolist())) == 3
    al = gpu_aligner_factory()
    amp = pairs[0][0].decode()
    al.set_reference(amp)
    pb = prepare(al, reads, single_end=True, trim=steps, **fm.PACKER_FILTER)
    assert_equals_model(pb, e, "single end")
    assert_same_ops(run_ops(al, len(pb)), run_ops(uploaded(gpu_aligner_factory, amp, e), len(pb)))
    # no trim, no filter: every read whole, an empty one among them
    plain = reads[:9] + [(b"", b"", b"", b"")] + reads[9:20]
    e = fm.expected(plain, single_end=True)
    assert len(e.src) == 21
    assert_equals_model(prepare(al, plain, single_end=True), e, "single end, plain")


# ---- alignment equality ---------------------------------------------------------------------

def test_alignment_on_the_adopted_batch(gpu_aligner_factory, oracle):
    from crispresso_amd.devmem import DeviceBuffer
    from crispresso_amd.needle import _printed_percents

    amp, pairs = fm.align_case()
    e = fm.expected(pairs)
    m = len(e.src)
    assert m >= 2900
    al = gpu_aligner_factory()
    al.set_reference(amp)
    pb = prepare(al, pairs)
    assert_equals_model(pb, e, "align")
    ob = run_ops(al, m)
    up = uploaded(gpu_aligner_factory, amp, e)
    ob2 = run_ops(up, m)
    assert_same_ops(ob, ob2)
    assert al.path_counts() == up.path_counts()
    assert_same(oracle, amp, e.buf, e.offsets, ob.expand(amp, pb.buf, pb.offsets), "adopted")

    # the quantification and the allele grouping read the batch where it lies
    args = quant_args({"amplicon_seq": amp, "guide_seq": amp[90:110]}, {"window": 1})
    g = quantify.globals_from_args(args)
    score = _printed_percents(ob.stats["n_ident"], np.maximum(ob.stats["aln_len"], 1))
    keep = ((ob.stats["flags"] & _lib.NW_FLAG_EMPTY) == 0) & (score > 60.0)
    got = []
    with quantify.GpuQuantifier(0) as gq:
        gq.set_params(g, args)
        for a, buf, off in ((al, pb.buf, pb.offsets), (up, e.buf, e.offsets)):
            with DeviceBuffer.from_array(quantify.pre_flags(score == 100)) as d_pre, DeviceBuffer(16 * m) as d_out:
                gq.run_device_ops(amp, a.device_ops(), d_pre.ptr, m, d_out.ptr)
                rr = d_out.download(np.zeros((m, 4), np.int32))
            gr = alleles.group_reads(a, buf, off, keep=keep)
            got.append((rr, gr.first.tolist(), gr.count.tolist()))
    assert np.array_equal(got[0][0], got[1][0])
    assert got[0][1:] == got[1][1:]
    assert sum(got[0][2]) == int(keep.sum())


# ---- the reference's pinned runs from the raw pairs, no file between the stages -------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_pinned_runs_from_raw_pairs(gpu_aligner_factory, name):
    import gzip
    import json

    from crispresso_amd.fastq import fasta_name
    from crispresso_amd.flash import read_fastq
    from crispresso_amd.needle import ops_to_dataframe

    case = dict(CASES[name], name=name)
    with gzip.open(os.path.join(HERE, case["fixture"]), "rt") as f:
        fx = json.load(f)
    args = quant_args(fx, case)
    amp = args.amplicon_seq
    al = gpu_aligner_factory()
    al.set_reference(amp)
    r1, r2 = (os.path.join(HERE, f"{case['prefix']}_L001_R{r}_001.fastq.gz") for r in (1, 2))
    pb, names = frontend.prepare_fastq(al, r1, r2, trim=case["trim"], flash=FLASH)
    assert pb.stats["pairs"] == case["pairs"] and len(pb) == case["merged"]
    # the batch's (name, read) list is the fixture's: R1's header lines at src, and their FASTA names
    headers = read_fastq(r1)[0]
    assert [[headers[int(i)].decode(), pb.read(j).decode()] for j, i in enumerate(pb.src)] == fx["merged_reads"]
    assert names == [fasta_name(b"@" + n.encode()) for n, _ in fx["merged_reads"]]
    ob = run_ops(al, len(pb))
    df = ops_to_dataframe(ob, amp, pb.buf, pb.offsets, names, "ref")
    df = df.loc[(df.score_ref > case["min_identity"]).to_numpy()].copy()
    check_rows(df, fx)
    g = quantify.globals_from_args(args)
    quantify.quantify_alignments(df, args, globals_=g)
    cuts = quantify.compute_cut_points(amp, args.guide_seq)
    assert summary_values(quantify.run_summary(df, g.LEN_AMPLICON, cuts)) == expected(fx)


# ---- refusals -------------------------------------------------------------------------------

def test_refusals(gpu_aligner_factory):
    from crispresso_amd.aligner import GpuAligner

    s, q, off, _, _, _ = fm.packed_inputs(simple_pairs(2, 3))
    al = gpu_aligner_factory()
    al.set_reference("ACGT" * 30)
    long_s = np.full(4097, ord("A"), np.uint8)
    long_q = np.full(4097, ord("I"), np.uint8)
    long_off = np.array([0, 4097], np.int64)
    with pytest.raises(frontend.FrontError) as ei:
        frontend.prepare_packed(al, long_s, long_q, long_off, long_s, long_q, long_off)
    assert ei.value.code == -3
    bad = np.array([0, 10, 5, len(s)], np.int64)
    with pytest.raises(frontend.FrontError) as ei:
        frontend.prepare_packed(al, s, q, bad, s, q, bad)
    assert ei.value.code == -1
    with GpuAligner(0) as bare:   # no reference
        with pytest.raises(frontend.FrontError) as ei:
            frontend.prepare_packed(bare, s, q, off, s, q, off)
        assert ei.value.code == _lib.NW_E_STATE
    al.set_output("rows")
    with pytest.raises(frontend.FrontError) as ei:
        frontend.prepare_packed(al, s, q, off, s, q, off, force_ops_output=False)
    assert ei.value.code == _lib.NW_E_STATE
    with pytest.raises(UnsupportedTrimStep):
        frontend.prepare_packed(al, s, q, off, s, q, off, trim="MAXINFO:40:0.5")
    with pytest.raises(UnsupportedTrimStep):
        frontend.prepare_packed(al, s, q, off, s, q, off, trim="TOPHRED33")
