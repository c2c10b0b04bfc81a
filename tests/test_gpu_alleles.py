"""The allele grouping kernels (crispresso_amd/csrc/nw_alleles.hip, include/crispr_alleles.h)
against a plain dict over (tag, bytes), and allele_table on the aligner's resident batch against
quantify.run_summary's df_alleles over the per-read DataFrame of the same kept reads."""
import ctypes
import json
import os
import subprocess
import sys
import types

import numpy as np
import pandas as pd
import pytest

from crispresso_amd import _lib, alleles, quantify, synth
from tests import alleles_cases as ac

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ac.families()


@pytest.fixture(scope="module")
def nwa():
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    assert lib.nwa_create(0, ctypes.byref(ctx)) == 0
    yield lib, ctx
    lib.nwa_destroy(ctx)


def check(nwa, reads, keep=None, tag=None, lead=0, bias=0):
    lib, ctx = nwa
    want = ac.expected_groups(reads, keep, tag)
    for _ in range(2):     # the second call reuses the context's buffers
        rc, first, count, gor, ng = ac.device_group(lib, ctx, reads, keep, tag, lead, bias)
        assert rc == 0, lib.nwa_last_error(ctx)
        assert ng == len(want[0])
        assert (first, count, gor) == want
        assert all(a < b for a, b in zip(first, first[1:]))
        assert lib.nwa_last_collided(ctx) == 0
    rc, first, count, gor, ng = ac.device_group(lib, ctx, reads, keep, tag, lead, bias, want_gor=False)
    assert rc == 0 and (first, count) == want[:2]


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_group_device_equals_dict(nwa, name):
    reads, keep, tag = FAMILIES[name]
    check(nwa, reads, keep, tag)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_every_start_alignment_and_bias(nwa, lead):
    """The batch starts at every offset mod 4 (the reads' odd lengths move every later start),
    with and without a bias on the offsets."""
    reads, _, _ = FAMILIES["near_equal"]
    check(nwa, reads, lead=lead)
    check(nwa, reads + ac.random_reads(200, 9), tag=np.arange(len(reads) + 200, dtype=np.int32) % 2, lead=lead,
          bias=1000003)


def test_identical_reads_one_slot(nwa):
    """20,000 copies of one 250-byte read: one slot, the count added once per wavefront."""
    read = bytes(np.random.Generator(np.random.PCG64(1)).choice(np.frombuffer(b"ACGT", np.uint8), 250))
    check(nwa, [read] * 20000)
    check(nwa, [read] * 20000, keep=(np.arange(20000) % 7 != 0).astype(np.uint8), lead=3)


def test_all_distinct_reads(nwa):
    """20,000 distinct reads: every read claims a slot (table at half load, probe chains)."""
    rng = np.random.Generator(np.random.PCG64(2))
    body = rng.choice(np.frombuffer(b"ACGT", np.uint8), (20000, 24))
    reads = [bytes(body[i]) + b"%05d" % i for i in range(20000)]
    assert len(set(reads)) == 20000
    check(nwa, reads, lead=1)


def test_every_wavefront_takes_several_reads(nwa):
    """More than twice the reads one step of the hash / verify launch takes (2 * 4 * 16 * CUs + 5)."""
    lib, ctx = nwa
    slots = int(lib.nwa_reads_per_step(ctx))
    assert slots > 0 and slots % 64 == 0
    check(nwa, ac.random_reads(2 * slots + 5, 4, pool=300, lengths=(0, 1, 7, 8, 9, 30, 63, 64, 65, 130)))


def test_capacity_and_invalid(nwa):
    lib, ctx = nwa
    reads, _, _ = FAMILIES["size5000"]
    want = ac.expected_groups(reads)
    need = len(want[0])
    rc, first, count, gor, ng = ac.device_group(lib, ctx, reads, cap=need - 1)
    assert rc == _lib.NW_E_CAPACITY and ng == need
    assert gor == [-5] * len(reads)                       # nothing else written
    rc, first, count, gor, ng = ac.device_group(lib, ctx, reads, cap=need)
    assert rc == 0 and (first, count, gor) == want
    n_out = ctypes.c_int64()
    one = np.zeros(1, np.int64)
    for n in (-1, 2 ** 31):
        assert lib.nwa_group_device(ctx, None, None, 0, n, None, None, _lib.ptr(one), _lib.ptr(one), 1, None,
                                    ctypes.byref(n_out), None) == _lib.NW_E_INVALID


@pytest.mark.parametrize("bits", [0, 3, 12])
def test_forced_collisions(bits):
    """CRISPR_NWA_HASH_BITS cuts the hash to `bits` bits (read at nwa_create: a child process
    each): equal hashes of different reads go through the probe chains, the verify pass and the
    host's exact grouping, and the groups are still the dict's."""
    reads = ac.collision_reads()
    distinct = len(set(reads))
    assert len(reads) == 2000 and distinct == 200
    if bits <= 3:
        assert distinct > 2 ** bits                        # collisions are certain, not just likely
    env = dict(os.environ, CRISPR_NWA_HASH_BITS=str(bits))
    p = subprocess.run([sys.executable, "-m", "tests.alleles_cases", "forced"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"], out
    assert all(c > 0 for c in out["collided"]), out


# ------------------------------------------------------------------ after the aligner

@pytest.fixture(scope="module")
def gq():
    q = quantify.GpuQuantifier(0)
    yield q
    q.close()


@pytest.fixture(scope="module")
def grouper():
    with alleles.GpuAlleleGrouper(0) as g:
        yield g


def quant_args(amp):
    return types.SimpleNamespace(
        amplicon_seq=amp, guide_seq=amp[105:125], cleavage_offset=-3, window_around_sgrna=1, exclude_bp_from_left=15,
        exclude_bp_from_right=15, coding_seq=None, ignore_substitutions=False, ignore_insertions=False,
        ignore_deletions=False, hide_mutations_outside_window_NHEJ=False, expected_hdr_amplicon_seq=None,
        hdr_perfect_alignment_threshold=98.0)


def kept_reads(stats, min_identity):
    from crispresso_amd.needle import _printed_percents

    live = (stats["flags"] & _lib.NW_FLAG_EMPTY) == 0
    score = _printed_percents(stats["n_ident"], np.maximum(stats["aln_len"], 1))
    return live & (score > min_identity), score


def resident_tables(al, gq, grouper, amp, buf, off, min_identity, packed=True):
    """(allele_table on the resident batch, run_summary's df_alleles over the DataFrame path on
    the same kept reads, the groups, the per-read results)."""
    from crispresso_amd.aligner import pack_2bit
    from crispresso_amd.devmem import DeviceBuffer
    from crispresso_amd.needle import ops_to_dataframe

    n = len(off) - 1
    al.set_reference(amp)
    al.set_output("ops")
    if packed:
        al.upload_packed(pack_2bit(buf, off))
    else:
        al.upload(buf, off)
    al.run_async()
    al.sync()
    dev = al.device_ops()
    ob = al.download_ops(n)
    keep, score = kept_reads(ob.stats, min_identity)
    args = quant_args(amp)
    g = quantify.globals_from_args(args)
    gq.set_params(g, args)
    with DeviceBuffer.from_array(quantify.pre_flags(score == 100)) as d_pre, DeviceBuffer(16 * n) as d_out:
        gq.run_device_ops(amp, dev, d_pre.ptr, n, d_out.ptr)
        rr = d_out.download(np.zeros((n, 4), np.int32))
    groups = alleles.group_reads(al, buf, off, keep=keep)
    direct = grouper.group(dev, n, keep=keep, want_group_of_read=True)
    assert direct.first.tolist() == groups.first.tolist() and direct.count.tolist() == groups.count.tolist()
    assert groups.collided == 0
    got = alleles.allele_table(amp, buf, off, ob, rr, groups)
    # the path it replaces: one DataFrame row per read, quantified, grouped by pandas
    df = ops_to_dataframe(ob, amp, buf, off, [f"r{i}" for i in range(n)], "ref")
    df = df.loc[(df.score_ref > min_identity).to_numpy()].copy()
    assert len(df) == int(keep.sum())
    quantify.quantify_alignments(df, args, quantifier=gq, globals_=g)
    cuts = quantify.compute_cut_points(amp, args.guide_seq)
    want = quantify.run_summary(df, len(amp), cuts)["df_alleles"]
    return got, want, direct, rr, ob, keep


def assert_tables_equal(got, want):
    pd.testing.assert_frame_equal(got.reset_index(drop=True), want.reset_index(drop=True))


def test_after_aligner_c2(gpu_aligner_factory, gq, grouper):
    amp = synth.random_amplicon(250, 31)
    buf, off = synth.reads_from(amp, 12000, 32)
    got, want, groups, rr, ob, keep = resident_tables(gpu_aligner_factory(), gq, grouper, amp, buf, off, 60.0)
    assert_tables_equal(got, want)
    reads = [bytes(buf[off[r]:off[r + 1]]) for r in range(len(off) - 1)]
    assert (groups.first.tolist(), groups.count.tolist(), groups.group_of_read.tolist()) == \
        ac.expected_groups(reads, keep)


def test_after_aligner_parity_mix(gpu_aligner_factory, gq, grouper):
    """N bytes (exceptions of the 2-bit pack) and reverse-complemented reads, which the identity
    filter drops (keep = printed identity > 60)."""
    amp = synth.random_amplicon(250, 33)
    buf, off = synth.reads_from(amp, 12000, 34, synth.PARITY_MIX)
    got, want, groups, rr, ob, keep = resident_tables(gpu_aligner_factory(), gq, grouper, amp, buf, off, 60.0)
    assert 0 < int(keep.sum()) < len(keep)
    assert_tables_equal(got, want)


def test_after_aligner_short_reads(gpu_aligner_factory, gq, grouper):
    """151-bp reads on a 280-bp amplicon (the reference's own test shape), min_identity 30."""
    amp = synth.random_amplicon(280, 35)
    buf, off = synth.window_reads(amp, 12000, 36, 151)
    got, want, groups, rr, ob, keep = resident_tables(gpu_aligner_factory(), gq, grouper, amp, buf, off, 30.0,
                                                      packed=False)
    assert_tables_equal(got, want)


def test_pooled_tags(gpu_aligner_factory, gq, grouper):
    """3 amplicons x 2,000 reads in one pooled pass (align_multi_ops), grouped with tag =
    ref_of_read; amplicon 0's exact copy is planted among amplicon 1's reads: the same bytes
    against two amplicons are two alleles.  Per-amplicon tables against the single-amplicon
    DataFrame path."""
    from crispresso_amd.devmem import DeviceBuffer

    al = gpu_aligner_factory()
    amps = [synth.random_amplicon(250, 40 + a) for a in range(3)]
    reads, tag = [], []
    for a, amp in enumerate(amps):
        b, o = synth.reads_from(amp, 2000, 50 + a)
        reads += [bytes(b[o[r]:o[r + 1]]) for r in range(2000)]
        tag += [a] * 2000
    reads[2000 + 17] = amps[0].encode()                 # the plant: amplicon 0's bytes, tag 1
    assert amps[0].encode() in reads[:2000]
    tag = np.array(tag, np.int32)
    buf, off = ac.pack(reads)
    n = len(reads)
    want, rr, keep = [], np.zeros((n, 4), np.int32), np.zeros(n, bool)
    for a, amp in enumerate(amps):
        sel = np.flatnonzero(tag == a)
        sb, so = ac.pack([reads[r] for r in sel])
        _, w, _, rr_a, _, keep_a = resident_tables(al, gq, grouper, amp, sb, so, 30.0, packed=False)
        want.append(w)
        rr[sel] = rr_a
        keep[sel] = keep_a
    assert keep[2000 + 17]
    ob = al.align_multi_ops(amps, buf, off, tag)
    with DeviceBuffer.from_array(buf) as d_buf, DeviceBuffer.from_array(off + 7) as d_off:
        dev = {"reads": d_buf.ptr, "offsets": d_off.ptr, "reads_bias": 7}
        groups = grouper.group(dev, n, keep=keep, tag=tag, want_group_of_read=True)
    assert (groups.first.tolist(), groups.count.tolist(), groups.group_of_read.tolist()) == \
        ac.expected_groups(reads, keep, tag)
    assert groups.group_of_read[2000 + 17] != groups.group_of_read[reads.index(amps[0].encode())]
    for a, amp in enumerate(amps):
        mine = tag[groups.first] == a
        ga = alleles.ReadGroups(groups.first[mine], groups.count[mine], None)
        assert_tables_equal(alleles.allele_table(amp, buf, off, ob, rr, ga), want[a])


def test_reference_pin(tmp_path, gpu_aligner_factory, gq, grouper):
    """The reference's `test` run from the raw pairs (tests/crispresso_tests.py:125-195): the four
    most frequent alleles from allele_table on the resident batch."""
    import gzip

    from crispresso_amd import fastq
    from crispresso_amd.flash import FlashOptions, run_flash
    from tests.test_e2e_pin import CASES, HERE, restated_merge

    case = dict(CASES["test"], name="test")
    with gzip.open(os.path.join(HERE, case["fixture"]), "rt") as f:
        fx = json.load(f)
    r1, r2 = restated_merge(case, tmp_path)
    st = run_flash(r1, r2, str(tmp_path), options=FlashOptions(min_overlap=4, max_overlap=100, allow_outies=True))
    assert st["combined"] == case["merged"]
    names, buf, off = fastq.read_fastq_as_fasta(str(tmp_path / "out.extendedFrags.fastq.gz"))
    amp = fx["amplicon_seq"].upper()
    al = gpu_aligner_factory()
    n = len(off) - 1
    al.set_reference(amp)
    al.set_output("ops")
    al.upload(buf, off)
    al.run_async()
    al.sync()
    dev = al.device_ops()
    ob = al.download_ops(n)
    keep, score = kept_reads(ob.stats, case["min_identity"])
    args = quant_args(amp)
    args.guide_seq, args.window_around_sgrna = fx["guide_seq"], case["window"]
    gq.set_params(quantify.globals_from_args(args), args)
    from crispresso_amd.devmem import DeviceBuffer

    with DeviceBuffer.from_array(quantify.pre_flags(score == 100)) as d_pre, DeviceBuffer(16 * n) as d_out:
        gq.run_device_ops(amp, dev, d_pre.ptr, n, d_out.ptr)
        rr = d_out.download(np.zeros((n, 4), np.int32))
    table = alleles.allele_table(amp, buf, off, ob, rr, alleles.group_reads(al, buf, off, keep=keep))
    assert int(table["#Reads"].sum()) == 7058
    assert [int(x) for x in table["#Reads"].values[:4]] == [1098, 346, 19, 17]
