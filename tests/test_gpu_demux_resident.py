"""The device-resident hand-off of the pooled amplicon flow (nwd_pack, nwd_fetch_packed,
nwd_adopt_group; crispresso_amd.demux.align_demultiplexed_resident): the packer against the host
packer on demultiplex's own text and against tests/demux_pack_model.py, the adopted groups
against the host path, the model's groups and the needle oracle.  Everything exact."""
import ctypes
import json
import os
import subprocess
import sys
import types

import numpy as np
import pandas as pd
import pytest

from crispresso_amd import _lib, aligner, alleles, demux, quantify
from crispresso_amd.devmem import DeviceBuffer
from tests import demux_cases as dc
from tests import demux_model as dm
from tests import demux_pack_cases as pc
from tests import demux_pack_model as pm
from tests.alleles_cases import pack
from tests.helpers import oracle_batch, runs_from_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_CASES = ("lengths", "strand_breaks", "phases")


@pytest.fixture(scope="module")
def d():
    with demux.GpuDemultiplexer(0) as x:
        yield x


def check_pack(d, name):
    """One case through set_amplicons / assign / pack / fetch_packed, held to the model and to
    pack_2bit of demultiplex's own text; returns the digest of everything the packer gave."""
    amps, reads, want = pc.case(name)
    got, pk, packed, pos, byt = pc.run_pack(d, amps, reads)
    assert got[0].tolist() == want["which"] and got[1].tolist() == want["strand"]
    order, strands, dst = pm.layout(want, reads)
    m_packed, m_pos, m_byt = pm.pack(order, strands, dst, reads)
    assert pk.group_offsets.tolist() == want["group_offsets"] and pk.order.tolist() == order
    assert pk.text_offsets.tolist() == dst and pk.lens.dtype == np.uint16
    assert pk.lens.tolist() == np.diff(dst).tolist()
    assert packed.tobytes() == m_packed.tobytes(), "the 2-bit stream differs from the model's"
    assert pos.tolist() == m_pos.tolist() and byt.tolist() == m_byt.tolist() and pk.n_exc == len(m_pos)
    assert pk.group_exc.tolist() == pm.group_exceptions(m_pos, dst, want["group_offsets"])
    out = pc.digest(pk, packed, pos, byt)
    # the same from the path this replaces: the gathered text, packed on the host
    res = demux.demultiplex(list(amps), pack(reads), demultiplexer=d, **pc.KW)
    assert not dc.mismatches(res, want)
    host = aligner.pack_2bit(res.text, res.text_offsets)
    nbytes = (dst[-1] + 3) // 4
    assert len(packed) == nbytes and packed.tobytes() == host.packed[:nbytes].tobytes()
    assert np.array_equal(pos, host.exc_pos) and np.array_equal(byt, host.exc_byte)
    assert np.array_equal(pk.lens, host.lens[:len(order)])
    for name_ in ("group_offsets", "order", "text_offsets"):
        assert np.array_equal(getattr(pk, name_), getattr(res, name_)), name_
    return out, pk, packed, pos


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_packer_parity(d, name):
    _, pk, packed, pos = check_pack(d, name)
    assert (pk.n_exc > 0) == (name in ("strand_breaks", "exception_blocks", "long_group"))
    if name == "none_assigned":
        assert pk.group_offsets.tolist() == [0, 0, 0] and pk.text_offsets.tolist() == [0] and pk.kernel_ms == 0.0
        assert len(packed) == 0 and len(pos) == 0 and pk.group_exc.tolist() == [0, 0, 0]


def test_no_reads_at_all(d):
    amps, _, _ = pc.case("none_assigned")
    _, pk, packed, pos, byt = pc.run_pack(d, amps, [])
    assert pk.group_offsets.tolist() == [0, 0, 0] and pk.text_offsets.tolist() == [0] and pk.n_exc == 0
    assert pk.kernel_ms == 0.0 and len(pk.order) == len(pk.lens) == len(packed) == len(pos) == len(byt) == 0


def test_pack_twice_and_second_assign(d):
    amps, reads, _ = pc.case("strand_breaks")
    _, pk, packed, pos, byt = pc.run_pack(d, amps, reads)
    first = pc.digest(pk, packed, pos, byt)
    pk2 = d.pack(len(pk.order))
    assert pc.digest(pk2, *d.fetch_packed()) == first
    # gather after pack leaves the packed arrays alone
    goff, order, text, toff = d.gather(len(pk.order), int(pk.text_offsets[-1]))
    assert np.array_equal(toff, pk.text_offsets) and pc.digest(pk2, *d.fetch_packed()) == first
    # a second assign replaces the first: the other case's result, not a mix
    other = check_pack(d, "exception_blocks")[0]
    assert other != first
    assert check_pack(d, "strand_breaks")[0] == first


def child(names, **env):
    p = subprocess.run([sys.executable, "-m", "tests.demux_pack_cases", *names], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("env", [{"CRISPR_NWD_CHUNK": "1"}, {"CRISPR_NWD_CHUNK": "7"}, {"CRISPR_NWD_CHUNK": "64"},
                                 {"CRISPR_NWD_TALLY_SLOTS": "2"}], ids=lambda e: "-".join(e.values()))
def test_settings_leave_the_packer_unchanged(d, env):
    """The chunked upload and the fallback reads (settings read at nwd_create: a child process)
    give the same bytes."""
    here = [check_pack(d, name)[0] for name in CHILD_CASES]
    out = child(CHILD_CASES, **env)
    assert out["digest"] == here
    if "CRISPR_NWD_TALLY_SLOTS" in env:
        assert sum(out["fallback"]) > 0      # (a 4096-base read has 8-mers of other amplicons)


# ---- the hand-off ------------------------------------------------------------------------------

def panel(variant):
    """dc.pooled_panel(): 8 amplicons x 50 reads.  "flipped": every odd read reverse-complemented
    and one N put into ten of the reads; "breaks": the panel's own strands with those N."""
    amps, reads = dc.pooled_panel()
    if variant == "flipped":
        reads = [dm.revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
    if variant in ("flipped", "breaks"):
        for t, i in enumerate(range(5, 400, 40)):          # five even and five odd reads
            i += t % 2
            p = (17 * t + 3) % len(reads[i])
            reads[i] = reads[i][:p] + b"N" + reads[i][p + 1:]
    return amps, reads


def model_groups(amps, reads):
    want = dm.demultiplex([a.encode() for a in amps], reads)
    flat = [r for grp in want["groups"] for r in grp]
    buf, off = pack(flat)
    which = np.repeat(np.arange(len(amps), dtype=np.int32), want["counts"])
    return want, buf, off, which


def assert_group_equals(ob, ref, lo, hi):
    """ob (one group's OpsBatch) against reads lo..hi of the whole-call OpsBatch ref."""
    o0, o1 = int(ref.ops_off[lo]), int(ref.ops_off[hi])
    assert len(ob) == hi - lo
    assert np.array_equal(ob.stats, ref.stats[lo:hi])
    assert np.array_equal(ob.ops_off, ref.ops_off[lo:hi + 1] - o0)
    assert np.array_equal(ob.ops, ref.ops[o0:o1])
    assert np.array_equal(ob.read_lens, ref.read_lens[lo:hi])


@pytest.mark.parametrize("variant", ["plain", "flipped", "breaks"])
def test_hand_off_parity_and_oracle(d, gpu_aligner_factory, variant):
    amps, reads = panel(variant)
    want, buf, off, which = model_groups(amps, reads)
    assert sum(want["counts"]) >= 390 and min(want["counts"]) >= 45
    al = gpu_aligner_factory()
    ref = al.align_multi_ops(amps, buf, off, which)
    assert al.output_mode == "rows"
    seen = []
    obs, res, skipped = demux.align_demultiplexed_resident(amps, pack(reads), al, demultiplexer=d, with_text=True,
                                                           on_group=lambda g, a, n: seen.append((g, n)))
    assert al.output_mode == "rows"                       # restored
    assert skipped == [] and not dc.mismatches(res, want)
    assert seen == [(g, want["counts"][g]) for g in range(8)]
    goff = want["group_offsets"]
    # any order of adoption, any number of times: a slice's result does not depend on what came before
    pk = d._packed
    al.set_output("ops")
    for g in (5, 0, 7, 5):
        al.set_reference(amps[g])
        n = d.adopt(al, g)
        al.run_async()
        al.sync()
        assert_group_equals(al.download_ops(n), ref, goff[g], goff[g + 1])
    assert pk is d._packed
    al.set_output("rows")
    host, _, _ = demux.align_demultiplexed(amps, pack(reads), al, demultiplexer=d)
    n_exc = 0
    for g in range(8):
        lo, hi = goff[g], goff[g + 1]
        assert_group_equals(obs[g], ref, lo, hi)
        gbuf, goffs = res.reads_per_amplicon()[g]
        rows = obs[g].expand(amps[g], gbuf, goffs)
        oracle = oracle_batch(amps[g], gbuf, np.ascontiguousarray(goffs))
        for f in ("aln_len", "n_ident", "n_sim", "n_gaps", "score", "end_i", "end_j"):
            assert np.array_equal(rows.stats[f], oracle.stats[f]), (g, f)
        assert np.array_equal(rows.stats, host[g].stats) and np.array_equal(rows.read_lens, host[g].read_lens)
        for i in range(hi - lo):
            L = int(oracle.stats["aln_len"][i])
            assert np.array_equal(rows.aln[i, :, :L], host[g].aln[i, :, :L])
            assert np.array_equal(rows.aln[i, :, :L], oracle.aln[i, :, :L]), (g, i)
            if b"-" not in want["groups"][g][i]:
                assert obs[g].ops[obs[g].ops_off[i]:obs[g].ops_off[i + 1]].tolist() == \
                    runs_from_rows(oracle.aln[i, 0, :L].tobytes(), oracle.aln[i, 2, :L].tobytes())
        n_exc += sum(r.count(b"N") for r in want["groups"][g])
    assert n_exc == (0 if variant == "plain" else 10)


def test_min_reads_is_strict(d, gpu_aligner_factory):
    amps, reads = dc.pooled_panel()
    fewer = [r for i, r in enumerate(reads) if not (i % 8 == 3 and i > 200) and not (i % 8 == 5 and i > 350)]
    want, buf, off, which = model_groups(amps, fewer)
    counts = want["counts"]
    assert counts[3] < counts[5] < 50 and [counts[g] for g in (0, 1, 2, 4, 6, 7)] == [50] * 6
    al = gpu_aligner_factory()
    ref = al.align_multi_ops(amps, buf, off, which)
    obs, res, skipped = demux.align_demultiplexed_resident(amps, pack(fewer), al, min_reads=counts[5], demultiplexer=d)
    assert skipped == [3, 5] and res.counts.tolist() == counts and len(res.text) == 0
    assert all((obs[g] is None) == (g in skipped) for g in range(8))
    goff = want["group_offsets"]
    for g in (0, 7):
        assert_group_equals(obs[g], ref, goff[g], goff[g + 1])
    obs, res, skipped = demux.align_demultiplexed_resident(amps, pack(fewer), al, min_reads=counts[5] - 1, demultiplexer=d)
    assert skipped == [3] and len(obs[5]) == counts[5]
    assert_group_equals(obs[5], ref, goff[5], goff[6])


def test_long_group_through_the_aligner(d, gpu_aligner_factory):
    """A group of kLenGroup + 1 reads that starts at gathered read 3: the adoption's group-base
    offsets count from the group's first read."""
    amps, reads, want = pc.case("long_group")
    names = [a.decode() for a in amps]
    flat = [r for grp in want["groups"] for r in grp]
    buf, off = pack(flat)
    al = gpu_aligner_factory()
    ref = al.align_multi_ops(names, buf, off, np.repeat(np.arange(len(amps), dtype=np.int32), want["counts"]))
    obs, res, skipped = demux.align_demultiplexed_resident(names, pack(reads), al, demultiplexer=d, **pc.KW)
    assert skipped == [0, 3, 4, 5] and res.counts.tolist() == want["counts"]
    goff = want["group_offsets"]
    for g in (1, 2):
        assert_group_equals(obs[g], ref, goff[g], goff[g + 1])


# ---- a consumer on the resident group ----------------------------------------------------------

def quant_args(amp):
    mid = len(amp) // 2
    return types.SimpleNamespace(
        amplicon_seq=amp, guide_seq=amp[mid - 10:mid + 10], cleavage_offset=-3, window_around_sgrna=1,
        exclude_bp_from_left=15, exclude_bp_from_right=15, coding_seq=None, ignore_substitutions=False,
        ignore_insertions=False, ignore_deletions=False, hide_mutations_outside_window_NHEJ=False,
        expected_hdr_amplicon_seq=None, hdr_perfect_alignment_threshold=98.0)


def consume(al, gq, grouper, amp, buf, off, n):
    """Quantification totals, per-read results and the allele table from the batch resident in
    ``al`` (already run); buf / off: the group's text on the host."""
    from crispresso_amd.needle import _printed_percents

    dev = al.device_ops()
    ob = al.download_ops(n)
    score = _printed_percents(ob.stats["n_ident"], np.maximum(ob.stats["aln_len"], 1))
    keep = ((ob.stats["flags"] & _lib.NW_FLAG_EMPTY) == 0) & (score > 60.0)
    args = quant_args(amp)
    gq.set_params(quantify.globals_from_args(args), args)
    with DeviceBuffer.from_array(quantify.pre_flags(score == 100)) as d_pre, DeviceBuffer(16 * n) as d_out:
        totals = gq.run_device_ops(amp, dev, d_pre.ptr, n, d_out.ptr)
        rr = d_out.download(np.zeros((n, 4), np.int32))
    groups = grouper.group(dev, n, keep=keep, want_group_of_read=True)
    table = alleles.allele_table(amp, buf, off, ob, rr, groups)
    return totals, rr, groups, table


def test_resident_consumers(d, gpu_aligner_factory):
    amps, reads = panel("breaks")
    want, _, _, _ = model_groups(amps, reads)
    al = gpu_aligner_factory()
    picked = (2, 6)
    texts = {g: pack(want["groups"][g]) for g in picked}
    got = {}
    with quantify.GpuQuantifier(0) as gq, alleles.GpuAlleleGrouper(0) as grouper:
        def on_group(g, a, n):
            if g in picked:
                got[g] = consume(a, gq, grouper, amps[g], *texts[g], n)

        demux.align_demultiplexed_resident(amps, pack(reads), al, demultiplexer=d, on_group=on_group)
        assert sorted(got) == list(picked)
        al.set_output("ops")
        for g in picked:      # the host path: the group's text packed on the host and uploaded
            buf, off = texts[g]
            al.set_reference(amps[g])
            al.upload_packed(aligner.pack_2bit(buf, off))
            al.run_async()
            al.sync()
            totals, rr, groups, table = consume(al, gq, grouper, amps[g], buf, off, len(off) - 1)
            assert totals.any() and np.array_equal(got[g][0], totals)
            assert np.array_equal(got[g][1], rr)
            assert got[g][2].first.tolist() == groups.first.tolist() and got[g][2].count.tolist() == groups.count.tolist()
            pd.testing.assert_frame_equal(got[g][3].reset_index(drop=True), table.reset_index(drop=True))
            assert len(table) > 1


# ---- refusals at the C entry -------------------------------------------------------------------

def test_c_entry_refusals(gpu_aligner_factory):
    amps, reads = dc.pooled_panel()
    want, buf, off, which = model_groups(amps, reads)
    extra = amps + [dc.bases(150, 99).decode()]            # no read comes from the last one
    al, bare, rows = gpu_aligner_factory(), gpu_aligner_factory(), gpu_aligner_factory()
    ref = al.align_multi_ops(amps, buf, off, which)
    al.set_output("ops")
    al.set_reference(amps[2])
    bare.set_output("ops")
    rows.set_reference(amps[2])
    with demux.GpuDemultiplexer(0) as fresh:
        lib, ctx = fresh._lib, fresh._ctx

        def refused(rc, code):
            assert rc == code and lib.nwd_last_error(ctx), (rc, code)

        refused(lib.nwd_pack(ctx, *[None] * 7), _lib.NW_E_STATE)                       # no index yet
        refused(lib.nwd_fetch_packed(ctx, None, 0, None, None, None), _lib.NW_E_STATE)
        refused(lib.nwd_adopt_group(ctx, al._h, 0), _lib.NW_E_STATE)
        abuf, aoff = demux.pack_amplicons(extra)
        rbuf, roff = pack(reads)
        fresh.set_amplicons(abuf, aoff, 16)
        got = fresh.assign(rbuf, roff, 2, True)
        refused(lib.nwd_adopt_group(ctx, al._h, 2), _lib.NW_E_STATE)                   # adopt before pack
        refused(lib.nwd_fetch_packed(ctx, None, 0, None, None, None), _lib.NW_E_STATE)
        ne = ctypes.c_int64(-1)
        assert lib.nwd_pack(ctx, None, None, None, None, None, ctypes.byref(ne), None) == 0 and ne.value == 0
        pk = fresh.pack(got[5])
        for g in (-1, 9, 1 << 40):
            refused(lib.nwd_adopt_group(ctx, al._h, g), _lib.NW_E_INVALID)             # g out of range
        refused(lib.nwd_adopt_group(ctx, al._h, 8), _lib.NW_E_INVALID)                 # an empty group
        refused(lib.nwd_adopt_group(ctx, None, 2), _lib.NW_E_INVALID)
        refused(lib.nwd_adopt_group(ctx, bare._h, 2), _lib.NW_E_STATE)                 # no reference
        assert b"nw_set_reference" in lib.nwd_last_error(ctx)
        refused(lib.nwd_adopt_group(ctx, rows._h, 2), _lib.NW_E_STATE)                 # rows mode
        assert b"NW_OUT_OPS" in lib.nwd_last_error(ctx)
        nbytes = (int(pk.text_offsets[-1]) + 3) // 4
        need = ctypes.c_int64()
        packed = np.zeros(nbytes, np.uint8)
        for cap in (0, nbytes - 1):
            refused(lib.nwd_fetch_packed(ctx, _lib.ptr(packed), cap, None, None, ctypes.byref(need)), _lib.NW_E_CAPACITY)
            assert need.value == nbytes and not packed.any()
        assert lib.nwd_fetch_packed(ctx, _lib.ptr(packed), nbytes, None, None, None) == 0
        text, toff = pack([r for grp in want["groups"] for r in grp])
        assert packed.tobytes() == aligner.pack_2bit(text, toff).packed[:nbytes].tobytes()
        # both contexts are as they were: the next valid calls give the parity result
        goff = want["group_offsets"]
        for g in (2, 7):
            al.set_reference(amps[g])
            n = fresh.adopt(al, g)
            al.run_async()
            al.sync()
            assert_group_equals(al.download_ops(n), ref, goff[g], goff[g + 1])
        # and the aligners the refusals named still work
        for other in (bare, rows):
            other.set_output("ops")
            other.set_reference(amps[4])
            n = fresh.adopt(other, 4)
            other.run_async()
            other.sync()
            assert_group_equals(other.download_ops(n), ref, goff[4], goff[5])
