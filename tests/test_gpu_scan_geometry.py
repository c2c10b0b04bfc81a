"""Every stage's block-sum scan past 1,024 block sums, against its model (the inputs and expected
arrays of tests/scan_geometry_cases.py, which tests/test_scan_geometry_cases.py pins to the slow
models): the front packer (nwp_scan_kernel), the demux packer (nwd_pack_scan_kernel), the region
extractor and packer (nwr_scan_kernel, both uses of nwr_pack_scan_kernel) and the allele grouper
(tile_scan_kernel, through nwa_group_device and nwa_table_device).  Integers and bytes, all exact;
no read, hit or group is sampled or skipped."""
import ctypes
import os

import numpy as np
import pytest

from crispresso_amd import _lib, demux, frontend, regions
from crispresso_amd.aligner import GpuAligner, pack_2bit
from crispresso_amd.devmem import DeviceBuffer
from crispresso_amd.needle_options import NeedleOptions
from tests import regions_cases as rc
from tests import scan_geometry_cases as sg
from tests.test_gpu_front import FLASH, assert_equals_model, assert_same_ops, run_ops

pytestmark = pytest.mark.gpu
FRONT_AMPLICON = "ACGTTGCAAGGCTTACGGATCCATGCAAGTCTAGGCTAAC"


# ---- 1. the front packer --------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(sg.FRONT_SIZES))
def test_front_packer(name):
    pool, pick, e, single_end = sg.front_case(name)
    kw = sg.front_settings(single_end)
    kw.pop("single_end")
    with GpuAligner(0, NeedleOptions()) as al:
        al.set_reference(FRONT_AMPLICON)
        pb = frontend.prepare_packed(al, *sg.front_inputs(pool, pick, single_end), with_quals=True, with_packed=True,
                                     flash=FLASH, **kw)
        assert_equals_model(pb, e, name)
        assert {k: pb.stats[k] for k in e.trim} == e.trim
        assert pb.stats["trim_pairs"] == sum(e.trim.values())
        assert pb.stats["bases"] == int(e.offsets[-1]) and pb.stats["exceptions"] == len(e.packed.exc_pos)
        if name != "se_1025":
            return
        # the adopted batch (gbase and the offset rebuild) against the same reads uploaded
        m = len(e.src)
        assert m % sg.LEN_GROUP == 0
        ob = run_ops(al, m)
        with GpuAligner(0, NeedleOptions()) as up:
            up.set_reference(FRONT_AMPLICON)
            up.upload_packed(pack_2bit(e.buf, e.offsets))
            assert_same_ops(ob, run_ops(up, m))


# ---- 2. the demux packer --------------------------------------------------------------------

@pytest.fixture(scope="module")
def demultiplexer():
    with demux.GpuDemultiplexer(0) as d:
        abuf, aoff = demux.pack_amplicons(list(sg.demux_amplicons()))
        d.set_amplicons(abuf, aoff, sg.DEMUX_K)
        yield d


@pytest.mark.parametrize("name", sorted(sg.DEMUX_SIZES))
def test_demux_packer(demultiplexer, name):
    d = demultiplexer
    pool, pick, e = sg.demux_case(name)
    rbuf, roff = pool.inputs.take(pick)
    got = d.assign(np.concatenate([rbuf, np.zeros(8, np.uint8)]), roff, sg.DEMUX_MIN_HITS, True)
    assert np.array_equal(got[0], e.which), np.flatnonzero(got[0] != e.which)[:10]
    assert np.array_equal(got[1], e.strand), np.flatnonzero(got[1] != e.strand)[:10]
    assert got[5] == len(e.order)
    pk = d.pack(got[5])
    packed, pos, byt = d.fetch_packed()
    assert np.array_equal(pk.group_offsets, e.group_offsets)
    assert np.array_equal(pk.order, e.order), np.flatnonzero(pk.order != e.order)[:10]
    assert np.array_equal(pk.text_offsets, e.text_offsets)
    assert pk.lens.dtype == np.uint16 and np.array_equal(pk.lens, e.lens)
    assert len(packed) == len(e.packed) and np.array_equal(packed, e.packed), np.flatnonzero(packed != e.packed)[:10]
    assert pk.n_exc == e.n_exc == len(pos)
    assert np.array_equal(pos, e.exc_pos), np.flatnonzero(pos != e.exc_pos)[:10]
    assert np.array_equal(byt, e.exc_byte), np.flatnonzero(byt != e.exc_byte)[:10]
    assert np.array_equal(pk.group_exc, e.group_exc)


# ---- 3. regions -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def extractor():
    assert "CRISPR_NWR_CHUNK" not in os.environ          # (read at creation: the BAM must stay one chunk)
    with regions.GpuRegionExtractor(0) as x:
        yield x


@pytest.fixture(scope="module")
def region_bam():
    pool, pick = sg.region_case()
    return regions.read_bam(sg.region_bam(pool, pick))


def test_region_extract(extractor, region_bam):
    want, major, packed, found = sg.region_expected()
    res = regions.extract_regions(region_bam, sg.REGION_TABLE, extractor=extractor)
    bad = rc.mismatches(rc.got_hits(res), want)
    assert not bad, "\n".join(bad)
    assert res.n_reads.tolist() == [len(h) for h in want["hits"]]
    text, off, roff, src, st, en = major
    assert np.array_equal(res.region_offsets, roff) and np.array_equal(res.src, src)
    assert np.array_equal(res.st, st) and np.array_equal(res.en, en)
    assert np.array_equal(res.text_offsets, off) and np.array_equal(res.text, text)


def test_region_packer(extractor, region_bam):
    want, major, host, found = sg.region_expected()
    text, off, roff, src, st, en = major
    with regions.extract_regions_resident(region_bam, sg.REGION_TABLE, extractor=extractor) as res:
        packed, pos, byt = res.fetch_packed()
        assert np.array_equal(res.region_offsets, roff) and np.array_equal(res.src, src)
        assert np.array_equal(res.st, st) and np.array_equal(res.en, en) and np.array_equal(res.text_offsets, off)
        assert res.lens.dtype == np.uint16 and np.array_equal(res.lens, np.diff(off))
        assert res.n_no_seq == want["n_no_seq"]
        nbytes = (int(off[-1]) + 3) // 4
        assert len(packed) == nbytes and np.array_equal(packed, host.packed[:nbytes]), \
            np.flatnonzero(packed != host.packed[:nbytes])[:10]
        assert res.n_exc == len(host.exc_pos) == len(pos)
        assert np.array_equal(pos, host.exc_pos), np.flatnonzero(pos != host.exc_pos)[:10]
        assert np.array_equal(byt, host.exc_byte), np.flatnonzero(byt != host.exc_byte)[:10]
        assert np.array_equal(res.region_exc, np.searchsorted(host.exc_pos, off[roff], side="left"))


def test_region_discover(extractor, region_bam):
    want, major, host, found = sg.region_expected()
    res = regions.discover_regions(region_bam, sg.DISCOVER_MIN_READS, extractor=extractor)
    table = [tuple(int(v) for v in (r["ref_id"], r["bpstart"], r["bpend"])) for r in res.region_table]
    assert table == found["regions"]
    assert res.regions == [(sg.REGION_REFS[k[0]][0], k[1], k[2]) for k in found["regions"]]
    assert res.n_records.tolist() == found["n_records"]
    assert (res.n_aligned, res.n_no_seq, res.n_kept) == (found["n_aligned"], found["n_no_seq"], found["n_kept"])
    assert res.n_emitted == sum(n >= sg.DISCOVER_MIN_READS for n in found["n_records"])
    bad = rc.mismatches(rc.got_hits(res), found)
    assert not bad, "\n".join(bad)
    assert res.n_reads.tolist() == [len(h) for h in found["hits"]]
    for g, s in enumerate(found["strand"]):
        assert res.strand(g).tobytes() == b"".join(s)


# ---- 4. the allele grouper ------------------------------------------------------------------

@pytest.fixture(scope="module")
def nwa():
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    assert lib.nwa_create(0, ctypes.byref(ctx)) == 0
    yield lib, ctx
    lib.nwa_destroy(ctx)


@pytest.mark.parametrize("name", sorted(sg.ALLELE_SIZES))
def test_allele_groups(nwa, name):
    lib, ctx = nwa
    pool, pick, keep = sg.allele_case(name)
    n = len(pick)
    buf, off = pool.take(pick)
    buf = np.concatenate([buf, np.full(8, 0xEE, np.uint8)])
    with DeviceBuffer.from_array(buf) as d_buf, DeviceBuffer.from_array(off) as d_off:
        for k in (keep, None):                           # values 0, 1 and 2, then NULL
            want_first, want_count, want_gor = sg.allele_groups(pick, k)
            cap = n if k is None else int(np.count_nonzero(k))
            first, count = np.full(cap, -5, np.int64), np.full(cap, -5, np.int64)
            gor = np.full(n, -5, np.int32)
            ng, ms = ctypes.c_int64(-5), ctypes.c_float()
            rc_ = lib.nwa_group_device(ctx, d_buf.ptr, d_off.ptr, 0, n, _lib.ptr(k), None, _lib.ptr(first), _lib.ptr(count),
                                       cap, _lib.ptr(gor), ctypes.byref(ng), ctypes.byref(ms))
            assert rc_ == 0, lib.nwa_last_error(ctx)
            g = int(ng.value)
            assert g == len(want_first)
            assert np.array_equal(first[:g], want_first), np.flatnonzero(first[:g] != want_first)[:10]
            assert np.array_equal(count[:g], want_count), np.flatnonzero(count[:g] != want_count)[:10]
            assert np.array_equal(gor, want_gor), np.flatnonzero(gor != want_gor)[:10]


def test_allele_table(nwa):
    """nwa_table_device reaches the shared grouping with the keep flags in HBM: the rows of every
    group's first read, an M run over the read and a Y run over the rest of the 16-base amplicon."""
    lib, ctx = nwa
    pool, pick, keep = sg.allele_case("two_steps")
    n = len(pick)
    buf, off = pool.take(pick)
    buf = np.concatenate([buf, np.full(8, 0xEE, np.uint8)])
    ops, ops_off, stats, rr = sg.allele_table_arrays(pool, pick)
    want_first, want_count, _ = sg.allele_groups(pick, keep)
    want_rows = sg.allele_table_rows(pool, pick, want_first)
    amp = sg.ALLELE_AMPLICON.encode()
    ng, stride = ctypes.c_int64(-5), ctypes.c_int32(-5)
    with DeviceBuffer.from_array(buf) as d_buf, DeviceBuffer.from_array(off) as d_off, \
            DeviceBuffer.from_array(ops) as d_ops, DeviceBuffer.from_array(ops_off) as d_ops_off, \
            DeviceBuffer.from_array(stats) as d_stats, DeviceBuffer.from_array(rr) as d_rr, \
            DeviceBuffer.from_array(keep) as d_keep:
        rc_ = lib.nwa_table_device(ctx, d_ops.ptr, d_ops_off.ptr, d_stats.ptr, d_buf.ptr, d_off.ptr, 0, n, 5000, amp,
                                   len(amp), d_keep.ptr, d_rr.ptr, ctypes.byref(ng), ctypes.byref(stride))
    assert rc_ == 0, lib.nwa_last_error(ctx)
    g, w = int(ng.value), int(stride.value)
    assert g == len(want_first) and w == 16 and lib.nwa_table_collided(ctx) == 0
    rows = np.full((g, 2, w), 0xEE, np.uint8)
    cols, res = np.full(g, -5, np.int32), np.full((g, 4), -5, np.int32)
    first, count = np.full(g, -5, np.int64), np.full(g, -5, np.int64)
    assert lib.nwa_table_fetch(ctx, _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(first), _lib.ptr(count), _lib.ptr(res)) == 0
    assert np.array_equal(first, want_first) and np.array_equal(count, want_count)
    assert np.all(cols == 16) and np.array_equal(res, rr[want_first])
    assert np.array_equal(rows, want_rows), np.flatnonzero((rows != want_rows).any(axis=(1, 2)))[:10]
