"""A BAM's region reads to the summary inside HBM (NWR_PACKED of include/crispr_regions.h,
crispresso_amd.regions.summarize_regions): the packed batch against the library's host packer on
the unflagged call's text, at the edges of the dword packer and across chunks; the refusals; the
adoption against an upload of the same reads and against the CPU oracle; the summary against the
host path and the CPU oracles.  Everything exact."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest

from crispresso_amd import _lib, demux, quantify, regions, synth
from crispresso_amd.aligner import pack_2bit
from crispresso_amd.pooled import align_pooled
from tests import demux_pack_model as dpm
from tests import regions_cases as rc
from tests import regions_model as rm
from tests import regions_summary_cases as sc
from tests.helpers import oracle_batch, runs_from_rows
from tests.test_gpu_summary import OPTS, SCORE, host_slots, oracle_slots

pytestmark = pytest.mark.gpu
INDEX_ARRAYS = ("region_offsets", "src", "st", "en", "text_offsets", "n_reads")


@pytest.fixture(scope="module")
def extractor():
    with regions.GpuRegionExtractor(0) as x:
        yield x


def bam_of(refs, records, cuts=None):
    return regions.read_bam(rc.bgzf(rc.bam_plain(refs, records), cuts))


def run(x, bam, regs, mode, packed, eqx=False, min_reads=0):
    if mode == "by_reference":
        return (regions.demux_by_reference_resident if packed else regions.demux_by_reference)(bam, extractor=x)
    if mode == "discover":
        return (regions.discover_regions_resident if packed else regions.discover_regions)(bam, min_reads, eqx, extractor=x)
    return (regions.extract_regions_resident if packed else regions.extract_regions)(bam, regs, eqx, extractor=x)


def packed_arrays(res):
    """Everything a packed result holds, for comparisons between calls."""
    return [np.asarray(getattr(res, f)) for f in INDEX_ARRAYS] + [res.lens, res.region_exc, *res.fetch_packed(),
                                                                 np.array([res.n_exc, res.n_no_seq])]


def check_packed(plain, res, decode=True):
    """A packed result against the unflagged call: the index arrays are identical, the batch is
    nw_pack_reads of the unflagged text, whole and sliced per region."""
    assert isinstance(res, regions.ResidentRegionReads) and res.text is None and res.qual is None
    for f in INDEX_ARRAYS:
        assert np.array_equal(getattr(res, f), getattr(plain, f)), f
    assert res.n_no_seq == plain.n_no_seq and res.target_names == plain.target_names
    assert res.by_reference == plain.by_reference
    host = pack_2bit(np.ascontiguousarray(plain.text), plain.text_offsets, nthreads=2)
    packed, pos, byt = res.fetch_packed()
    nbytes = (len(plain.text) + 3) // 4
    assert packed.dtype == np.uint8 and len(packed) == nbytes and np.array_equal(packed, host.packed[:nbytes])
    assert pos.dtype == np.int64 and np.array_equal(pos, host.exc_pos) and np.array_equal(byt, host.exc_byte)
    assert res.n_exc == len(host.exc_pos)
    assert res.lens.dtype == np.uint16 and np.array_equal(res.lens, np.diff(plain.text_offsets))
    starts = plain.text_offsets[plain.region_offsets]
    assert res.region_exc.dtype == np.int64
    assert np.array_equal(res.region_exc, np.searchsorted(host.exc_pos, starts, side="left"))
    if decode:          # region by region, as the adoption sees its slice of the stream
        for g in range(len(plain)):
            a, b = int(plain.region_offsets[g]), int(plain.region_offsets[g + 1])
            if a == b:
                continue
            e0, e1 = int(res.region_exc[g]), int(res.region_exc[g + 1])
            buf, off = plain.reads(g)
            got = dpm.decode_slice(packed, pos[e0:e1], byt[e0:e1], plain.text_offsets[a:b + 1])
            assert got == [buf[off[k]:off[k + 1]].tobytes() for k in range(b - a)], g
            mine = pack_2bit(np.ascontiguousarray(buf), np.ascontiguousarray(off), nthreads=1)
            assert np.array_equal(mine.exc_byte, byt[e0:e1]) and np.array_equal(mine.exc_pos, pos[e0:e1] - starts[g])
    assert res.names(0) == plain.names(0) if len(plain) else True
    return packed, pos, byt


# ---- packed equals the host packer ---------------------------------------------------------------

TOO_LONG = [(1, 1, 70000), (1, 2, 69999)]          # slice_edges' two hits of more than 65535 bases


def slice_edges_that_fit():
    refs, records, regs = rc.slice_edges()
    return refs, records, [r for r in regs if r not in TOO_LONG]


CASES = {
    "cigar_edges": (rc.cigar_edges, "regions", True),
    "cigar_edges_eqx": (rc.cigar_edges, "regions_eqx", True),
    "slice_edges": (slice_edges_that_fit, "regions", True),
    "record_filter": (rc.record_filter, "regions", True),
    "many_regions_one_record": (rc.many_regions_one_record, "regions", True),
    "many_records_one_region": (rc.many_records_one_region, "regions", False),
    "random_case": (rc.random_case, "regions", True),
    "table_past_lds": (lambda: rc.table_past_lds(1000), "regions", False),
    "demux_case": (lambda: rc.demux_case() + (None,), "by_reference", True),
    "discover": (lambda: rc.random_case(500, 1)[:2] + (None,), "discover", True),
    "discover_min_reads": (lambda: rc.random_case(500, 1, n_ref=1, span=12)[:2] + (None,), "discover_3", True),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_packed_equals_the_host_packer(extractor, name):
    make, mode, decode = CASES[name]
    refs, records, regs = make()
    bam = bam_of(refs, records, [777])
    kw = dict(eqx=mode.endswith("_eqx"), min_reads=3 if mode == "discover_3" else 0)
    mode = mode.split("_")[0] if not mode.startswith("by_") else mode
    plain = run(extractor, bam, regs, mode, False, **kw)
    with run(extractor, bam, regs, mode, True, **kw) as res:
        check_packed(plain, res, decode)
        assert len(plain.text) > 50 and res.pack_ms > 0
        if mode == "discover":
            assert res.regions == plain.regions and np.array_equal(res.n_records, plain.n_records)
            assert (res.n_aligned, res.n_kept, res.n_emitted) == (plain.n_aligned, plain.n_kept, plain.n_emitted)
            if kw["min_reads"]:
                assert 0 < res.n_emitted < len(res)
        with pytest.raises(regions.RegionsError, match="resident"):
            res.reads(0)
        with pytest.raises(regions.RegionsError, match="resident"):
            res.fastq_bytes(0)
    assert res.closed
    with pytest.raises(regions.RegionsError, match="released"):
        res.fetch_packed()


def test_a_result_outlives_its_context_and_the_next_call():
    refs, records, regs = rc.random_case(200, 20)
    bam = bam_of(refs, records)
    with regions.GpuRegionExtractor(0) as x:
        plain = run(x, bam, regs, "regions", False)
        first = run(x, bam, regs, "regions", True)
        other = run(x, bam, regs[:5], "regions", True)          # the context runs on while `first` lives
        want = packed_arrays(first)
        other.close()
    check_packed(plain, first)                                   # after nwr_destroy
    assert all(np.array_equal(a, b) for a, b in zip(packed_arrays(first), want))
    first.close()
    first.close()


# ---- the edge panel -------------------------------------------------------------------------------

LENS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 257)
OTHERS = "=MRSVWYHKDBN"


def mixed(n, seed):
    """n letters, about one in ten not a base."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return "".join(OTHERS[int(x) % 12] if x >= 36 else "ACGT"[int(x) % 4] for x in rng.integers(0, 40, n))


def edge_panel(tail):
    """Hits of every length in LENS from even and odd st, 17 regions of 17 bases (a region's first
    base on each position of a dword), a record of all 16 codes, 40 exceptions in a row over final
    positions 4080 .. 4119 (a dword edge and the edge of a block's 4096 positions), a region of
    empty hits alone, a region without hits between two with hits, and a last dword with `tail`
    bases."""
    refs = [("c0", 100000), ("c1", 1000)]
    records = [rc.rec("big", 0, 100, "4081M"),
               rc.rec("nrun", 0, 5000, "61M", seq=(OTHERS * 4)[:40] + "ACGT" * 5 + "A"),
               rc.rec("nrun2", 0, 5005, "30M", seq=mixed(30, 1)),
               rc.rec("all16", 0, 6000, "33M", seq=rc.NIBBLES * 2 + "A")]
    regs = [(0, 100, 4180), (0, 5000, 5060), (0, 5010, 5010), (0, 9000, 9010), (0, 6000, 6032), (0, 6001, 6032)]
    for i, L in enumerate(LENS):
        for par in (0, 1):
            p, st = 10000 + 400 * (2 * i + par), par + 2 * (i % 5)
            records.append(rc.rec("len%d_%d" % (L, par), 0, p, "300M", seq=mixed(300, 10 + 2 * i + par)))
            regs.append((0, p + st, p + st + L))
    for j in range(17):
        records.append(rc.rec("phase%d" % j, 0, 30000 + 400 * j, "20M", seq=mixed(20, 100 + j)))
        regs.append((0, 30000 + 400 * j, 30000 + 400 * j + 17))
    records.append(rc.rec("tail", 0, 50000, "20M", seq=mixed(20, 5)))
    total = sum(len(h[3]) for hits in rm.extract(records, regs)["hits"] for h in hits)
    regs.append((0, 50000, 50000 + (tail - total) % 16 + (16 if (tail - total) % 16 == 0 else 0)))
    return refs, records, regs


@pytest.mark.parametrize("tail", [1, 15])
def test_edge_panel(extractor, tail):
    refs, records, regs = edge_panel(tail)
    bam = bam_of(refs, records)
    plain = run(extractor, bam, regs, "regions", False)
    assert not rc.mismatches(rc.got_hits(plain), rm.extract(records, regs))
    with run(extractor, bam, regs, "regions", True) as res:
        packed, pos, byt = check_packed(plain, res)
    lens, off = np.diff(plain.text_offsets), plain.text_offsets
    assert len(plain.text) % 16 == tail and set(LENS) <= set(lens.tolist()) and lens[0] == 4080
    by_len = {(int(n), int(s) & 1) for n, s in zip(lens, plain.st)}
    assert {(L, par) for L in LENS for par in (0, 1)} <= by_len
    starts = off[plain.region_offsets[:-1]][plain.n_reads > 0]
    assert set((starts % 16).tolist()) == set(range(16))
    assert plain.n_reads[2] == 2 and lens[1 + 1:1 + 3].tolist() == [0, 0] and plain.n_reads[3] == 0
    assert pos[:40].tolist() == list(range(4080, 4120)) and byt[:40].tobytes() == (OTHERS * 4)[:40].encode()
    assert res.region_exc[:5].tolist() == [0, 0, 40, 40, 40]
    a = int(plain.text_offsets[plain.region_offsets[4]])
    assert plain.text[a:a + 16].tobytes() == rc.NIBBLES.encode() and set(byt.tolist()) == set(OTHERS.encode())


# ---- chunks and determinism -------------------------------------------------------------------

def chunk_cases():
    refs, records, regs = rc.random_case(500, 40)
    yield refs, records, regs, "regions"
    yield (*edge_panel(15), "regions")
    yield refs, records, None, "discover"
    yield refs, records, None, "by_reference"


@pytest.mark.parametrize("chunk", [1, 2, 7, 64])
def test_chunks(extractor, chunk, monkeypatch):
    """With one record a chunk every boundary between two hits of a region is a chunk boundary:
    partial dwords from different sweeps meet in one word of the stream."""
    one = []
    for refs, records, regs, mode in chunk_cases():
        bam = bam_of(refs, records)
        with run(extractor, bam, regs, mode, True) as res:
            one.append((bam, regs, mode, packed_arrays(res)))
    monkeypatch.setenv("CRISPR_NWR_CHUNK", str(chunk))
    with regions.GpuRegionExtractor(0) as x:
        for bam, regs, mode, want in one:
            with run(x, bam, regs, mode, True) as res:
                got = packed_arrays(res)
            assert len(got) == len(want)
            for k, (a, b) in enumerate(zip(got, want)):
                assert np.array_equal(a, b), (mode, k)
            assert len(want[-4]) > 100


def test_determinism(extractor):
    refs, records, regs = edge_panel(1)
    bam = bam_of(refs, records)
    runs = []
    for _ in range(3):
        with run(extractor, bam, regs, "regions", True) as res:
            runs.append(packed_arrays(res))
    for other in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], other))
    assert runs[0][-2].size > 40


# ---- refusals ------------------------------------------------------------------------------------

def test_refusals(extractor, gpu_aligner_factory):
    lib = extractor._lib
    refs, records, regs = rc.many_regions_one_record()
    regs = regs + [(1, 5, 6)]                                   # a region without hits
    bam = bam_of(refs, records)

    def good():
        plain = run(extractor, bam, regs, "regions", False)
        with run(extractor, bam, regs, "regions", True) as res:
            check_packed(plain, res, decode=False)
        return plain

    plain = good()
    al = gpu_aligner_factory()
    # an unknown flag is still refused
    bad = _lib.NwrResult()
    table, _ = regions.region_table(bam, regs)
    assert lib.nwr_extract(extractor._ctx, bam._h, _lib.ptr(table), len(table), 8, ctypes.byref(bad)) == _lib.NW_E_INVALID
    assert lib.nwr_discover(extractor._ctx, bam._h, 1 | _lib.NWR_PACKED, 0, ctypes.byref(bad)) == _lib.NW_E_INVALID
    # text or qualities of a packed result
    with run(extractor, bam, regs, "regions", True) as res:
        text = np.zeros(int(res.text_offsets[-1]), np.uint8)
        none = [None] * 5
        assert lib.nwr_fetch(ctypes.byref(res._res), *none, _lib.ptr(text), None) == _lib.NW_E_STATE
        assert lib.nwr_fetch(ctypes.byref(res._res), *none, None, _lib.ptr(text)) == _lib.NW_E_STATE
        assert not text.any()
        src = np.zeros(len(res.src), np.int64)
        assert lib.nwr_fetch(ctypes.byref(res._res), None, _lib.ptr(src), None, None, None, None, None) == 0
        assert np.array_equal(src, plain.src)
        # a short capacity
        need = ctypes.c_int64()
        small = np.zeros(4, np.uint8)
        assert lib.nwr_fetch_packed(ctypes.byref(res._res), _lib.ptr(small), 4, None, None, ctypes.byref(need)) \
            == _lib.NW_E_CAPACITY
        assert need.value == (int(res.text_offsets[-1]) + 3) // 4 and not small.any()
        # adoption: no reference, rows output, out of range, a hitless region, another result's state untouched
        with pytest.raises(regions.RegionsError) as exc:
            res.adopt(al, 0)
        assert exc.value.code == _lib.NW_E_STATE
        al.set_reference("ACGT" * 30)
        with pytest.raises(regions.RegionsError) as exc:      # rows output
            res.adopt(al, 0)
        assert exc.value.code == _lib.NW_E_STATE
        al.set_output("ops")
        for g in (-1, len(regs), len(regs) - 1):
            with pytest.raises(regions.RegionsError) as exc:
                res.adopt(al, g)
            assert exc.value.code == _lib.NW_E_INVALID
        assert res.n_reads[len(regs) - 1] == 0
        assert lib.nwr_adopt_region(ctypes.byref(res._res), None, 0) == _lib.NW_E_INVALID
        n = res.adopt(al, 3)                                     # and then a good one
        al.run_async()
        al.sync()
        assert len(al.download_ops(n)) == n == int(res.n_reads[3]) > 0
        al.set_output("rows")
    # the packed entry points on an unpacked result
    res0 = _lib.NwrResult()
    assert lib.nwr_extract(extractor._ctx, bam._h, _lib.ptr(table), len(table), 0, ctypes.byref(res0)) == 0
    try:
        assert lib.nwr_packed_info(ctypes.byref(res0), None, None, None, None) == _lib.NW_E_STATE
        assert lib.nwr_fetch_packed(ctypes.byref(res0), None, 0, None, None, None) == _lib.NW_E_STATE
        al.set_output("ops")
        assert lib.nwr_adopt_region(ctypes.byref(res0), al._h, 0) == _lib.NW_E_STATE
        al.set_output("rows")
    finally:
        lib.nwr_release(ctypes.byref(res0))
    good()


def test_a_read_of_65536_bases_is_refused(extractor):
    refs = [("long", 70000), ("short", 100)]
    records = [rc.rec("fits", 1, 1, "50M"), rc.rec("too_long", 0, 1, "65536M", seq="ACGT" * 16384,
                                                  qual=[30] * 65536)]
    bam = bam_of(refs, records)
    with pytest.raises(regions.RegionsError, match="record 1 .*65536 bases") as exc:
        regions.demux_by_reference_resident(bam, extractor=extractor)
    assert exc.value.code == _lib.NW_E_UNSUPPORTED
    plain = regions.demux_by_reference(bam, extractor=extractor)     # the same records unflagged still work
    assert plain.n_reads.tolist() == [1, 1] and len(plain.text) == 65536 + 50
    # slice_edges' hits of 69,999 and 69,997 bases are refused likewise; one base fewer than 65536 is taken
    refs2, records2, regs2 = rc.slice_edges()
    with pytest.raises(regions.RegionsError) as exc:
        regions.extract_regions_resident(bam_of(refs2, records2), regs2, extractor=extractor)
    assert exc.value.code == _lib.NW_E_UNSUPPORTED and "record 3" in str(exc.value)
    records[1] = rc.rec("just_fits", 0, 1, "65535M", seq=("ACGTN" * 13107), qual=[30] * 65535)
    bam = bam_of(refs, records)
    with regions.demux_by_reference_resident(bam, extractor=extractor) as res:
        check_packed(regions.demux_by_reference(bam, extractor=extractor), res, decode=False)
        assert res.lens.tolist() == [65535, 50] and res.n_exc == 13107


# ---- adoption equals upload ---------------------------------------------------------------------

def pooled_case():
    """tests/test_gpu_regions.py's shape: 3 amplicons laid on one reference; reads that span them
    with soft clips, an insertion, a deletion, and an N in every fifth."""
    amps = [synth.random_amplicon(n, seed) for n, seed in ((150, 1), (180, 2), (201, 3))]
    genome = "".join("T" * 50 + a for a in amps) + "T" * 50
    starts = [genome.index(a) + 1 for a in amps]
    refs = [("chrA", len(genome)), ("chrB", 1000)]
    records = []
    for g, (a, s) in enumerate(zip(amps, starts)):
        for k in range(20):
            lead, tail = 5 + k % 7, 3 + k % 5
            body = genome[s - 1 - lead:s - 1 + len(a) + tail]
            if k % 5 == 0:
                body = body[:lead + 30 + k] + "N" + body[lead + 31 + k:]
            if k % 4 == 1:
                at = lead + 60 + k
                seq, cigar = body[:at] + body[at + 3:], "%dM3D%dM" % (at, len(body) - at - 3)
            elif k % 4 == 2:
                at = lead + 40 + k
                seq, cigar = body[:at] + "GG" + body[at:], "%dM2I%dM" % (at, len(body) - at)
            else:
                seq, cigar = "AC" + body, "2S%dM" % len(body)
            records.append(rc.rec("a%d_%d" % (g, k), 0, s - lead, cigar, seq=seq))
    records.append(rc.rec("elsewhere", 1, starts[0], "200M"))
    regs = [("chrA", s, s + len(a), "amp%d" % g) for g, (a, s) in enumerate(zip(amps, starts))]
    return amps, refs, records, regs


def uploaded(al, amp, buf, off):
    """The ops of the same reads through nw_batch_upload_packed."""
    al.set_reference(amp)
    al.upload_packed(pack_2bit(np.ascontiguousarray(buf), np.ascontiguousarray(off), nthreads=1))
    al.run_async()
    al.sync()
    return al.download_ops(len(off) - 1)


def same_ops(a, b):
    return (np.array_equal(a.stats, b.stats) and np.array_equal(a.ops, b.ops) and np.array_equal(a.ops_off, b.ops_off)
            and np.array_equal(a.read_lens, b.read_lens))


def test_adoption_equals_upload(extractor, gpu_aligner_factory):
    amps, refs, records, regs = pooled_case()
    bam = bam_of(refs, records, [5000])
    plain = regions.extract_regions(bam, regs, extractor=extractor)
    assert plain.n_reads.tolist() == [20, 20, 20] and (plain.text == ord("N")).sum() == 12
    al = gpu_aligner_factory()
    want = [uploaded(al, amps[g], *plain.reads(g)) for g in range(3)]
    with regions.extract_regions_resident(bam, regs, extractor=extractor) as res:
        check_packed(plain, res)
        al.set_output("ops")
        for g in (2, 0, 1, 0):
            al.set_reference(amps[g])
            n = res.adopt(al, g)
            al.run_async()
            al.sync()
            assert n == 20 and same_ops(al.download_ops(n), want[g]), g
        al.set_output("rows")
        seen = []
        obs, skipped = regions.align_regions_resident(res, amps, al, on_group=lambda g, a, n: seen.append((g, n)))
        assert al.output_mode == "rows" and skipped == [] and seen == [(0, 20), (1, 20), (2, 20)]
        obs2, skipped2 = regions.align_regions_resident(res, amps, al, min_reads=21)
        assert skipped2 == [0, 1, 2] and obs2 == [None] * 3
    for g in range(3):
        assert same_ops(obs[g], want[g])
        buf, off = plain.reads(g)
        rows = obs[g].expand(amps[g], np.ascontiguousarray(buf), np.ascontiguousarray(off))
        oracle = oracle_batch(amps[g], np.ascontiguousarray(buf), np.ascontiguousarray(off))
        for f in ("aln_len", "n_ident", "n_sim", "n_gaps", "score", "end_i", "end_j"):
            assert np.array_equal(rows.stats[f], oracle.stats[f]), (g, f)
        for i in range(20):
            L = int(oracle.stats["aln_len"][i])
            assert np.array_equal(rows.aln[i, :, :L], oracle.aln[i, :, :L]), (g, i)
            assert obs[g].ops[obs[g].ops_off[i]:obs[g].ops_off[i + 1]].tolist() == \
                runs_from_rows(oracle.aln[i, 0, :L].tobytes(), oracle.aln[i, 2, :L].tobytes())
        assert int(rows.stats["n_ident"].min()) >= len(amps[g]) - 5


def test_a_region_of_empty_reads_is_adoptable(extractor, gpu_aligner_factory):
    refs, records, regs = edge_panel(15)
    bam = bam_of(refs, records)
    plain = regions.extract_regions(bam, regs, extractor=extractor)
    al = gpu_aligner_factory()
    amp = synth.random_amplicon(60, 9)
    buf, off = plain.reads(2)
    assert off.tolist() == [0, 0, 0]
    want = uploaded(al, amp, buf, off)
    assert (want.stats["flags"] & _lib.NW_FLAG_EMPTY).all() and len(want) == 2
    others = {g: uploaded(al, amp, *plain.reads(g)) for g in (1, 4)}
    with regions.extract_regions_resident(bam, regs, extractor=extractor) as res:
        al.set_output("ops")
        for g in (2, 1, 4, 2):                                   # its neighbours too, exceptions included
            al.set_reference(amp)
            n = res.adopt(al, g)
            al.run_async()
            al.sync()
            assert same_ops(al.download_ops(n), want if g == 2 else others[g]), g
        al.set_output("rows")


# ---- the summary ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wgs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wgs")
    bam_path, table, fasta = sc.write_inputs(tmp)
    rows = regions.wgs_rows(regions.read_wgs_region_file(table), fasta)
    slots = sc.oracle_check(rows, oracle_slots)      # the choice of inputs, before any GPU call
    return tmp, bam_path, table, fasta, rows, slots


def reads_of(plain, g):
    buf, off = plain.reads(g)
    return [buf[off[k]:off[k + 1]].tobytes() for k in range(len(off) - 1)]


def check_frame(frame, names, n_reads, counts, skipped):
    assert list(frame.columns) == list(demux.SUMMARY_COLUMNS) and frame["Name"].tolist() == names
    assert frame["Reads_total"].tolist() == n_reads
    for g in range(len(names)):
        if g in skipped or counts[g][1] == 0:
            assert frame.iloc[g][1:6].isna().all()
        else:
            s, total = counts[g], float(counts[g][1])
            assert frame.iloc[g][1:6].tolist() == [s[2] / total * 100., s[3] / total * 100., s[4] / total * 100.,
                                                  s[5] / total * 100., total]


def test_summarize_regions_equals_the_host_path_and_the_oracles(extractor, gpu_aligner_factory, wgs):
    tmp, bam_path, table, fasta, rows, slots = wgs
    _, amps, raw = sc.genome()
    assert [r["Amplicon_Sequence"] for r in rows] == amps and [r["Name"] for r in rows] == ["region_%d" % g for g in range(4)]
    assert rows[0]["sgRNA"] == raw[0]["sgRNA"] and rows[1]["sgRNA"] == "" and raw[1]["sgRNA"]
    bam = regions.read_bam(bam_path)
    targets = [(r["chr_id"], r["bpstart"], r["bpend"], r["Name"]) for r in rows]
    plain = regions.extract_regions(bam, targets, extractor=extractor)
    assert plain.n_reads.tolist() == list(sc.N_RECORDS)
    assert [reads_of(plain, g) for g in range(4)] == sc.model_reads()
    al = gpu_aligner_factory()
    batches = align_pooled(amps[:3], [plain.reads(g) for g in range(3)], al)
    with quantify.GpuQuantifier(0) as gq:
        host = {g: host_slots(batches[g], rows[g], gq) for g in range(3)}
    seen = []
    with regions.extract_regions_resident(bam, targets, extractor=extractor) as res:
        rs = regions.summarize_regions(rows, res, al, min_reads=sc.MIN_READS, min_identity_score=SCORE,
                                       on_group=lambda g, a, n: seen.append((g, n)), **OPTS)
        again = regions.summarize_regions(rows, res, al, min_reads=sc.MIN_READS, min_identity_score=SCORE, **OPTS)
        at_six = regions.summarize_regions(rows, res, al, min_reads=6, **OPTS)      # >=, not Pooled's >
        with pytest.raises(ValueError, match="Expected_HDR"):
            regions.summarize_regions([dict(rows[0], Expected_HDR="ACGT")] + rows[1:], res, al)
    assert al.output_mode == "rows" and rs.skipped == [3] and rs.counts.dtype == np.int64 and rs.counts.shape == (4, 16)
    assert seen == [(g, sc.N_RECORDS[g]) for g in range(3)]
    for g in range(3):
        assert rs.counts[g].tolist() == host[g], g
        assert rs.counts[g].tolist() == slots[g], g
    assert not rs.counts[3].any() and rs.kernel_ms["summary"] > 0 and rs.kernel_ms["flags"] > 0
    check_frame(rs.frame, [r["Name"] for r in rows], list(sc.N_RECORDS), rs.counts, rs.skipped)
    assert rs.frame.iloc[3][1:6].isna().all() and rs.frame["Reads_total"][3] == 6
    assert np.array_equal(again.counts, rs.counts)
    pd.testing.assert_frame_equal(again.frame, rs.frame)
    assert at_six.skipped == [] and at_six.counts[3, 0] == 6 and np.array_equal(at_six.counts[:3], rs.counts[:3])
    with pytest.raises(ValueError, match="released"):
        regions.summarize_regions(rows, res, al)
    # a row without a sequence is not analysed and reports no reads
    with regions.extract_regions_resident(bam, targets, extractor=extractor) as res:
        blank = regions.summarize_regions([dict(rows[0], Amplicon_Sequence="")] + rows[1:], res, al,
                                          min_reads=sc.MIN_READS, **OPTS)
    assert blank.skipped == [0, 3] and blank.frame["Reads_total"].tolist() == [0] + list(sc.N_RECORDS[1:])
    assert np.array_equal(blank.counts[1:], rs.counts[1:])
    # the command line writes the same table
    out = str(tmp / "cli")
    assert regions.main(["--bam", bam_path, "--regions", table, "--genome", fasta, "--summary", "--out", out]) == 0
    want = str(tmp / "want.txt")
    demux.write_summary(want, rs.frame)
    got = open(os.path.join(out, "SAMPLES_QUANTIFICATION_SUMMARY.txt"), "rb").read()
    assert got == open(want, "rb").read() and got.count(b"\n") == 5 and b"NA" in got
    assert os.listdir(out) == ["SAMPLES_QUANTIFICATION_SUMMARY.txt"]


def test_summarize_discovered_regions(extractor, gpu_aligner_factory, wgs):
    tmp, bam_path, table, fasta, _, _ = wgs
    bam = regions.read_bam(bam_path)
    plain = regions.discover_regions(bam, 3, extractor=extractor)
    keep = [g for g in range(len(plain)) if plain.n_reads[g] >= 3]
    assert 20 < len(keep) < len(plain) and plain.n_emitted == len(keep)
    al = gpu_aligner_factory()
    with regions.discover_regions_resident(bam, 3, extractor=extractor) as res:
        rows = regions.discovered_rows(res, fasta)
        assert [r["Name"] for r in rows] == plain.target_names and rows == regions.discovered_rows(plain, fasta)
        rs = regions.summarize_regions(rows, res, al, min_reads=3, min_identity_score=SCORE, **OPTS)
    assert rs.skipped == [g for g in range(len(plain)) if g not in keep]
    amps = [rows[g]["Amplicon_Sequence"] for g in keep]
    assert all(amps) and all(len(a) == e - s for a, (_, s, e) in zip(amps, (plain.regions[g] for g in keep)))
    batches = align_pooled(amps, [plain.reads(g) for g in keep], al)
    with quantify.GpuQuantifier(0) as gq:
        for b, g in zip(batches, keep):
            assert rs.counts[g].tolist() == host_slots(b, rows[g], gq), g
            assert rs.counts[g].tolist() == oracle_slots(rows[g], reads_of(plain, g)), g
    assert rs.counts[:, 1].sum() > 50 and rs.counts[:, 3].sum() > 10 and not rs.counts[:, 15].any()
    check_frame(rs.frame, plain.target_names, plain.n_reads.tolist(), rs.counts, rs.skipped)
    out = str(tmp / "cli_discover")
    assert regions.main(["--bam", bam_path, "--discover", "--min-reads", "3", "--genome", fasta, "--summary",
                         "--out", out]) == 0
    want = str(tmp / "want_discover.txt")
    demux.write_summary(want, rs.frame)
    assert open(os.path.join(out, "SAMPLES_QUANTIFICATION_SUMMARY.txt"), "rb").read() == open(want, "rb").read()
