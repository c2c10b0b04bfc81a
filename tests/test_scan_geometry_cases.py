"""The inputs of tests/test_gpu_scan_geometry.py are what they claim (tests/scan_geometry_cases.py):
every scan block sees more than 1,024 block sums with the intended sums per thread, a share that
sums to 0, a clamped share, sums that differ from their neighbours; and every assembled
expectation equals the slow model run outright on a prefix and on a window that straddles item
262,144.  No GPU: these are conditions on the inputs, met by the models alone."""
import numpy as np
import pytest

from crispresso_amd import alleles
from crispresso_amd.aligner import pack_2bit
from tests import alleles_cases as ac
from tests import demux_model as dm
from tests import front_model as fm
from tests import genome_regions_model as gm
from tests import regions_cases as rc
from tests import regions_model as rm
from tests import scan_geometry_cases as sg
from tests.alleles_cases import pack

PREFIX = 5000
HALF = 2500


def check_scan(sums, per, partial):
    """The conditions every scan's input meets, the last working thread's share cut to ``partial``
    blocks (``per`` where the issue's size leaves it whole); returns (lo, hi, share sums)."""
    sums = np.asarray(sums)
    assert len(sums) > sg.SCAN_THREADS
    got, lo, hi, share = sg.shares(sums)
    assert got == per and per > 1
    working = hi > lo
    assert np.any(share[working] == 0), "no scan thread's share sums to 0"
    cut = (lo < len(sums)) & (len(sums) < lo + per)      # hi = min(blocks, lo + per) cuts a share that holds blocks
    assert np.any(cut) == (partial < per), "no share is clamped"
    assert int((hi - lo)[working][-1]) == partial
    assert lo[np.flatnonzero(working)[-1] + 1] == len(sums)          # the thread after it starts at `blocks`
    assert np.mean(sums[1:] != sums[:-1]) >= 0.5
    return lo, hi, share


def windows(n, straddle=sg.STRADDLE):
    """The prefix and the window around item 262,144 (the first of block 1,024; cut to the batch)."""
    assert HALF < straddle < n
    return [(0, min(n, PREFIX)), (straddle - HALF, min(n, straddle + HALF))]


# ---- 1. the front packer --------------------------------------------------------------------

FRONT_GEOMETRY = {"se_1025": (1025, 2, 1), "se_2049": (2049, 3, 3), "se_2050": (2050, 3, 1), "pe_1025": (1025, 2, 1)}


def test_front_pools():
    se, pe = sg.front_pool(True), sg.front_pool(False)
    lens = se.inputs[0].lens
    assert lens.min() == 1 and lens.max() == 40 and len(set(p[:2] for p in se.pairs)) == len(se.pairs)
    odd = sum(1 for p in se.pairs if p[0].translate(None, b"ACGT"))
    assert 0.05 * len(se.pairs) <= odd <= 0.2 * len(se.pairs)
    assert set(se.status.tolist()) == {fm.FILTERED, fm.TRIMMED, fm.COMBINED}
    assert len(pe.pairs) >= 1500 and set(pe.status.tolist()) == {0, 1, 2, 3, 4}
    assert int(np.sum(pe.status == fm.COMBINED_OUTIE)) >= 10 and int(np.sum(pe.status == fm.NOT_COMBINED)) >= 100
    assert any(r.translate(None, b"ACGTacgt") for r in pe.merged.items)         # survivors with exceptions
    assert set(pe.trim_class.tolist()) == {-1, 0, 1, 2, 3}


@pytest.mark.parametrize("name", sorted(sg.FRONT_SIZES))
def test_front_geometry(name):
    pool, pick, e, single_end = sg.front_case(name)
    n, m = len(pick), len(e.src)
    blocks, per, partial = FRONT_GEOMETRY[name]
    assert n == sg.FRONT_SIZES[name] and (n + sg.FRONT_BLOCK - 1) // sg.FRONT_BLOCK == blocks
    assert (m % sg.LEN_GROUP == 0) == (name == "se_1025") and m > 0
    alive = pool.status[pick] >= fm.COMBINED
    mid = np.flatnonzero(~alive[sg.DEAD_RUN:n - sg.DEAD_RUN])
    runs = np.split(mid, np.flatnonzero(np.diff(mid) != 1) + 1)
    assert not alive[:1000].any() and not alive[-1000:].any() and max(map(len, runs)) >= 1000
    assert e.src[0] >= sg.FRONT_BLOCK                    # the first survivor is not in block 0
    for q, sums in enumerate(sg.front_block_sums(pool, pick, e)):
        lo, hi, share = check_scan(sums, per, partial)
        assert sums[0] == 0 and sums[-1] == 0 and share[0] == 0          # a whole share of nothing opens the scan
        zero = np.flatnonzero((share == 0) & (hi > lo))
        assert np.any((lo[zero] * sg.FRONT_BLOCK > sg.DEAD_RUN) & (hi[zero] * sg.FRONT_BLOCK < n - sg.DEAD_RUN))
        assert int(sums.sum()) == (m, int(e.offsets[-1]), len(e.packed.exc_pos))[q]
    assert len(e.packed.exc_pos) > 1000 and e.packed.exc_pos[-1] > e.offsets[m // 2]


@pytest.mark.parametrize("name", sorted(sg.FRONT_SIZES))
def test_front_assembly_is_the_model(name):
    pool, pick, e, single_end = sg.front_case(name)
    for a, b in windows(len(pick)):
        w = fm.expected([pool.pairs[p] for p in pick[a:b]], **sg.front_settings(single_end))
        j0, j1 = np.searchsorted(e.src, [a, b])
        t0, t1 = int(e.offsets[j0]), int(e.offsets[j1])
        assert np.array_equal(e.status[a:b], w.status) and np.array_equal(e.src[j0:j1] - a, w.src)
        assert np.array_equal(e.offsets[j0:j1 + 1] - t0, w.offsets) and np.array_equal(e.lens[j0:j1], w.lens)
        assert np.array_equal(e.buf[t0:t1], w.buf) and np.array_equal(e.qbuf[t0:t1], w.qbuf)
        x0, x1 = np.searchsorted(e.packed.exc_pos, [t0, t1])
        assert np.array_equal(e.packed.exc_pos[x0:x1] - t0, w.packed.exc_pos)
        assert np.array_equal(e.packed.exc_byte[x0:x1], w.packed.exc_byte)
        tc = pool.trim_class[pick[a:b]]
        assert {k: int(np.sum(tc == i)) for i, k in enumerate(("both", "fwd_only", "rev_only", "dropped"))} == w.trim
    # the inputs are the pool's reads in the order drawn
    args = sg.front_inputs(pool, pick[:300], single_end)
    want = fm.packed_inputs([pool.pairs[p] for p in pick[:300]], single_end)
    assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(args, want))


# ---- 2. the demux packer --------------------------------------------------------------------

@pytest.mark.parametrize("name,per,floor", [("per2", 2, 4194305), ("per3", 3, 8388609 + 77)])
def test_demux_geometry(name, per, floor):
    pool, pick, e = sg.demux_case(name)
    assert len(pool.reads) <= 2000 and 100 <= pool.inputs.lens.min() and pool.inputs.lens.max() <= 180
    assert set(pool.which.tolist()) >= set(range(6)) and (pool.which < 0).sum() >= 20
    assert all(set(pool.strand[pool.which == g].tolist()) == {0, 1} for g in range(6))
    total = int(e.text_offsets[-1])
    sums = sg.demux_block_sums(e)
    assert total >= floor and len(sums) == (total + sg.DEMUX_BLOCK - 1) // sg.DEMUX_BLOCK
    lo, hi, share = check_scan(sums, per, 1)
    assert sums[0] > 0 and sums[-1] > 0 and np.any(sums[sg.SCAN_THREADS:] > 0)
    assert e.exc_pos[0] == 7 and e.exc_pos[-1] == total - 1                   # the placed first and last read
    quiet = np.flatnonzero(sums == 0)
    assert max(map(len, np.split(quiet, np.flatnonzero(np.diff(quiet) != 1) + 1))) >= 3 * per
    starts = e.text_offsets[e.group_offsets[:-1]]
    g = sg.FIRST_EXC_GROUP
    assert e.exc_pos[e.group_exc[g]] == starts[g] and e.exc_byte[e.group_exc[g]] == ord("N")
    assert e.group_exc[sg.CLEAN_GROUP] == e.group_exc[sg.CLEAN_GROUP + 1]     # a group with none
    assert np.all(np.diff(e.group_offsets) > 1000) and np.any(e.which < 0)
    assert set(e.exc_byte.tolist()) >= set(b"NnRYKM-")


@pytest.mark.parametrize("name", sorted(sg.DEMUX_SIZES))
def test_demux_assembly_is_the_model(name):
    pool, pick, e = sg.demux_case(name)
    amps = list(sg.demux_amplicons())
    # the reads whose gathered bases lie around position 4,194,304, the first of block 1,024
    j = int(np.searchsorted(e.text_offsets, sg.SCAN_THREADS * sg.DEMUX_BLOCK))
    around = np.sort(e.order[j - 40:j + 40])
    assert e.text_offsets[j - 40] < sg.SCAN_THREADS * sg.DEMUX_BLOCK < e.text_offsets[j + 40]
    for a, b in [(0, PREFIX), (int(around[0]), int(around[-1]) + 1)]:
        assert 0 < b - a <= PREFIX
        reads = [pool.reads[p] for p in pick[a:b]]
        want = dm.demultiplex(amps, reads, k=sg.DEMUX_K, min_hits=sg.DEMUX_MIN_HITS)
        got = sg.demux_assemble(pool, pick[a:b])
        assert got.which.tolist() == want["which"] and got.strand.tolist() == want["strand"]
        assert got.order.tolist() == want["order"] and got.group_offsets.tolist() == want["group_offsets"]
        text, off = pack([r for grp in want["groups"] for r in grp])
        assert np.array_equal(got.text, text[:len(got.text)]) and np.array_equal(got.text_offsets, off)
        host = pack_2bit(text, off, nthreads=1)
        assert np.array_equal(got.exc_pos, host.exc_pos) and np.array_equal(got.exc_byte, host.exc_byte)
        assert np.array_equal(e.which[a:b], got.which) and np.array_equal(e.strand[a:b], got.strand)
        for g in range(len(amps)):       # the window's reads of a group lie together in the whole call's group
            mine = e.order[e.group_offsets[g]:e.group_offsets[g + 1]]
            mine = mine[(mine >= a) & (mine < b)] - a
            assert mine.tolist() == want["order"][want["group_offsets"][g]:want["group_offsets"][g + 1]]
    s, off = pool.inputs.take(pick[:200])
    ws, woff = pack([pool.reads[p] for p in pick[:200]])
    assert np.array_equal(s, ws[:len(s)]) and np.array_equal(off, woff)


# ---- 3. regions -----------------------------------------------------------------------------

def test_region_geometry():
    pool, pick = sg.region_case()
    want, major, packed, found = sg.region_expected()
    n = len(pick)
    assert n == sg.REGION_RECORDS >= 262145 + 77 and len(rc.record_bytes(sg.region_records(pool, pick[:1])[0])) * n < (256 << 20)   # one chunk
    total = int(major[1][-1])
    assert total > 8380416 and len(major[3]) >= 0.95 * n
    lens = np.diff(major[1])
    assert np.mean(lens >= 33) > 0.9 and pool.hit[pick].sum(axis=1).max() == 2
    cigars = "".join(r["cigar"] for r in pool.items)
    assert all(op in cigars for op in "SID") and {r["ref_id"] for r in pool.items} == {-1, 0, 1, 2}
    bases = "".join(r["seq"] for r in pool.items if r["seq"] != "*")
    assert 0.01 < sum(c not in "ACGT" for c in bases) / len(bases) < 0.03
    assert want["n_no_seq"] > 0 and any(r["flag"] & 4 for r in pool.items)
    sums = sg.region_block_sums(pool, pick, want, major, packed, found)
    assert {k: len(v) for k, v in sums.items()} == {"extract": 1025, "discover": 1025, "pack": 2680, "rank": 1341}
    per = {"extract": 2, "discover": 2, "pack": 3, "rank": 2}
    for what, s in sums.items():
        check_scan(s, per[what], 1)
        assert s[0] > 0 and np.any(s[sg.SCAN_THREADS:] > 0)                   # hits and exceptions in late blocks
    assert sums["rank"][-1] == 0 and sums["pack"][-1] > 0 and sums["extract"][-1] > 0
    assert int(sums["pack"].sum()) == int(sums["rank"].sum()) == len(packed.exc_pos) > 1000
    nohit = np.flatnonzero(pool.hit[pick].sum(axis=1) == 0)
    assert max(map(len, np.split(nohit, np.flatnonzero(np.diff(nohit) != 1) + 1))) >= 1000
    kept = sum(1 for h in found["hits"] if h)
    assert 0 < kept < len(found["regions"]) and found["n_no_seq"] > 0          # min_reads keeps some spans, drops others
    assert all((len(h) > 0) == (c >= sg.DISCOVER_MIN_READS) for h, c in zip(found["hits"], found["n_records"]))


def test_region_assembly_is_the_model():
    pool, pick = sg.region_case()
    want, major, packed, found = sg.region_expected()
    for a, b in windows(len(pick)):
        records = sg.region_records(pool, pick[a:b], base=a)
        assert sg.region_extract_assemble(pool, pick[a:b], base=a) == rm.extract(records, sg.REGION_TABLE)
        for min_reads in (0, 12):
            assert sg.region_discover_assemble(pool, pick[a:b], min_reads, base=a) == gm.discover(records, False, min_reads)
        assert sg.region_bam(pool, pick[a:b], base=a) == rc.bgzf(rc.bam_plain(sg.REGION_REFS, records), stored=True)
        for g, hits in enumerate(want["hits"]):          # the window's hits of a region, in the whole call's list
            mine = [h for h in hits if a <= h[0] < b]
            ref = rm.extract(records, sg.REGION_TABLE)["hits"][g]
            assert [(h[0] - a,) + h[1:5] for h in mine] == [h[:5] for h in ref]
    small = rm.extract(sg.region_records(pool, pick[:PREFIX]), sg.REGION_TABLE)
    text, off, roff, src, st, en = sg.region_major(small)
    assert text.tobytes() == b"".join(h[3] for g in small["hits"] for h in g) and roff[-1] == len(src) == len(off) - 1


# ---- 4. the allele grouper ------------------------------------------------------------------

@pytest.mark.parametrize("name,steps", [("two_steps", 2), ("three_steps", 3)])
def test_allele_geometry_and_groups(name, steps):
    pool, pick, keep = sg.allele_case(name)
    n = len(pick)
    tiles = (n + sg.TILE - 1) // sg.TILE
    assert n == sg.ALLELE_SIZES[name] and tiles > sg.TILES_PER_STEP
    assert (tiles + sg.TILES_PER_STEP - 1) // sg.TILES_PER_STEP == steps and tiles % sg.TILES_PER_STEP != 0     # a short last step
    assert 8 <= pool.lens.min() and pool.lens.max() <= 16 and len(set(pool.items)) == len(pool.items)
    assert 4500 <= len(pool.items) <= 5500               # about 5,000 sequences
    assert set(keep.tolist()) == {0, 1, 2} and not np.array_equal(keep[:n // 2], keep[n - n // 2:])
    buf, off = pool.take(pick)
    for k in (None, keep):
        first, count, gor = sg.allele_groups(pick, k)
        sums = sg.allele_tile_sums(first, n)
        assert len(sums) == tiles and np.mean(sums[1:] != sums[:-1]) >= 0.5
        quiet = np.flatnonzero(sums == 0)
        assert k is not None or set(range(*sg.QUIET_TILES)) <= set(quiet.tolist())
        assert len(quiet) >= 3 and sums[0] > 0 and sums[-1] == 1 and first[-1] == n - 1      # tile_off of the last tile is used
        late = int(np.sum(first >= sg.TILES_PER_STEP * sg.TILE))
        assert late >= (len(first) // 3 if steps == 3 else 1)
        assert np.all(np.diff(first) > 0) and int(count.sum()) == (n if k is None else int(np.count_nonzero(k)))
        host = alleles.group_reads_host(buf, off, keep=k, want_group_of_read=True)
        assert np.array_equal(host.first, first) and np.array_equal(host.count, count)
        assert np.array_equal(host.group_of_read, gor)
    for a, b in windows(n, sg.TILES_PER_STEP * sg.TILE):     # (around the first read of tile 1,024)
        reads = [pool.items[p] for p in pick[a:b]]
        for k in (None, keep[a:b]):
            first, count, gor = sg.allele_groups(pick[a:b], k)
            assert (first.tolist(), count.tolist(), gor.tolist()) == ac.expected_groups(reads, k)


def test_allele_table_rows_are_the_host_rows():
    """The rows of the table call for a few thousand reads: nw_expand_ops_subset on the groups'
    first reads, as tests/resident_alleles_cases.host_table does it."""
    from crispresso_amd import _lib

    pool, pick, keep = sg.allele_case("two_steps")
    pick, keep = pick[:PREFIX], keep[:PREFIX]
    first, count, _ = sg.allele_groups(pick, keep)
    ops, ops_off, stats, rr = sg.allele_table_arrays(pool, pick)
    buf, off = pool.take(pick)
    buf = np.concatenate([buf, np.zeros(8, np.uint8)])
    amp = sg.ALLELE_AMPLICON.encode()
    rows = np.zeros((len(first), 3, 16), np.uint8)
    idx = np.ascontiguousarray(first, np.int64)
    assert _lib.load().nw_expand_ops_subset(amp, len(amp), _lib.ptr(buf), _lib.ptr(off), _lib.ptr(idx), len(idx),
                                            _lib.ptr(ops), _lib.ptr(ops_off), _lib.ptr(rows), 16, 1) == 0
    want = sg.allele_table_rows(pool, pick, first)
    assert np.array_equal(rows[:, 2, :], want[:, 0, :]) and np.array_equal(rows[:, 0, :], want[:, 1, :])
    assert set(np.diff(ops_off).tolist()) <= {1, 2} and np.all(stats[:, 0] == 16)
