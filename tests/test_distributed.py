"""Sharding across devices / ranks (CPU: gloo world_size 2, oracle-backed aligner)."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from crispresso_amd import synth
from crispresso_amd.distributed import (MultiGpuAligner, align_pooled_sharded, align_sharded, cell_partition,
                                        pooled_costs, shard_range)


def test_shard_ranges_cover_everything():
    for n in (0, 1, 7, 8, 1001):
        for world in (1, 2, 3, 8):
            spans = [shard_range(n, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1


def _same(a, b):
    assert len(a) == len(b)
    for f in ("aln_len", "n_ident", "n_sim", "n_gaps", "score", "end_i", "end_j", "flags"):
        assert np.array_equal(a.stats[f], b.stats[f]), f
    for i in range(len(a)):
        L = int(a.stats["aln_len"][i])
        assert np.array_equal(a.aln[i, :, :L], b.aln[i, :, :L])


def test_multi_device_threads_equal_single():
    from tests.helpers import OracleAligner

    amp = synth.random_amplicon(150, 3)
    buf, off = synth.reads_from(amp, 301, 4, synth.PARITY_MIX)
    single = OracleAligner()
    single.set_reference(amp)
    ref = single.align_packed(buf, off)
    multi = MultiGpuAligner([0, 1, 2], factory=lambda d, o: OracleAligner(d, o))
    multi.set_reference(amp)
    _same(multi.align_packed(buf, off), ref)
    multi.close()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    from tests.helpers import OracleAligner

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    amp = synth.random_amplicon(120, 5)
    buf, off = synth.reads_from(amp, 97, 6, synth.PARITY_MIX)
    res = align_sharded(amp, buf, off, OracleAligner(), dist)
    if rank == 0:
        rows = res.expand(amp, buf, off, nthreads=1)   # rank 0 got records + runs, not rows
        np.save(os.path.join(out_dir, "stats.npy"), rows.stats)
        np.save(os.path.join(out_dir, "aln.npy"), rows.aln)
    else:
        assert res is None
    # pooled: cell-count partition, records + runs gathered in read order
    amps, pbuf, poff, which = _pooled()
    pres = align_pooled_sharded(amps, pbuf, poff, which, OracleAligner(), dist)
    if rank == 0:
        np.save(os.path.join(out_dir, "pstats.npy"), pres.stats)
        np.save(os.path.join(out_dir, "pops.npy"), pres.ops)
        np.save(os.path.join(out_dir, "poff.npy"), pres.ops_off)
    else:
        assert pres is None
    dist.barrier()
    dist.destroy_process_group()


def _pooled():
    amps = synth.pooled_amplicons(5, 9)
    parts = [synth.reads_from(a, 7 + 13 * g, 20 + g) for g, a in enumerate(amps)]
    reads = []
    for b, o in parts:
        reads += synth.unpack(b, o)
    which = np.repeat(np.arange(len(amps), dtype=np.int32), [len(o) - 1 for _, o in parts])
    from crispresso_amd.aligner import pack_reads

    buf, off = pack_reads(reads)
    return amps, buf, off, which


def test_gloo_world2_gathers_in_read_order(tmp_path):
    from tests.helpers import OracleAligner

    mp.start_processes(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="fork")
    amp = synth.random_amplicon(120, 5)
    buf, off = synth.reads_from(amp, 97, 6, synth.PARITY_MIX)
    al = OracleAligner()
    al.set_reference(amp)
    ref = al.align_packed(buf, off)
    stats = np.load(tmp_path / "stats.npy")
    aln = np.load(tmp_path / "aln.npy")
    assert np.array_equal(stats, ref.stats)
    for i in range(len(stats)):
        L = int(stats["aln_len"][i])
        assert np.array_equal(aln[i, :, :L], ref.aln[i, :, :L])
    amps, pbuf, poff, which = _pooled()
    want = OracleAligner().align_multi_ops(amps, pbuf, poff, which)
    assert np.array_equal(np.load(tmp_path / "pstats.npy"), want.stats)
    assert np.array_equal(np.load(tmp_path / "pops.npy"), want.ops)
    assert np.array_equal(np.load(tmp_path / "poff.npy"), want.ops_off)


def test_cell_partition_balances_pooled_work():
    amps = synth.pooled_amplicons(96, 5)
    rng = np.random.Generator(np.random.PCG64(1))
    counts = rng.integers(0, 2000, 96)
    which = np.repeat(np.arange(96, dtype=np.int32), counts)
    lens = np.concatenate([rng.integers(len(a) - 30, len(a) + 10, c) for a, c in zip(amps, counts)])
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    costs = pooled_costs(amps, off, which)
    for world in (1, 2, 3, 8):
        parts = cell_partition(costs, world)
        assert parts[0][0] == 0 and parts[-1][1] == len(costs)
        assert all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        share = costs.sum() / world
        for lo, hi in parts:
            assert abs(costs[lo:hi].sum() - share) <= costs.max() + 1   # within one read of the ideal share
    assert cell_partition(np.zeros(0), 4) == [(0, 0)] * 4


def test_multi_device_ops_and_pooled_equal_single():
    from tests.helpers import OracleAligner

    amp = synth.random_amplicon(150, 3)
    buf, off = synth.reads_from(amp, 301, 4)
    single = OracleAligner()
    single.set_reference(amp)
    ref = single.align_ops(buf, off)
    multi = MultiGpuAligner([0, 1, 2], factory=lambda d, o: OracleAligner(d, o))
    multi.set_reference(amp)
    got = multi.align_ops(buf, off)
    assert np.array_equal(got.stats, ref.stats) and np.array_equal(got.ops, ref.ops)
    assert np.array_equal(got.ops_off, ref.ops_off)
    amps, pbuf, poff, which = _pooled()
    want = single.align_multi_ops(amps, pbuf, poff, which)
    got = multi.align_multi_ops(amps, pbuf, poff, which)
    assert np.array_equal(got.stats, want.stats) and np.array_equal(got.ops, want.ops)
    multi.close()


def test_multi_device_pooled_then_single_amplicon_pass():
    """A pooled call leaves every context without an amplicon; the MultiGpuAligner says
    so too, so the next single-amplicon pass (needle_pass) sets its amplicon again
    instead of finding it 'already set' (ADVICE r2)."""
    from crispresso_amd.needle import needle_pass
    from tests.helpers import OracleAligner

    multi = MultiGpuAligner([0, 1], factory=lambda d, o: OracleAligner(d, o))
    amp = synth.random_amplicon(150, 3)
    buf, off = synth.reads_from(amp, 51, 4)
    multi.set_reference(amp)
    amps, pbuf, poff, which = _pooled()
    multi.align_multi_ops(amps, pbuf, poff, which)
    assert multi.reference is None
    for al in multi.aligners:
        al.reference = None    # what the native contexts are left with
    res = needle_pass(multi, amp, [f"r{i}" for i in range(51)], buf, off)
    want = OracleAligner()
    want.set_reference(amp)
    assert np.array_equal(res.ops.stats, want.align_ops(buf, off).stats)
    multi.close()


def test_multi_device_resident_second_pass():
    """align_ops(resident=True) re-aligns each device's last shard (the HDR pass)."""
    from tests.helpers import OracleAligner

    multi = MultiGpuAligner([0, 1, 2], factory=lambda d, o: OracleAligner(d, o))
    amp = synth.random_amplicon(150, 3)
    hdr = synth.hdr_amplicon(amp, 4)
    buf, off = synth.reads_from(amp, 301, 4)
    multi.set_reference(amp)
    multi.align_ops(buf, off)
    multi.set_reference(hdr)
    got = multi.align_ops(None, off, resident=True, records_only=True)
    single = OracleAligner()
    single.set_reference(hdr)
    assert np.array_equal(got.stats, single.align_ops(buf, off).stats)
    with pytest.raises(Exception):
        multi.align_ops(None, off[:100], resident=True)
    multi.close()


def _shm_write_seconds(nbytes):
    """Seconds the ranks take, between two barriers, to each write nbytes of its own into a fresh
    shared-memory mapping with one plain copy: what the host's memory system gives a gather's
    writers at this moment (page faults and the load of the host included)."""
    import mmap
    import time

    src = np.ones(nbytes, np.uint8)
    path = f"/dev/shm/crispr_gather_ref_{os.getpid()}"
    fd = os.open(path, os.O_CREAT | os.O_EXCL | os.O_RDWR, 0o600)
    try:
        os.ftruncate(fd, nbytes)
        mm = mmap.mmap(fd, nbytes)
    finally:
        os.close(fd)
        os.unlink(path)
    dst = np.ndarray(nbytes, np.uint8, buffer=mm)
    dist.barrier()
    t0 = time.perf_counter()
    dst[...] = src
    dist.barrier()
    dt = time.perf_counter() - t0
    del dst
    mm.close()
    return dt


def _gather_worker(rank, world, port, out_dir, n, method):
    import time

    from crispresso_amd import _lib
    from crispresso_amd.aligner import OpsBatch
    from crispresso_amd.distributed import _gather_ops

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rng = np.random.Generator(np.random.PCG64(rank))
    lo, hi = shard_range(n, world, rank)
    m = hi - lo
    stats = np.zeros(m, _lib.STAT_DTYPE)
    stats["aln_len"] = rng.integers(200, 300, m)
    stats["score"] = np.arange(lo, hi)
    cnt = rng.integers(1, 4, m)
    off = np.zeros(m + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    ops = (np.arange(int(off[-1]), dtype=np.uint32) + np.uint32(7 * rank)) & np.uint32(0x3fffffff)
    mine = OpsBatch(stats, ops, off, rng.integers(220, 260, m).astype(np.int64), 2)
    my_bytes = stats.nbytes + ops.nbytes + off.nbytes + mine.read_lens.nbytes
    ref_dt = _shm_write_seconds(my_bytes) if method == "shm" else 0.0
    dist.barrier()
    t0 = time.perf_counter()
    res = _gather_ops(mine, dist, rank, world, method)
    dt = time.perf_counter() - t0
    if method == "shm":   # the slower of the plain writes before and after the gather
        ref_dt = max(ref_dt, _shm_write_seconds(my_bytes))
    if rank == 0:
        np.save(os.path.join(out_dir, "g_stats.npy"), res.stats)
        np.save(os.path.join(out_dir, "g_ops.npy"), res.ops)
        np.save(os.path.join(out_dir, "g_off.npy"), res.ops_off)
        np.save(os.path.join(out_dir, "g_lens.npy"), res.read_lens)
        nbytes = res.stats.nbytes + res.ops.nbytes + res.ops_off.nbytes + res.read_lens.nbytes
        with open(os.path.join(out_dir, "g_rate.txt"), "w") as f:
            f.write(f"{nbytes / dt / 1e9:.3f} {dt:.3f} {nbytes / ref_dt / 1e9 if ref_dt else 0.0:.3f}")
    else:
        assert res is None
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("method,n", [("shm", 10_000_000), ("p2p", 1_000_000)])
def test_gather_records_and_runs_scales(tmp_path, method, n):
    """Rank 0 gathers 10M reads' records + runs (about 45 B per read, ~0.5 GB) of a world-2 job
    without pickling: shared memory between the ranks of one host (1.9-2.2 GB/s on an idle 8-CPU
    host, page faults dominating), tensors point-to-point otherwise; the joined arrays equal the
    parts concatenated in read order.  The rate is held against what the host gives at that moment:
    the ranks writing the same bytes into fresh shared memory with one plain copy each, timed the
    same way right before and right after the gather (the slower of the two).  The gather is that
    write plus a 32-byte exchange and two barriers, so it keeps within 2x of it, on an idle host
    (where this is the 1.0 GB/s floor the test had) as on a loaded one (where a fixed floor failed
    at 0.39 GB/s)."""
    from crispresso_amd import _lib
    from crispresso_amd.aligner import OpsBatch
    from crispresso_amd.distributed import concat_ops

    mp.start_processes(_gather_worker, args=(2, _free_port(), str(tmp_path), n, method), nprocs=2, join=True,
                       start_method="fork")
    parts = []
    for rank in range(2):
        rng = np.random.Generator(np.random.PCG64(rank))
        lo, hi = shard_range(n, 2, rank)
        m = hi - lo
        stats = np.zeros(m, _lib.STAT_DTYPE)
        stats["aln_len"] = rng.integers(200, 300, m)
        stats["score"] = np.arange(lo, hi)
        cnt = rng.integers(1, 4, m)
        off = np.zeros(m + 1, np.int64)
        np.cumsum(cnt, out=off[1:])
        ops = (np.arange(int(off[-1]), dtype=np.uint32) + np.uint32(7 * rank)) & np.uint32(0x3fffffff)
        parts.append(OpsBatch(stats, ops, off, rng.integers(220, 260, m).astype(np.int64), 2))
    want = concat_ops(parts)
    assert np.array_equal(np.load(tmp_path / "g_stats.npy"), want.stats)
    assert np.array_equal(np.load(tmp_path / "g_ops.npy"), want.ops)
    assert np.array_equal(np.load(tmp_path / "g_off.npy"), want.ops_off)
    assert np.array_equal(np.load(tmp_path / "g_lens.npy"), want.read_lens)
    rate, secs, ref_rate = map(float, open(tmp_path / "g_rate.txt").read().split())
    print(f"gather {method}: {rate:.2f} GB/s ({secs:.3f} s); plain shared-memory write {ref_rate:.2f} GB/s")
    if method == "shm":
        assert rate >= 0.5 * ref_rate, (rate, ref_rate)
