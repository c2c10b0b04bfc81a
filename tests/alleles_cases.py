"""Inputs and the check of the allele grouping tests (tests/test_alleles_host.py on the CPU,
tests/test_gpu_alleles.py on the GPU): read families as lists of ``bytes``, and the groups a
plain dict over ``(tag, bytes)`` gives for them.

Run as ``python -m tests.alleles_cases forced`` it is the child process of the forced-collision
GPU test: CRISPR_NWA_HASH_BITS is read when the context is created, so each setting needs a
process of its own.
"""
import ctypes
import json
import sys

import numpy as np

LENGTHS = (0, 1, 3, 4, 5, 255, 256, 257, 1000)
SIZES = (0, 1, 2, 63, 64, 65, 5000)


def expected_groups(reads, keep=None, tag=None):
    """(first, count, group_of_read) from a dict over (tag, bytes), first appearance order."""
    seen, first, count, gor = {}, [], [], []
    for r, s in enumerate(reads):
        if keep is not None and not keep[r]:
            gor.append(-1)
            continue
        k = (0 if tag is None else int(tag[r]), bytes(s))
        g = seen.get(k)
        if g is None:
            g = seen[k] = len(first)
            first.append(r)
            count.append(0)
        count[g] += 1
        gor.append(g)
    return first, count, gor


def pack(reads, lead=0, shift=0):
    """The reads concatenated after ``lead`` filler bytes (padded to whole dwords), and their
    offsets plus ``shift`` (the bias a device call subtracts again)."""
    lens = np.fromiter((len(s) for s in reads), np.int64, len(reads))
    off = np.zeros(len(reads) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    raw = b"\xee" * lead + b"".join(reads)
    raw += b"\xee" * (-len(raw) % 4 + 4)
    return np.frombuffer(raw, np.uint8).copy(), off + lead + shift


def random_reads(n, seed, pool=40, lengths=LENGTHS):
    """n reads drawn from `pool` distinct values of the edge lengths (so groups repeat)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    values = []
    for k in range(pool):
        L = lengths[k % len(lengths)]
        values.append(bytes(rng.choice(np.frombuffer(b"ACGTN-", np.uint8), L)))
    pick = rng.integers(0, pool, n)
    return [values[i] for i in pick]


def near_equal_reads():
    """Prefixes, reads that differ in the first or the last byte only, at every edge length."""
    rng = np.random.Generator(np.random.PCG64(5))
    out = []
    for L in LENGTHS[1:]:
        base = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L))
        flip = {65: b"C", 67: b"G", 71: b"T", 84: b"A"}
        out += [base, base[:-1], base, flip[base[0]] + base[1:], base[:-1] + flip[base[-1]], base + b"A",
                base[: L // 2], base]
    return out


def families():
    """name -> (reads, keep, tag) of every family both test files run."""
    fam = {}
    for n in SIZES:
        fam[f"size{n}"] = (random_reads(n, 100 + n), None, None)
    near = near_equal_reads()
    fam["near_equal"] = (near, None, None)
    twins = random_reads(300, 7, pool=12)
    fam["tags"] = (twins, None, np.arange(300, dtype=np.int32) % 3)
    fam["tags_negative"] = (near, None, -(np.arange(len(near), dtype=np.int32) % 2))
    fam["keep_zero"] = (twins, np.zeros(300, np.uint8), None)
    fam["keep_third"] = (twins, (np.arange(300) % 3 == 0).astype(np.uint8), None)
    fam["keep_third_tags"] = (twins, (np.arange(300) % 3 == 1).astype(np.uint8), np.arange(300, dtype=np.int32) % 2)
    return fam


def collision_reads():
    """2,000 reads of 200 distinct values (the forced-collision input)."""
    rng = np.random.Generator(np.random.PCG64(11))
    values = set()
    while len(values) < 200:
        values.add(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(rng.integers(30, 61)))))
    values = sorted(values)
    return [values[i] for i in rng.integers(0, 200, 2000)]


def device_group(lib, ctx, reads, keep=None, tag=None, lead=0, bias=0, cap=None, want_gor=True):
    """nwa_group_device on own device buffers -> (rc, first, count, group_of_read, n_groups)."""
    from crispresso_amd import _lib
    from crispresso_amd.devmem import DeviceBuffer

    n = len(reads)
    buf, off = pack(reads, lead, bias)
    keep = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    tag = None if tag is None else np.ascontiguousarray(tag, np.int32)
    cap = n if cap is None else cap
    first = np.full(max(cap, 1), -5, np.int64)
    count = np.full(max(cap, 1), -5, np.int64)
    gor = np.full(max(n, 1), -5, np.int32) if want_gor else None
    ng, ms = ctypes.c_int64(-5), ctypes.c_float()
    with DeviceBuffer.from_array(buf) as d_buf, DeviceBuffer.from_array(off) as d_off:
        rc = lib.nwa_group_device(ctx, d_buf.ptr, d_off.ptr, bias, n, _lib.ptr(keep), _lib.ptr(tag), _lib.ptr(first),
                                  _lib.ptr(count), cap, _lib.ptr(gor), ctypes.byref(ng), ctypes.byref(ms))
    k = max(0, min(int(ng.value), cap))
    return rc, first[:k].tolist(), count[:k].tolist(), None if gor is None else gor[:n].tolist(), int(ng.value)


def forced_child():
    """The forced-collision run (CRISPR_NWA_HASH_BITS from the environment): the groups of
    collision_reads() twice on one context, against the dict; one JSON line."""
    from crispresso_amd import _lib

    lib = _lib.load()
    ctx = ctypes.c_void_p()
    rc = lib.nwa_create(0, ctypes.byref(ctx))
    if rc != 0:
        print(json.dumps({"ok": False, "why": f"nwa_create {rc}"}))
        return
    reads = collision_reads()
    tag = np.arange(len(reads), dtype=np.int32) % 2
    out = {"ok": True, "collided": []}
    for t in (None, tag):
        want = expected_groups(reads, None, t)
        rc, first, count, gor, ng = device_group(lib, ctx, reads, tag=t, lead=1)
        good = rc == 0 and (first, count, gor) == want and ng == len(want[0])
        out["ok"] = out["ok"] and good
        out["collided"].append(int(lib.nwa_last_collided(ctx)))
    lib.nwa_destroy(ctx)
    print(json.dumps(out))


if __name__ == "__main__" and sys.argv[1:] == ["forced"]:
    forced_child()
