"""Inputs and the check of the sgRNA counting tests (tests/test_gpu_count.py): batches of reads as
lists of ``bytes``, and the comparison of a :class:`crispresso_amd.count.GuideCounts` with
tests/count_model.py read by read and group by group.

Run as ``python -m tests.count_cases <mode>`` it is the child process of the tests whose
setting is read when the context is created (CRISPR_NWC_HASH_BITS, CRISPR_NWC_CHUNK): one JSON
line with what the run found.
"""
import hashlib
import json
import sys

import numpy as np

from tests import count_model as cm
from tests.alleles_cases import pack

T20 = b"GTTTTAGAGCTAGAAATAGC"
ALPHABET = b"abcdefghijklmnopqrstuvwxyz"      # filler: lower case, which no pattern of upper-case bases matches
FLIP = {65: b"C", 67: b"G", 71: b"T", 84: b"N", 78: b"A"}


def pattern(m, seed=0):
    """m bases, the first equal to the last (so the pattern can overlap itself by one)."""
    rng = np.random.Generator(np.random.PCG64(1000 + 7 * m + seed))
    p = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), m).tobytes())
    p[-1] = p[0]
    return bytes(p)


def filler(n, k=0):
    """n filler bytes, different for every k (so the guides cut from them differ)."""
    a = len(ALPHABET)
    return bytes(ALPHABET[(k * 7 + i * (1 + k % 5)) % a] for i in range(n))


def edge_batch(m, L):
    """(reads, T, sizes): the find edges of one (m, L); ``sizes`` counts each family."""
    T = pattern(m)
    n70 = 70 if m <= 64 else m + 6
    fam = {}

    def add(name, rs):
        fam[name] = list(rs)

    add("every_position", [filler(idx, idx) + T + filler(n70 - m - idx, idx + 1) for idx in range(n70 - m + 1)])
    add("cut_off", [filler(n70 - m + 1, 3) + T[:m - 1]] if m > 1 else [filler(n70, 3)])
    straddle = []
    for k in sorted({1, m // 2, m - 1} - {0, m}):
        straddle += [filler(40, k) + T[:k], T[k:] + filler(41, k + 1)]
    add("straddle", straddle)
    add("lower", [filler(25, 5) + T.lower() + filler(9, 6)])
    add("one_substitution", [filler(30, j) + T[:j] + FLIP[T[j]] + T[j + 1:] + filler(11, j) for j in range(m)])
    add("twice", [filler(22, 8) + T + filler(5, 9) + T + filler(3, 1), filler(21, 2) + T + T[1:] + filler(7, 3),
                  T + T])
    add("short", [T[:m - 1], T[1:], b"A", filler(max(m - 1, 0), 4)])
    add("slice", [filler(3, 11) + T, filler(3, 12) + T + filler(2, 1), T, filler(L, 13) + T, filler(L + 1, 14) + T,
                  filler(max(L - 1, 0), 15) + T])
    g = (b"ACGTNACGT" * 8)[:L]
    add("guide_bytes", [g + T + b"xx", g.lower() + T + b"xx", g + T, g.lower() + T, g.replace(b"N", b"A") + T,
                        filler(6, 2) + g + T, b"n" * L + T])
    add("long", [filler(300 - m, 16) + T, filler(300, 17), filler(70000 - m - 11, 18) + T + filler(11, 19),
                 filler(1234, 20) + T + filler(70000, 21), filler(70000, 22)])
    body = [r for name in ("every_position", "cut_off", "straddle", "lower", "one_substitution", "twice", "short",
                           "slice", "guide_bytes") for r in fam[name]]
    plain = fam["every_position"]
    while len(body) < 130:
        body += plain
    # empties: consecutive ones at a wavefront's start and end (reads 0-1, 62-65, 126-129), one alone
    reads = [b"", b""] + body[:60] + [b""] * 4 + body[60:120] + [b""] * 4 + body[120:]
    reads = reads[:140] + fam["long"][:2] + reads[140:] + [b""] + fam["long"][2:] + plain[:3] + [b"", b""]
    assert all(reads[i] == b"" for i in (0, 1, 62, 63, 64, 65, 126, 127, 128, 129)) and reads[-1] == b""
    sizes = {k: len(v) for k, v in fam.items()}
    sizes["reads"] = len(reads)
    return reads, T, sizes


def slice_cases():
    """[(reads, T, L)] of the hand-computed list of tests/test_count_model.py."""
    T5 = b"ACGTA"
    out = []
    r70 = []
    for idx in list(range(20, 51)) + [0, 1, 19]:
        r70.append(filler(idx, idx) + T20 + filler(50 - idx, idx + 3))
    out.append((r70, T20, 20))
    out.append(([filler(3, 1) + T5 + filler(7, 2)], T5, 20))            # (15, 5, 20, 3): s[0:3]
    out.append(([filler(3, 1) + T5 + filler(17, 2)], T5, 22))           # (25, 5, 22, 3): empty
    out.append((r70, T20, 0))
    out.append(([b"A" * 30, b"A" * 4, b"A" * 3, b"cA" + b"A" * 40], b"AAAA", 20))
    out.append(([filler(25, 1) + T5 + filler(20, 2) + T5 + filler(15, 3)], T5, 4))
    return out


def _bases(rng, shape):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), shape)


def library(n_guides, seed, L=20):
    rng = np.random.Generator(np.random.PCG64(seed))
    lib = set()
    while len(lib) < n_guides:
        lib.add(_bases(rng, L).tobytes())
    return sorted(lib)


def mixed_batch(n=50000, n_guides=1000, seed=21, T=T20, L=20, sub=0.05, miss=0.02):
    """n reads of 4 + L + m + 6 bases: a guide of the library (Zipf-like weights), T, random
    flanks; `sub` of them with one substitution in the guide, `miss` with one in T (no match)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lib = library(n_guides, seed + 1, L)
    w = 1.0 / np.arange(1, n_guides + 1)
    pick = rng.choice(n_guides, n, p=w / w.sum())
    pick[:n_guides] = rng.permutation(n_guides)            # every guide at least once
    m = len(T)
    a = np.empty((n, 4 + L + m + 6), np.uint8)
    a[:, :4] = _bases(rng, (n, 4))
    a[:, 4:4 + L] = np.frombuffer(b"".join(lib), np.uint8).reshape(n_guides, L)[pick]
    a[:, 4 + L:4 + L + m] = np.frombuffer(T, np.uint8)
    a[:, 4 + L + m:] = np.frombuffer(b"cagtca"[:6], np.uint8)      # lower case: no second T by chance
    a[:, :4] |= 0x20
    kinds = rng.random(n)
    is_sub, is_miss = kinds < sub, (kinds >= sub) & (kinds < sub + miss)
    col = rng.integers(0, L, n)
    rows = np.flatnonzero(is_sub)
    a[rows, 4 + col[rows]] = np.frombuffer(b"N", np.uint8)
    rows = np.flatnonzero(is_miss)
    a[rows, 4 + L + (col[rows] % m)] = np.frombuffer(b"n", np.uint8)
    reads = [a[i].tobytes() for i in range(n)]
    return reads, T, L, {"sub": int(is_sub.sum()), "miss": int(is_miss.sum()), "library": lib}


def distinct_batch(n=20000, seed=22, T=T20, L=20):
    """n reads, every guide different (a counter written into the guide)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    body = _bases(rng, (n, L))
    reads = []
    for i in range(n):
        g = bytearray(body[i].tobytes())
        tag = b"%06d" % i
        g[:min(6, L)] = tag[:min(6, L)]
        reads.append(b"tt" + bytes(g) + T + b"c")
    return reads, T, L


def whitelist_batch(seed=23, L=20):
    """(reads, T, L, lines): 1,000 keys + a duplicate + the empty line + a 19-byte key; reads of
    members, of non-members and with empty guides; members without reads.  No read of L = 20 has
    a 19-byte guide (a tracrRNA at 19 gives the empty one), so that key must stay at zero."""
    reads, T, L, info = mixed_batch(20000, 1500, seed, T20, L)
    lib = info["library"]
    rng = np.random.Generator(np.random.PCG64(seed + 5))
    members = [lib[i] for i in rng.permutation(1500)[:1000]]
    absent = library(40, seed + 9, L)                                  # members no read holds
    short = members[3][:19]
    lines = members[:500] + [members[7] + b"\n", b""] + absent + members[500:] + [short, b"  " + members[0] + " ".encode()]
    extra = [T + b"cc", b"ac" + T, short + T, short + T, b"", T[:-1]]     # all of them the empty guide
    reads = reads[:5000] + extra + reads[5000:]
    return reads, T, L, lines, {"members": members, "absent": absent, "short": short}


def chunk_batch(seed=24):
    """10,500 reads for chunks of 1,000: the reads of chunk 5 (4000..4999) hold no T, and one
    guide is seen first in chunk 3 (read 2500) and again in chunks 7 and 11 only."""
    reads, T, L, info = mixed_batch(10500, 300, seed)
    special = b"NNNNACGTACGTACGTNNNN"
    for r in range(4000, 5000):
        reads[r] = reads[r].replace(T, T[:5] + b"n" + T[6:])
    for r in (2500, 6500, 10200):
        reads[r] = b"acgt" + special + T + b"cagtca"
    return reads, T, L, special


def mismatches(got, want, limit=5):
    """What differs between a GuideCounts and the model's dict, naming reads and groups."""
    bad = []
    for k in ("n_reads", "n_found", "n_counted"):
        if int(getattr(got, k)) != want[k]:
            bad.append(f"{k}: {getattr(got, k)} != {want[k]}")
    for name, ours in (("pos", got.pos), ("group_of_read", got.group_of_read)):
        if ours is None:
            continue
        ours = np.asarray(ours).tolist()
        if ours != want[name]:
            diff = [r for r, (x, y) in enumerate(zip(ours, want[name])) if x != y][:limit]
            bad.append(f"{name}: {len(ours)} vs {len(want[name])} reads; first differences at reads "
                       + ", ".join(f"{r}: {ours[r]} != {want[name][r]}" for r in diff))
    if list(got.guides) != want["guides"]:
        diff = [g for g, (x, y) in enumerate(zip(got.guides, want["guides"])) if x != y][:limit]
        bad.append(f"guides: {len(got.guides)} vs {len(want['guides'])}; first differences at groups "
                   + ", ".join(f"{g}: {got.guides[g]!r} != {want['guides'][g]!r}" for g in diff))
    for name, ours in (("counts", got.counts), ("first", got.first)):
        ours = np.asarray(ours).tolist()
        if ours != want[name]:
            diff = [g for g, (x, y) in enumerate(zip(ours, want[name])) if x != y][:limit]
            bad.append(f"{name}: first differences at groups " + ", ".join(f"{g}: {ours[g]} != {want[name][g]}" for g in diff))
    return bad


def digest(got):
    """One hash over every returned array (byte-equality of two runs)."""
    h = hashlib.sha256()
    for part in (b"\0".join(got.guides), np.asarray([len(g) for g in got.guides], np.int64).tobytes(),
                 got.counts.tobytes(), got.first.tobytes(), got.pos.tobytes(), got.group_of_read.tobytes(),
                 np.asarray([got.n_reads, got.n_found, got.n_counted], np.int64).tobytes()):
        h.update(part)
        h.update(b"|")
    return h.hexdigest()


def run(counter, reads, T, L, guides=None, lead=0):
    from crispresso_amd import count

    buf, off = pack(reads, lead)
    return count.count_guides(buf, off, T.decode(), L, guides, counter, want_pos=True, want_group_of_read=True)


def child(mode):
    from crispresso_amd import count

    out = {"ok": True, "bad": [], "collided": [], "digest": []}
    with count.GpuGuideCounter(0) as c:
        def one(reads, T, L, guides=None):
            got = run(c, reads, T, L, guides)
            bad = mismatches(got, cm.fast_model(reads, T, L, guides))
            out["ok"] = out["ok"] and not bad
            out["bad"] += bad
            out["collided"].append(got.collided)
            out["digest"].append(digest(got))

        if mode == "mixed":
            reads, T, L, _ = mixed_batch()
            one(reads, T, L)
        elif mode == "whitelist":
            reads, T, L, lines, _ = whitelist_batch()
            one(reads, T, L, lines)
        elif mode == "chunks":
            reads, T, L, _ = chunk_batch()
            one(reads, T, L)
            one(reads, T, L, [reads[2500][4:24], reads[0][4:24], b""])
            one([], T, L)
            one(reads[2500:2501], T, L)
            one(reads[4000:4001], T, L)
    print(json.dumps(out))


if __name__ == "__main__" and len(sys.argv) == 2:
    child(sys.argv[1])
