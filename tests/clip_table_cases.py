"""Adapter tables of other shapes than NexteraPE-PE.fa, and read pairs built for them, for the clip
kernel (crispresso_amd/csrc/trim_clip.hip) against oracle/trimmomatic_oracle.py.

Everything is drawn from seeded generators.  A table is a list of FASTA records (name, random ACGT
sequence) that `write_fasta` puts into a file, so the oracle's IlluminaClip and the package's
TrimOptions.from_steps sort the same records into roles, prefix pairs and duplicates:

  simple_only          4 common adapters of 24, 25, 27, 28 bases (3, 3, 3, 4 seeds), no prefix pair
  prefix_only          one pair of 34 + 34 bases, no adapter
  unequal_long_prefix  a pair of 58 / 61 bases (cut to 58, skip 42), common adapters of 58, 61, 39, 31
  roles                a pair of 20 + 20; OnlyOne/1 (30), OnlyTwo/2 (33), Both (40), and OnlyOne's sequence
                       a second time under another /1 name
  full                 4 pairs of 12/12, 16/16, 17/20, 128/128 (in that order by name) and 16 adapters of
                       24 ... 128 bases, names cycling through no suffix, /1 and /2: every limit of
                       include/crispr_trim.h at once

`pairs` draws six kinds in turn (read-through of a random prefix pair with both reads at 151 bases and
at random lengths, a random adapter written into each mate at a position from inside the adapter to
the read's last base, twice, unrelated mates, twice), `named` the cases that single rules decide,
`long_cases` the two 4,096-base pairs of `full`.  `oracle` is the cached IlluminaClip pass over one of
those lists; the `variant_*` functions give the oracle without one rule (the witnesses of
tests/test_clip_table_cases.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import trimmomatic_oracle as tmo  # noqa: E402

DEFAULT = ":0:90:10:0:true"
SPECS = [DEFAULT, ":2:30:10", ":1:30:7:1:false"]
TABLES = ("simple_only", "prefix_only", "unequal_long_prefix", "roles", "full")
NEVER = sys.maxsize
N_PAIRS, SEED = 300, 5

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
_ACGT = np.frombuffer(b"ACGT", np.uint8)

FULL_PREFIXES = ((12, 12), (16, 16), (17, 20), (128, 128))
FULL_ADAPTERS = (24, 26, 29, 31, 32, 36, 44, 47, 48, 63, 64, 65, 96, 127, 128, 128)


def rc(s):
    return s[::-1].translate(COMP)


def _rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


def _rnd(rng, k):
    return bytes(rng.choice(_ACGT, k))


def records(table):
    """The table's FASTA records, (name, sequence bytes), in file order."""
    rng = _rng(101, TABLES.index(table))
    r = lambda k: _rnd(rng, k)  # noqa: E731
    if table == "simple_only":
        return [("Short%d" % n, r(n)) for n in (24, 25, 27, 28)]
    if table == "prefix_only":
        return [("PrefixPE/1", r(34)), ("PrefixPE/2", r(34))]
    if table == "unequal_long_prefix":
        return [("PrefixPE/1", r(58)), ("PrefixPE/2", r(61)), ("PCR_1", r(58)), ("PCR_1_rc", r(61)),
                ("Flow_rc", r(39)), ("Flow", r(31))]
    if table == "roles":
        one = r(30)
        return [("PrefixR/1", r(20)), ("PrefixR/2", r(20)), ("OnlyOne/1", one), ("OnlyTwo/2", r(33)),
                ("Both", r(40)), ("OnlyOneAgain/1", one)]
    assert table == "full"
    out = []
    for k, (l1, l2) in enumerate(FULL_PREFIXES):
        out += [("Prefix%s/1" % "ABCD"[k], r(l1)), ("Prefix%s/2" % "ABCD"[k], r(l2))]
    for k, n in enumerate(FULL_ADAPTERS):
        out.append(("Ad%02d%s" % (k, ("", "/1", "/2")[k % 3]), r(n)))
    return out


def prefix_pairs(table):
    """(prefix 1, prefix 2) as written in the file, uncut, in the order of their names."""
    recs = dict(records(table))
    names = sorted(n[:-2] for n in recs if n.startswith("Prefix") and n.endswith("/1"))
    return [(recs[n + "/1"], recs[n + "/2"]) for n in names]


def adapters(table):
    """(sequence, role) of the simple-mode records, duplicates included: role 0 both reads, 1, 2."""
    return [(s, 1 if n.endswith("/1") else 2 if n.endswith("/2") else 0)
            for n, s in records(table) if not n.startswith("Prefix")]


def write_fasta(table, directory):
    path = os.path.join(str(directory), table + ".fa")
    if not os.path.exists(path):
        with open(path, "w") as f:
            for name, seq in records(table):
                f.write(">%s\n%s\n" % (name, seq.decode()))
    return path


def _quals(rng, n, high=42):
    return bytes(rng.integers(0, high, n).astype(np.uint8) + 33)


def pairs(table, n=N_PAIRS, seed=SEED):
    """n pairs (read 1, qualities 1, read 2, qualities 2), six kinds in turn, mates of 8 to 151 bases."""
    pps, ads = prefix_pairs(table), [s for s, _ in adapters(table)]
    rng = _rng(seed, TABLES.index(table))
    r = lambda k: _rnd(rng, k)  # noqa: E731
    pick = lambda seqs: seqs[int(rng.integers(0, len(seqs)))]  # noqa: E731
    out = []
    for k in range(n):
        kind = k % 6
        L1, L2 = int(rng.integers(8, 152)), int(rng.integers(8, 152))
        if kind in (0, 1):                             # a short fragment read through into the adapters
            f = r(int(rng.integers(0, 140)))
            if kind == 0:
                L1 = L2 = 151
            if pps:
                p1, p2 = pick(pps)
                t1, t2 = rc(p2), rc(p1)
            else:
                t1, t2 = pick(ads), pick(ads)
            r1 = bytearray((f + t1 + r(160))[:L1])
            r2 = bytearray((rc(f) + t2 + r(160))[:L2])
        elif kind in (2, 3) and ads:                   # an adapter in each mate, whatever its role
            mates = []
            for L in (L1, L2):
                m = bytearray(r(L))
                a = pick(ads)
                p = int(rng.integers(-(len(a) - 16), L))
                at = max(p, 0)
                m[at:] = (a[max(-p, 0):] + r(160))[:L - at]
                mates.append(m)
            r1, r2 = mates
        else:                                          # unrelated mates
            r1, r2 = bytearray(r(L1)), bytearray(r(L2))
        nerr = int(rng.integers(0, 5))
        for m in (r1, r2):
            for _ in range(nerr):
                m[int(rng.integers(0, len(m)))] = b"ACGTN"[int(rng.integers(0, 5))]
        high = 94 if k % 5 == 4 else 42               # every fifth pair: the whole of phred 33's range
        out.append((bytes(r1), _quals(rng, len(r1), high), bytes(r2), _quals(rng, len(r2), high)))
    return out


def seeds_of(length):
    """16-mers the kernel and the oracle take from an adapter: positions 0, 4, 8, ..."""
    return (length - 15 + 3) // 4


def named(table):
    """[(label, mates, pair)]: `mates` are the mates (1, 2) of the pair that carry what the label names.
      last16  the read begins with adapter[s:] for an s in (4 (nk - 2), 4 (nk - 1)]: only the adapter's
              last 16-mer can seed it
      head    an adapter's first 12 to 15 bases at the read's 3' end (the masked partial 16-mers; they
              seed only where the simple threshold puts the minimum overlap below them)
      prefix  a read equal to a prefix as the file has it
      short   mates of 15 and 16 bases
      walk    (prefix pairs of 17 or more bases with an odd number of skipped steps) a read-through whose
              read 1 has a wrong base just before the 16-mer the palindrome walk's `ref` stands on at
              the overlap's own step, and as many more inside it as the seed tolerates: a walk whose
              `ref` is one base behind does not seed the overlap"""
    rng = _rng(211, TABLES.index(table))
    r = lambda k: _rnd(rng, k)  # noqa: E731
    out = []

    def add(label, mates, s1, s2):
        out.append((label, mates, (s1, _quals(rng, len(s1)), s2, _quals(rng, len(s2)))))

    def both(label, role, make):
        mates = (1, 2) if role == 0 else (role,)
        add(label, mates, make() if 1 in mates else r(60), make() if 2 in mates else r(60))

    seen = set()
    for a, role in adapters(table):
        if (a, role) in seen:
            continue
        seen.add((a, role))
        nk = seeds_of(len(a))
        for s in range(4 * (nk - 2) + 1, 4 * (nk - 1) + 1):
            both("last16", role, lambda: a[s:] + r(40))
        for h in range(12, 16):
            both("head", role, lambda: r(70) + a[:h])
    for p1, p2 in prefix_pairs(table):
        add("prefix", (1,), p1, r(60))
        add("prefix", (2,), r(60), p2)
        add("prefix", (1, 2), p1, p2)
    for l1, l2 in ((15, 16), (16, 15), (15, 15), (16, 16)):
        add("short", (1, 2), r(l1), r(l2))
    for p1, p2 in prefix_pairs(table):
        skip = min(len(p1), len(p2)) - 16
        if skip > 0 and skip % 2 == 1:
            for m, frags in ((0, (125, 127, 129, 131, 133, 135)), (1, (41, 61, 83, 99, 121, 123)),
                             (2, (43, 63, 85, 101, 119, 125))):
                for f in frags:
                    out.append(("walk", (1, 2), walk_case(rng, p1, p2, f, m)))
    if prefix_pairs(table):                            # 16-base mates that are a read-through
        p1, p2 = prefix_pairs(table)[-1]
        f = r(6)
        add("short", (1, 2), (f + rc(p2) + r(16))[:16], (rc(f) + rc(p1) + r(16))[:16])
    return out


def walk_case(rng, p1, p2, f, m):
    """A read-through of (p1, p2) at the odd fragment length f, mates of 151 bases, phred 20.  The
    overlap of f + 2 pl bases is step count = f + pl - 16 of PrefixPair.compare; with skip = pl - 16 odd
    that step is even, `ref` stands on read 1's base h = (f + 1) / 2 and `test` 16 bases before h - 1, so
    both 16-mers the step tries lie around read 1's base h - 1 without holding it.  That base is made
    wrong, and m more on each side of it inside the 16-mers (a seed of m mismatches still matches): a walk
    whose `ref` is one base lower (and `test` one higher) has m + 1 wrong bases in both of its 16-mers."""
    assert f % 2 == 1 and f >= 35
    h = (f + 1) // 2
    r1 = bytearray((_rnd(rng, f) + rc(p2) + _rnd(rng, 160))[:151])
    r2 = (rc(bytes(r1[:f])) + rc(p1) + _rnd(rng, 160))[:151]
    for x in [h - 1] + [h + 3, h + 9][:m] + [h - 5, h - 11][:m]:
        r1[x] = b"ACGT"[(b"ACGT".index(r1[x]) + 1) % 4]
    return bytes(r1), b"5" * 151, r2, b"5" * 151


LONG_FRAGMENT = 1500


def long_cases():
    """The two 4,096-base pairs of `full` (the one-wave launch, 128 prefix bases staged in front of the
    reads): a read-through of the 128-base prefix pair at fragment length 1,500, and a mate whose last 96
    bases are the head of a 128-base adapter that clips it."""
    rng = _rng(307)
    r = lambda k: _rnd(rng, k)  # noqa: E731
    p1, p2 = prefix_pairs("full")[-1]
    assert len(p1) == len(p2) == 128
    f = r(LONG_FRAGMENT)
    seqs = [((f + rc(p2) + r(4096))[:4096], (rc(f) + rc(p1) + r(4096))[:4096])]
    a, role = [(s, ro) for s, ro in adapters("full") if len(s) == 128][-1]
    tail = r(4000) + a[:96]
    seqs.append((r(4096), tail) if role == 2 else (tail, r(4096)))
    return [(s1, _quals(rng, len(s1)), s2, _quals(rng, len(s2))) for s1, s2 in seqs]


def case_list(table, what):
    if what == "pairs":
        return pairs(table)
    if what == "named":
        return [p for _, _, p in named(table)]
    assert what == "long" and table == "full"
    return long_cases()


# ---- the oracle, and the oracle without one rule ----

def variant_roles_ignored(clip, table):
    clip.com = clip.fwd + clip.rev + clip.com
    clip.fwd, clip.rev = [], []


def variant_cut_5prime(clip, table):
    for pp, (p1, p2) in zip(clip.pairs, prefix_pairs(table)):
        m = min(len(p1), len(p2))
        pp.p1, pp.p2 = p1[:m].decode(), p2[:m].decode()


def variant_first_pair_only(clip, table):
    del clip.pairs[1:]


def variant_last_pair_only(clip, table):
    del clip.pairs[:-1]


def variant_no_last_seed(clip, table):
    for cs in clip.fwd + clip.rev + clip.com:
        cs.pack = cs.pack[:-1]
        cs.index = {}
        for j, p in enumerate(cs.pack):
            cs.index.setdefault(p, []).append(j)


class ShiftedWalkPair(tmo.PrefixPair):
    """PrefixPair whose walk has counted one even step too many among the skipped ones when their number
    is odd: `ref` one base lower and `test` one higher at every step, up to the same cap."""

    def compare(self, s1, q1, s2, q2):
        pack1 = tmo.pack_internal(self.p1 + s1, False)
        pack2 = tmo.pack_internal(self.p2 + s2, True)
        pl = len(self.p1)
        test, ref = 0, pl
        if len(pack1) <= ref or len(pack2) <= ref:
            return NEVER
        count = 0
        skip = pl - 16
        if skip > 0:
            test = count = skip
            shift = ((skip + 1) >> 1) - (skip >> 1)
            ref, test = ref - shift, test + shift
        len1, len2 = len(s1) + pl, len(s2) + pl
        max_count = max(len1, len2) - 15 - self.min_prefix
        while count < max_count:
            if ((test < len(pack2) and bin(pack1[ref] ^ pack2[test]).count("1") <= self.seed_max)
                    or (test < len(pack1) and bin(pack2[ref] ^ pack1[test]).count("1") <= self.seed_max)):
                total = count + pl + 16
                skip1 = max(total - len2, 0)
                skip2 = max(total - len1, 0)
                if self.quality(s1, q1, s2, q2, total - skip1 - skip2, skip1, skip2) >= self.min_likelihood:
                    return total - 2 * pl
            count += 1
            if (count & 1) == 0 and ref + 1 < len(pack1) and ref + 1 < len(pack2):
                ref += 1
            else:
                test += 1
        return NEVER


def variant_walk_shifted(clip, table):
    for pp in clip.pairs:
        pp.__class__ = ShiftedWalkPair


def oracle_pass(clip, plist, single_end=False):
    """IlluminaClip.process on every pair -> keep1, keep2 (clipped lengths before MINLEN, 0 = dropped)
    and how often each test fired: pairs with a palindrome hit, with a hit of each prefix pair, reads 1
    and reads 2 a simple-mode adapter clipped, reads 2 dropped."""
    pal = [[] for _ in clip.pairs]
    simple = []
    for k, pp in enumerate(clip.pairs):
        pp.compare = (lambda *a, _f=pp.compare, _l=pal[k]: (_l.append(_f(*a)), _l[-1])[1])
    for cs in clip.fwd + clip.rev + clip.com:
        cs.compare = (lambda *a, _f=cs.compare: (simple.append(_f(*a)), simple[-1])[1])
    n_r1 = len(clip.fwd) + len(clip.com)
    k1, k2 = [], []
    counts = dict(palindrome=0, per_pair=[0] * len(clip.pairs), simple1=0, simple2=0, dropped2=0)
    for s1, q1, s2, q2 in plist:
        for x in pal:
            del x[:]
        del simple[:]
        a = ("r", s1.decode(), q1.decode())
        b = None if single_end else ("r", s2.decode(), q2.decode())
        ca, cb = clip.process(a, b)
        k1.append(0 if ca is None else len(ca[1]))
        k2.append(0 if cb is None else len(cb[1]))
        counts["palindrome"] += any(v != NEVER for x in pal for v in x)
        for k, x in enumerate(pal):
            counts["per_pair"][k] += any(v != NEVER for v in x)
        counts["simple1"] += any(v != NEVER for v in simple[:n_r1])
        counts["simple2"] += any(v != NEVER for v in simple[n_r1:])
        counts["dropped2"] += (not single_end) and cb is None
    for x in clip.pairs + clip.fwd + clip.rev + clip.com:
        del x.compare
    return np.array(k1, np.int32), np.array(k2, np.int32), counts


_CACHE = {}


def oracle(table, spec, directory, what="pairs", single_end=False, variant=None):
    """The cached pass over case_list(table, what); `variant` is one of the variant_* functions."""
    key = (table, spec, what, single_end, variant)
    if key not in _CACHE:
        clip = tmo.IlluminaClip(write_fasta(table, directory) + spec)
        if variant is not None:
            variant(clip, table)
        res = oracle_pass(clip, case_list(table, what), single_end)
        for a in res[:2]:
            a.setflags(write=False)
        _CACHE[key] = res
    return _CACHE[key]


def changed(a, b):
    """Reads (of both mates) whose keep length differs between two passes."""
    return int((a[0] != b[0]).sum() + (a[1] != b[1]).sum())


def minlen_applied(k, minlen):
    k = k.copy()
    k[k < minlen] = 0
    return k
