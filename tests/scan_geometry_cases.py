"""Inputs and expected outputs of the block-sum scan tests (tests/test_scan_geometry_cases.py on
the CPU, tests/test_gpu_scan_geometry.py on the GPU): batches large enough that the one scan block
of a stage takes more than 1,024 block sums, so that every scan thread owns several sums
(``per > 1``), the last share is clamped, and some threads own a share with nothing in it.

In all of these stages the outcome of a read depends on the read alone; order comes from
cumulative sums only.  So every large input is a seeded, non-periodic draw from a small pool of
distinct items; the existing plain model gives each pool item's outcome once, and the expected
arrays are assembled with numpy.  tests/test_scan_geometry_cases.py pins every assembly to the slow
model run outright on a prefix and on a window that straddles item 262,144.
"""
import functools
import types

import numpy as np

from crispresso_amd.aligner import pack_2bit
from tests import demux_model as dm
from tests import front_model as fm
from tests import trim_steps_model as tsm

SCAN_THREADS = 1024        # kScanBlk: front_pack.hip:50, nw_demux.hip:326, nw_regions.hip:89
STRADDLE = 262144          # 1,024 blocks of 256: the first item whose block sum is the 1,025th


# ---- what the scan block will see -----------------------------------------------------------

def per_of(blocks):
    """Sums per scan thread: front_pack.hip:224, nw_demux.hip:442, nw_regions.hip:230 and 642."""
    return (blocks + SCAN_THREADS - 1) // SCAN_THREADS


def shares(block_sums):
    """(per, [(lo, hi)] of the 1,024 scan threads, each share's sum): lo = min(blocks, t * per),
    hi = min(blocks, lo + per)."""
    blocks = len(block_sums)
    per = per_of(blocks)
    lo = np.minimum(blocks, np.arange(SCAN_THREADS, dtype=np.int64) * per)
    hi = np.minimum(blocks, lo + per)
    cs = np.concatenate([[0], np.cumsum(np.asarray(block_sums, np.int64))])
    return per, lo, hi, cs[hi] - cs[lo]


def block_sums(values, block):
    """The sum of every ``block`` consecutive values (the last block short)."""
    v = np.asarray(values, np.int64)
    pad = (-len(v)) % block
    return np.concatenate([v, np.zeros(pad, np.int64)]).reshape(-1, block).sum(axis=1)


# ---- pools ----------------------------------------------------------------------------------

class Pool:
    """Distinct byte strings as a zero-padded matrix, so that a draw is assembled by indexing."""

    def __init__(self, items):
        self.items = [bytes(x) for x in items]
        self.lens = np.fromiter((len(x) for x in self.items), np.int64, len(self.items))
        self.mat = np.zeros((len(self.items), max(1, int(self.lens.max(initial=0)))), np.uint8)
        for i, x in enumerate(self.items):
            self.mat[i, :len(x)] = np.frombuffer(x, np.uint8)

    def take(self, pick):
        """(buf, offsets) of the items ``pick`` one after the other."""
        pick = np.asarray(pick, np.int64)
        lens = self.lens[pick]
        off = np.zeros(len(pick) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        out = np.empty(int(off[-1]), np.uint8)
        step = 1 << 18                                   # (bounds the temporary rows)
        for a in range(0, len(pick), step):
            b = min(len(pick), a + step)
            rows = self.mat[pick[a:b]]
            out[off[a]:off[b]] = rows[np.arange(rows.shape[1]) < lens[a:b, None]]
        return out, off


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# =============================================================================================
# 1. The front packer (front_pack.hip): 256 reads a block, three quantities a block
# =============================================================================================

FRONT_BLOCK = 256          # kBlk, front_pack.hip:49
LEN_GROUP = 1024           # nw::kLenGroup
FRONT_SE_TRIM = ["LEADING:5", "MINLEN:6"]
DEAD_RUN = 1600            # consecutive dead reads at the start, in the middle and at the end
# se_2049 is 2048 * 256 + 77 reads: 2,049 blocks, per = 3, every working thread's share full and
# thread 683 starting at `blocks`.  One block more (se_2050) leaves thread 683 a share of one block,
# clamped, and thread 684 starting at `blocks`.
FRONT_SIZES = {"se_1025": 262145, "se_2049": 2048 * 256 + 77, "se_2050": 2049 * 256 + 77, "pe_1025": 262145}


def front_se_pool():
    """480 single-end reads of 1-40 bases: good qualities (most), low throughout (the filter), one
    base below the single-base threshold (the filter), a low head (LEADING cuts it), too short
    after the cut (MINLEN drops it); a tenth carries N, IUPAC codes, a dash or lower case."""
    rng = _rng(9101)
    out, seen = [], set()
    while len(out) < 480:
        L = int(rng.integers(1, 41))
        s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].copy()
        q = rng.integers(25, 41, L)
        fam = rng.choice(5, p=[0.6, 0.12, 0.06, 0.12, 0.1])
        if fam == 1:
            q = rng.integers(4, 16, L)
        elif fam == 2:
            q[int(rng.integers(0, L))] = 2
        elif fam == 3:
            q[:int(rng.integers(1, 6))] = rng.integers(3, 5)
        elif fam == 4:
            q[:max(0, L - int(rng.integers(0, 6)))] = 3
        if rng.random() < 0.1:
            for p in rng.integers(0, L, int(rng.integers(1, 4))):
                s[p] = rng.choice(np.frombuffer(b"NNnRY-acgt", np.uint8))
        item = (s.tobytes(), (q + 33).astype(np.uint8).tobytes(), b"", b"")
        if item[:2] not in seen:
            seen.add(item[:2])
            out.append(item)
    return out


def front_pe_pool():
    """1,600 pairs of tests/front_model.py's packer families (unrelated mates, read-through, the
    filter's, SLIDINGWINDOW's, N in a tenth), another seed than the packer test's."""
    return fm.packer_pairs(seed=9102, n=1600)


def front_settings(single_end):
    kw = dict(fm.PACKER_FILTER, single_end=single_end)
    kw["trim"] = FRONT_SE_TRIM if single_end else fm.PACKER_TRIM
    return kw


def front_trim_class(pairs, single_end):
    """Per pair 0..3 = both / fwd_only / rev_only / dropped of Trimmomatic's summary, -1 for a
    pair the quality filter took first: fm.expected's own rule, kept per pair."""
    from crispresso_amd import fastq

    kw = front_settings(single_end)
    a = fastq.quality_pass([p[1] for p in pairs], kw["min_bp_quality"], kw["min_single_bp_quality"])
    b = a if single_end else fastq.quality_pass([p[3] for p in pairs], kw["min_bp_quality"], kw["min_single_bp_quality"])
    rec1, rec2 = tsm.run_pairs(kw["trim"], pairs, single_end=single_end)
    out = np.full(len(pairs), -1, np.int64)
    for i, (x, y) in enumerate(zip(rec1, rec2)):
        if a[i] and b[i]:
            ok_b = single_end or y is not None
            out[i] = 0 if x is not None and ok_b else 1 if x is not None else 2 if (y is not None and not single_end) else 3
    return out


@functools.lru_cache(maxsize=None)
def front_pool(single_end):
    """The pool and the model's outcome of each of its items."""
    pairs = front_se_pool() if single_end else front_pe_pool()
    e = fm.expected(pairs, **front_settings(single_end))
    merged, mquals = [b""] * len(pairs), [b""] * len(pairs)
    for j, i in enumerate(e.src.tolist()):
        merged[i], mquals[i] = e.reads[j], e.quals[j]
    return types.SimpleNamespace(
        pairs=pairs, status=e.status.copy(), trim_class=front_trim_class(pairs, single_end),
        inputs=[Pool([p[k] for p in pairs]) for k in range(4)], merged=Pool(merged), mquals=Pool(mquals),
        dead=np.flatnonzero(e.status < fm.COMBINED), alive=np.flatnonzero(e.status >= fm.COMBINED))


def front_assemble(pool, pick):
    """fm.Expected of the pool items ``pick``, from the pool's outcomes alone."""
    pick = np.asarray(pick, np.int64)
    status = pool.status[pick]
    src = np.flatnonzero(status >= fm.COMBINED).astype(np.int64)
    buf, offsets = pool.merged.take(pick[src])
    qbuf, _ = pool.mquals.take(pick[src])
    lens = np.diff(offsets).astype(np.uint16)
    pk = pack_2bit(buf, offsets, nthreads=1)
    tc = pool.trim_class[pick]
    trim = {name: int(np.sum(tc == k)) for k, name in enumerate(("both", "fwd_only", "rev_only", "dropped"))}
    return fm.Expected(status, src, None, None, buf, qbuf, offsets, lens, pk, trim)


def front_inputs(pool, pick, single_end):
    """The six arguments of frontend.prepare_packed."""
    s1, off1 = pool.inputs[0].take(pick)
    q1, _ = pool.inputs[1].take(pick)
    if single_end:
        return s1, q1, off1, None, None, None
    s2, off2 = pool.inputs[2].take(pick)
    q2, _ = pool.inputs[3].take(pick)
    return s1, q1, off1, s2, q2, off2


@functools.lru_cache(maxsize=None)
def front_case(name):
    """(pool, pick, expected, single_end).  DEAD_RUN dead reads open the batch, close it and sit
    in the middle; se_1025's survivor count is a multiple of 1,024, the others' is not."""
    single_end = name.startswith("se")
    n = FRONT_SIZES[name]
    pool = front_pool(single_end)
    rng = _rng(9110 + len(name) + n % 97)
    pick = rng.integers(0, len(pool.pairs), n)
    mid = n // 2 - 311
    for a in (0, mid, n - DEAD_RUN):
        pick[a:a + DEAD_RUN] = pool.dead[rng.integers(0, len(pool.dead), DEAD_RUN)]
    free = np.concatenate([np.arange(DEAD_RUN, mid), np.arange(mid + DEAD_RUN, n - DEAD_RUN)])
    m = int(np.sum(pool.status[pick] >= fm.COMBINED))
    want_multiple = name == "se_1025"
    extra = m % LEN_GROUP if want_multiple else (1 if m % LEN_GROUP == 0 else 0)
    if extra:                                            # that many survivors, anywhere, become dead reads
        live = free[pool.status[pick[free]] >= fm.COMBINED]
        kill = rng.choice(live, extra, replace=False)
        pick[kill] = pool.dead[rng.integers(0, len(pool.dead), extra)]
    return pool, pick, front_assemble(pool, pick), single_end


def front_block_sums(pool, pick, e):
    """[3][blocks]: survivors, bytes and exceptions of every block of 256 input reads."""
    alive = pool.status[pick] >= fm.COMBINED
    nbytes = np.zeros(len(pick), np.int64)
    nbytes[e.src] = np.diff(e.offsets)
    nexc = np.zeros(len(pick), np.int64)
    read_of_exc = np.searchsorted(e.offsets, e.packed.exc_pos, side="right") - 1
    np.add.at(nexc, e.src[read_of_exc], 1)
    return [block_sums(v, FRONT_BLOCK) for v in (alive, nbytes, nexc)]


# =============================================================================================
# 2. The demux packer (nw_demux.hip): 256 dwords = 4,096 gathered positions a block
# =============================================================================================

DEMUX_BLOCK = 256 * 16     # kPackBlk dwords of 16 positions: nw_demux.hip:325
DEMUX_K, DEMUX_MIN_HITS = 16, 2
# sizes at which the last working scan thread's share is cut to one block: 1,059 blocks at 2 a
# thread, 2,116 blocks at 3 a thread (tests/test_scan_geometry_cases.py holds them to that)
DEMUX_SIZES = {"per2": 31520, "per3": 63080}
CLEAN_GROUP, FIRST_EXC_GROUP = 3, 2
_EXC_BYTES = np.frombuffer(b"NNNnRYKM-", np.uint8)


@functools.lru_cache(maxsize=None)
def demux_amplicons():
    rng = _rng(9201)
    return tuple(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 420)].tobytes() for _ in range(6))


@functools.lru_cache(maxsize=None)
def demux_pool():
    """1,850 reads: 300 pieces of 100-180 bases of each of 6 amplicons on both strands, a
    substitution or two in half of them, exceptions (N, IUPAC codes, a dash) in a third of those
    of every amplicon but CLEAN_GROUP's, and 50 unrelated reads; then three placed ones.
    ``which`` / ``strand`` are tests/demux_model.py's."""
    rng = _rng(9202)
    amps = demux_amplicons()
    reads = []
    for g, amp in enumerate(amps):
        for _ in range(300):
            L = int(rng.integers(100, 181))
            s = int(rng.integers(0, len(amp) - L + 1))
            a = np.frombuffer(amp[s:s + L], np.uint8).copy()
            if rng.random() < 0.5:
                for p in rng.integers(0, L, int(rng.integers(1, 3))):
                    a[p] = b"ACGT"[(b"ACGT".index(a[p]) + 1) % 4]
            if g != CLEAN_GROUP and rng.random() < 0.33:
                for p in rng.integers(0, L, int(rng.integers(1, 4))):
                    a[p] = rng.choice(_EXC_BYTES)
            r = a.tobytes()
            reads.append(dm.revcomp(r) if rng.random() < 0.5 else r)
    for _ in range(50):
        reads.append(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(rng.integers(100, 181)))].tobytes())
    placed = len(reads)
    reads.append(amps[0][5:130][:7] + b"N" + amps[0][13:130])                      # group 0, an exception early on
    reads.append(dm.revcomp(b"N" + amps[FIRST_EXC_GROUP][41:180]))                 # gathers to N first
    reads.append(amps[5][200:330] + b"R")                                          # group 5, an exception last
    want = dm.demultiplex(list(amps), reads, k=DEMUX_K, min_hits=DEMUX_MIN_HITS)
    which, strand = np.array(want["which"], np.int32), np.array(want["strand"], np.uint8)
    oriented = [dm.revcomp(r) if s else r for r, s in zip(reads, strand)]
    return types.SimpleNamespace(reads=reads, which=which, strand=strand, inputs=Pool(reads), oriented=Pool(oriented),
                                 placed=placed)


def demux_assemble(pool, pick):
    """Everything nwd_assign + nwd_pack + nwd_fetch_packed return for the pool items ``pick``."""
    pick = np.asarray(pick, np.int64)
    which, strand = pool.which[pick], pool.strand[pick]
    hit = np.flatnonzero(which >= 0)
    order = hit[np.argsort(which[hit], kind="stable")].astype(np.int64)
    group_offsets = np.zeros(len(demux_amplicons()) + 1, np.int64)
    np.cumsum(np.bincount(which[hit], minlength=len(demux_amplicons())), out=group_offsets[1:])
    text, text_offsets = pool.oriented.take(pick[order])
    host = pack_2bit(text, text_offsets, nthreads=1)
    nbytes = (int(text_offsets[-1]) + 3) // 4
    group_exc = np.searchsorted(host.exc_pos, text_offsets[group_offsets], side="left").astype(np.int64)
    return types.SimpleNamespace(
        which=which, strand=np.where(which >= 0, strand, 0).astype(np.uint8), group_offsets=group_offsets, order=order,
        text=text, text_offsets=text_offsets, lens=np.diff(text_offsets).astype(np.uint16), packed=host.packed[:nbytes],
        exc_pos=host.exc_pos, exc_byte=host.exc_byte, group_exc=group_exc, n_exc=len(host.exc_pos))


@functools.lru_cache(maxsize=None)
def demux_case(name):
    """(pool, pick, expected): the first read is group 0's with an early exception, the second the
    first of FIRST_EXC_GROUP and gathers to an N first, the last is group 5's and ends in one."""
    pool = demux_pool()
    n = DEMUX_SIZES[name]
    rng = _rng(9210 + n % 89)
    pick = rng.integers(0, pool.placed, n)
    pick[0], pick[1], pick[-1] = pool.placed, pool.placed + 1, pool.placed + 2
    return pool, pick, demux_assemble(pool, pick)


def demux_block_sums(e):
    """Exceptions of every block of 4,096 gathered positions."""
    blocks = ((int(e.text_offsets[-1]) + 15) // 16 + 255) // 256              # nw_demux.hip:968-969
    return np.bincount(e.exc_pos // DEMUX_BLOCK, minlength=blocks).astype(np.int64)


# =============================================================================================
# 3. The region extractor and the region packer (nw_regions.hip)
# =============================================================================================

REGION_BLOCK = 256         # kBlk records a block: nw_regions.hip:89
REGION_PACK_BLOCK = 256 * 16    # kPackBlk dwords of 16 positions: nw_regions.hip:520, 1199
REGION_RANK_BLOCK = 256 * 32    # kRankBlk mask words of 32 positions: nw_regions.hip:521, 1117
# 262,145 + 77 and 150 more, so that both uses of the packer's scan end in a share cut to one
# block: 2,680 blocks at 3 a thread, 1,341 rank sums at 2 a thread
REGION_RECORDS = 262145 + 77 + 150
REGION_REFS = [("chrA", 5000), ("chrB", 5000), ("chrC", 5000)]
REGION_ANCHORS = (100, 400, 700, 1000)
# per reference: a region at every anchor and one that overlaps the first (a record can hit both)
REGION_TABLE = [(ref, a, a + 34 + (a // 100) % 4) for ref in range(3) for a in REGION_ANCHORS] + \
               [(ref, 104, 141) for ref in range(3)]
REGION_CLEAN = (1, 700)    # the records at this anchor carry no non-ACGT base: its region packs without exceptions
REGION_NO_HIT_RUN = 1500
DISCOVER_MIN_READS = 300
_NAME = b"r%06d"
_NON_ACGT = "NNNRYMKSW"


def _cigar_shapes(rng):
    """One CIGAR of 40-60 M bases: plain, soft-clipped, with an insertion, a deletion, or all."""
    m = int(rng.integers(40, 61))
    a = int(rng.integers(8, m - 8))
    kind = int(rng.integers(0, 6))
    if kind == 0:
        return "%dM" % m
    if kind == 1:
        return "%dS%dM" % (int(rng.integers(1, 6)), m)
    if kind == 2:
        return "%dM%dI%dM" % (a, int(rng.integers(1, 4)), m - a)
    if kind == 3:
        return "%dM%dD%dM" % (a, int(rng.integers(1, 4)), m - a)
    if kind == 4:
        return "%dM%dS" % (m, int(rng.integers(1, 5)))
    b = int(rng.integers(4, m - a - 3))
    return "%dS%dM%dI%dM%dD%dM%dS" % (int(rng.integers(1, 4)), a, int(rng.integers(1, 3)), b, int(rng.integers(1, 3)),
                                      m - a - b, int(rng.integers(1, 4)))


@functools.lru_cache(maxsize=None)
def region_pool():
    """312 mapped records, 26 at every anchor of every reference (pos 0-3 before the anchor, one of
    _cigar_shapes, about 2 % of the bases a non-ACGT nibble but at REGION_CLEAN, every third on the
    reverse strand),
    6 records far from every region, and the records that are never a hit: flag 4, no reference,
    no sequence, no qualities.  Outcomes: tests/regions_model.py and tests/genome_regions_model.py
    on each record alone."""
    from tests import genome_regions_model as gm
    from tests import regions_cases as rc
    from tests import regions_model as rm

    rng = _rng(9301)
    items = []

    def add(ref, pos, cigar, **kw):
        n = sum(k for k, op in rm.parse_cigar(cigar) if op in "MIS=X")
        seq = "".join("ACGT"[x] for x in rng.integers(0, 4, n))
        if not kw.pop("clean", False):
            seq = "".join(_NON_ACGT[int(rng.integers(0, len(_NON_ACGT)))] if rng.random() < 0.02 else c for c in seq)
        qual = rng.integers(0, 42, n).tolist()
        seq = kw.pop("seq", seq)
        items.append(rc.rec(_NAME % 0, ref, pos, cigar, seq=seq, qual=None if seq == "*" else qual, **kw))

    for ref in range(3):
        for a in REGION_ANCHORS:
            for j in range(26):
                add(ref, a - int(rng.integers(0, 4)), _cigar_shapes(rng), flag=16 if j % 3 == 0 else 0,
                    clean=(ref, a) == REGION_CLEAN)
    for j in range(6):
        add(j % 3, 3000 + 7 * j, "50M")
    live = len(items)
    add(0, 100, "50M", flag=4)
    add(1, 400, "45M5S", flag=4 | 16)
    add(-1, 100, "50M")
    add(2, 700, "50M", seq="*")
    add(1, 100, "52M", noqual=True)
    weight = np.ones(live)
    weight[::7] = 0.03                                   # rare records: their spans stay under min_reads
    hit = np.zeros((len(items), len(REGION_TABLE)), bool)
    out, dropped, key = [], np.zeros(len(items), np.int64), []
    for i, r in enumerate(items):
        w = rm.extract([r], REGION_TABLE)
        out.append([h[0][1:5] if h else None for h in w["hits"]])
        hit[i] = [bool(h) for h in w["hits"]]
        dropped[i] = w["n_no_seq"]
        d = gm.discover([r])
        key.append(d["regions"][0] if d["regions"] else None)
    templates = [rc.record_bytes(r) for r in items]
    cut = 36 + len(_NAME % 0)                             # block_size, the 32 fixed bytes, the name
    return types.SimpleNamespace(
        items=items, live=live, weight=weight / weight.sum(), hit=hit, out=out, dropped=dropped, key=key,
        head=[t[:36] for t in templates], tail=[t[cut:] for t in templates],
        no_hit=np.arange(live, len(items)), flag=np.array([r["flag"] for r in items]),
        has_seq=np.array([rm.has_seq(r) for r in items]),
        takes_part=np.array([gm.takes_part(r) for r in items]))


def region_records(pool, pick, base=0):
    """The records as the models take them (for the slow model on a few thousand)."""
    return [dict(pool.items[p], name=_NAME % (base + i)) for i, p in enumerate(pick)]


def region_bam(pool, pick, base=0):
    """The BAM of these records in stored BGZF blocks: tests/regions_cases.py's record bytes per
    pool record with the record's own name in place."""
    from tests import regions_cases as rc

    body = b"".join(pool.head[p] + _NAME % (base + i) + pool.tail[p] for i, p in enumerate(pick.tolist()))
    return rc.bgzf(rc.bam_plain(REGION_REFS, []) + body, stored=True)


def region_extract_assemble(pool, pick, base=0):
    """tests/regions_model.extract's dict for the records ``pick`` against REGION_TABLE."""
    hits = []
    for g in range(len(REGION_TABLE)):
        members = np.flatnonzero(pool.hit[pick, g]).tolist()
        hits.append([(i,) + pool.out[pick[i]][g] + (_NAME % (base + i) + b"_%d" % (k + 1),) for k, i in enumerate(members)])
    return {"hits": hits, "n_no_seq": int(pool.dropped[pick].sum())}


def region_discover_assemble(pool, pick, min_reads, base=0):
    """tests/genome_regions_model.discover's dict for the records ``pick``."""
    from tests import regions_model as rm

    by_key = {}
    for i, p in enumerate(pick.tolist()):
        if pool.key[p] is not None:
            by_key.setdefault(pool.key[p], []).append(i)
    regions = sorted(by_key)
    hits, strands = [], []
    for k in regions:
        src = by_key[k] if len(by_key[k]) >= min_reads else []
        rows = []
        for i in src:
            r = pool.items[pick[i]]
            rows.append((i, 0, len(r["seq"]), r["seq"].encode(), rm.qual_text(r["qual"]).encode(), _NAME % (base + i)))
        hits.append(rows)
        strands.append([b"-" if pool.flag[pick[i]] % 32 >= 16 else b"+" for i in src])
    tp = pool.takes_part[pick]
    return {"regions": regions, "n_records": [len(by_key[k]) for k in regions], "hits": hits, "strand": strands,
            "n_no_seq": int(np.sum(tp & ~pool.has_seq[pick])), "n_aligned": int(np.sum((pool.flag[pick] & 0x904) == 0)),
            "n_kept": sum(map(len, by_key.values()))}


def region_major(want):
    """(text, text_offsets, region_offsets, src, st, en) of a model dict: the hits region by region."""
    flat = [h for g in want["hits"] for h in g]
    off = np.zeros(len(flat) + 1, np.int64)
    np.cumsum([len(h[3]) for h in flat], out=off[1:])
    roff = np.zeros(len(want["hits"]) + 1, np.int64)
    np.cumsum([len(g) for g in want["hits"]], out=roff[1:])
    text = np.frombuffer(b"".join(h[3] for h in flat), np.uint8)
    return (text, off, roff, np.array([h[0] for h in flat], np.int64), np.array([h[1] for h in flat], np.int32),
            np.array([h[2] for h in flat], np.int32))


@functools.lru_cache(maxsize=None)
def region_case():
    """(pool, pick): REGION_RECORDS records of one chunk, REGION_NO_HIT_RUN records that are never
    a hit in the middle (flag 4, no reference, no sequence, no qualities), the rare records rare."""
    pool = region_pool()
    rng = _rng(9310)
    pick = rng.choice(pool.live, REGION_RECORDS, p=pool.weight)
    a = 3 * REGION_RECORDS // 5
    pick[a:a + REGION_NO_HIT_RUN] = pool.no_hit[rng.integers(0, len(pool.no_hit), REGION_NO_HIT_RUN)]
    return pool, pick


@functools.lru_cache(maxsize=None)
def region_expected():
    """(extract's dict, its region-major arrays, the host packer's PackedReads of that text,
    discover's dict) of region_case()."""
    pool, pick = region_case()
    want = region_extract_assemble(pool, pick)
    major = region_major(want)
    return want, major, pack_2bit(major[0], major[1], nthreads=1), region_discover_assemble(pool, pick, DISCOVER_MIN_READS)


def region_block_sums(pool, pick, want, major, packed, found):
    """The four scans' inputs: hits per 256 records (extract), emitted records per 256 records
    (discover), exceptions per 4,096 packed positions, mask bits per 8,192 positions and the empty
    last block of nw_regions.hip:1117."""
    total = int(major[1][-1])
    emitted = np.zeros(len(pick), np.int64)
    for g in found["hits"]:
        emitted[[h[0] for h in g]] = 1
    pack_blocks = ((total + 15) // 16 + 255) // 256                           # nw_regions.hip:1116, 1184, 1199
    rank_blocks = ((total + 31) // 32 + 255) // 256 + 1                       # nw_regions.hip:1117
    return {"extract": block_sums(pool.hit[pick].sum(axis=1), REGION_BLOCK), "discover": block_sums(emitted, REGION_BLOCK),
            "pack": np.bincount(packed.exc_pos // REGION_PACK_BLOCK, minlength=pack_blocks).astype(np.int64),
            "rank": np.bincount(packed.exc_pos // REGION_RANK_BLOCK, minlength=rank_blocks).astype(np.int64)}


# =============================================================================================
# 4. The allele grouper (nw_alleles.hip): tiles of 2,048 reads, 1,024 tiles a step of the scan
# =============================================================================================

TILE = 2048                # kTile, nw_alleles.hip:45
TILES_PER_STEP = 1024      # tile_scan_kernel's block, nw_alleles.hip:183-185
ALLELE_SIZES = {"two_steps": 1024 * TILE + 1, "three_steps": 2 * 1024 * TILE + 77}
ALLELE_FIRSTS = {"two_steps": 10, "three_steps": 5}     # a tile is given 0..this many first reads: about 5,000 a case
QUIET_TILES = (700, 705)   # no read of these tiles is planned as a group's first
ALLELE_AMPLICON = "ACGTTGCAAGGCTTAC"


@functools.lru_cache(maxsize=None)
def allele_case(name):
    """(pool, pick, keep): every tile is given 0 to ALLELE_FIRSTS[name] reads that show a pool
    sequence for the first time (none in QUIET_TILES, the batch's last read always one), every
    other read repeats a sequence already shown.  So the groups' first reads are spread over all tiles, past tile 1,023
    too, and neighbouring tile sums differ.  In three_steps half of the pool is first shown after
    read 2,097,152; two_steps has one read there (tile 1,024 holds nothing else), and it is a
    group's first, so emit_kernel takes its base from tile_off[1024].  keep: 0, 1 and 2 without
    a period, the last read kept."""
    n = ALLELE_SIZES[name]
    rng = _rng(9400 + n % 83)
    tiles = (n + TILE - 1) // TILE
    most = ALLELE_FIRSTS[name]
    per_tile = rng.integers(0, most + 1, tiles)
    per_tile[QUIET_TILES[0]:QUIET_TILES[1]] = 0
    per_tile[0] = max(per_tile[0], 1)
    per_tile[tiles - 1] = 0
    slot = TILE // most
    firsts = [t * TILE + j * slot + int(rng.integers(0, slot)) for t in range(tiles) for j in range(per_tile[t])]
    firsts[0] = 0
    firsts = np.array(sorted(set(firsts) | {n - 1}), np.int64)
    P = len(firsts)
    seqs = set()
    while len(seqs) < P:
        seqs.add(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(rng.integers(8, 17)))].tobytes())
    pool = Pool(sorted(seqs))
    shown = np.searchsorted(firsts, np.arange(n), side="right")        # sequences shown up to and with read r
    pick = (rng.random(n) * shown).astype(np.int64)
    pick[firsts] = np.arange(P)
    keep = rng.choice(np.array([0, 1, 2], np.uint8), n, p=[0.3, 0.4, 0.3])
    keep[-1] = 2
    return pool, pick, keep


def allele_groups(pick, keep=None):
    """(first, count, group_of_read): np.unique over the kept reads' pool indices, the groups in
    ascending order of their first read."""
    kept = np.arange(len(pick)) if keep is None else np.flatnonzero(keep)
    _, idx, inv, cnt = np.unique(pick[kept], return_index=True, return_inverse=True, return_counts=True)
    by_first = np.argsort(idx, kind="stable")
    rank = np.empty(len(by_first), np.int64)
    rank[by_first] = np.arange(len(by_first))
    gor = np.full(len(pick), -1, np.int32)
    gor[kept] = rank[inv]
    return kept[idx[by_first]].astype(np.int64), cnt[by_first].astype(np.int64), gor


def allele_tile_sums(first, n):
    """Groups' first reads per tile: what tile_sum_kernel leaves for the scan."""
    return np.bincount(first // TILE, minlength=(n + TILE - 1) // TILE).astype(np.int64)


def allele_table_arrays(pool, pick):
    """The aligner's device arrays for these reads against ALLELE_AMPLICON (16 bases), one M run
    over the read and, where the read is shorter, a Y run over the rest of the amplicon:
    (ops, ops_off, stats, results) with results a function of the read's bytes."""
    la = len(ALLELE_AMPLICON)
    lens = pool.lens[pick]
    nruns = 1 + (lens < la)
    ops_off = np.zeros(len(pick) + 1, np.int64)
    np.cumsum(nruns, out=ops_off[1:])
    ops = np.zeros(int(ops_off[-1]) + 1, np.uint32)
    ops[ops_off[:-1]] = lens.astype(np.uint32)                              # M = 0 << 28
    short = lens < la
    ops[ops_off[:-1][short] + 1] = (2 << 28) | (la - lens[short]).astype(np.uint32)   # Y
    ops[-1] = 0xDEADBEEF
    stats = np.full((len(pick), 8), -7, np.int32)
    stats[:, 0] = la
    rr = np.stack([pick % 3, pick % 11, pick % 7, la - lens], axis=1).astype(np.int32)
    return ops, ops_off, stats, rr


def allele_table_rows(pool, pick, first):
    """[groups][2][16]: the aligned-read row (the read, then '-') and the reference row."""
    la = len(ALLELE_AMPLICON)
    rows = np.empty((len(first), 2, la), np.uint8)
    rows[:, 1, :] = np.frombuffer(ALLELE_AMPLICON.encode(), np.uint8)
    item = pick[first]
    body = pool.mat[item][:, :la]
    rows[:, 0, :] = np.where(np.arange(la) < pool.lens[item, None], body, ord("-"))
    return rows
