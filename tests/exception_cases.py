"""Reads with exception bytes (every byte that is not ACGTacgt: N, IUPAC codes, '-', ...) at the places
where the packed aligner does position arithmetic on them.  TEST INFRASTRUCTURE ONLY: one generator for
tests/test_exception_cases.py (which holds it to its conditions on the CPU) and tests/test_gpu_exceptions.py.

``batch(seed)`` -> Batch: a 250-bp amplicon, its HDR amplicon, 6144 reads and one class label per read.
Every even read, and the reads on both sides of every place a chunk or block boundary can fall, carry at
least one exception byte; the odd reads are plain neighbours (exact copies, one-substitution reads, indel
reads, HDR reads), so a store that spills into the next read shows up there.

Classes (LABELS): a label starting with "x_" marks an exception read, "p_" a plain one.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from crispresso_amd import synth

N_READS = 6144
LA = 250
HDR_START, HDR_LEN = 120, 10          # synth.hdr_amplicon's block
# a chunk boundary can fall at a multiple of these: CRISPR_NW_CHUNK=1024 cuts 6144 reads at multiples of
# 1024, CRISPR_NW_CHUNK=257 into 24 equal chunks (multiples of 256: plan_chunks evens the chunks out);
# 257 itself as the switch's literal value; 256 is also classify's block, 64 its wavefront
BOUNDARIES = (64, 256, 257, 1024)
# the pooled test's groups (four amplicons): cut at multiples of 257, so that its chunks under
# CRISPR_NW_CHUNK=257 are not aligned to classify's blocks of 256 reads
POOLED_GROUPS = (0, 1542, 3084, 4626, N_READS)

ACGT = b"ACGTacgt"
OTHER_BYTES = (b"R", b"Y", b"-", b"n", b"*", b"\xe9")

PLAIN = ("p_exact", "p_sub1", "p_del", "p_ins", "p_hdr")
SPECIAL = (
    "x_first_byte", "x_last_byte", "x_res16",
    "x_nn_dword", "x_run5", "x_run17", "x_all_n",
    "x_pair_last", "x_pair_first",
    "x_byte_R", "x_byte_Y", "x_byte_dash", "x_byte_n", "x_byte_star", "x_byte_high",
    "x_amp_n_at_a", "x_amp_n_at_c", "x_hdr_n_at_a_block", "x_hdr_n_at_a_outside",
    "x_sub1_n", "x_sub2_n", "x_sub3_n", "x_indel1_n",
    "x_len1", "x_len2", "x_len3", "x_len_mod0", "x_len_mod1", "x_len_mod2", "x_len_mod3", "x_longer",
)
FILL = ("x_fill_exact", "x_fill_sub1", "x_fill_del", "x_fill_hdr")
LABELS = PLAIN + SPECIAL + FILL


@dataclass
class Batch:
    amp: str
    hdr: str
    reads: list            # bytes per read
    labels: list           # one of LABELS per read
    buf: np.ndarray        # uint8, the reads end to end
    off: np.ndarray        # int64 [n + 1]

    @property
    def n(self) -> int:
        return len(self.reads)

    def has_exception(self) -> np.ndarray:
        return np.array([any(b not in ACGT for b in r) for r in self.reads], bool)


def exceptions_of(buf: np.ndarray, base: int = 0):
    """(positions ascending, bytes) of the bytes of `buf` not in ACGTacgt; positions from `base`."""
    is_exc = ~np.isin(buf, np.frombuffer(ACGT, np.uint8))
    pos = np.flatnonzero(is_exc).astype(np.int64)
    return pos + base, buf[pos]


def plan_sizes(n: int, chunk: int) -> list:
    """The chunk sizes the host plans for a call over n reads of one amplicon (plan_chunks: ramp parts of
    chunk / 4 and chunk / 2 at both ends when they hold 1024 reads or more, even chunks in between)."""
    if n <= chunk:
        return [n]
    head, left = [], n
    for part in (chunk // 4, chunk // 2):
        if part >= 1024 and left > 2 * (part + chunk):
            head.append(part)
            left -= 2 * part
    mid = (left + chunk - 1) // chunk
    return head + [left // mid + (1 if q < left % mid else 0) for q in range(mid)] + head[::-1]


def _sub(seq: bytearray, i: int, rng) -> None:
    seq[i] = b"ACGT"[(b"ACGT".index(seq[i]) + int(rng.integers(1, 4))) % 4]


def _amplicons(seed: int):
    """A 250-bp amplicon whose HDR amplicon has an A inside and outside the block, and that has an A and a C."""
    s = 7000 + 10 * seed
    while True:
        amp = synth.random_amplicon(LA, s)
        hdr = synth.hdr_amplicon(amp)
        if "A" in hdr[HDR_START:HDR_START + HDR_LEN] and "A" in hdr[:HDR_START] and "A" in amp and "C" in amp:
            return amp, hdr
        s += 1


@functools.lru_cache(maxsize=None)
def batch(seed: int, n: int = N_READS) -> Batch:
    rng = np.random.Generator(np.random.PCG64(9000 + seed))
    amp, hdr = _amplicons(seed)
    A, H = amp.encode(), hdr.encode()

    def put(seq, i, b=b"N"):
        s = bytearray(seq)
        s[i:i + len(b)] = b
        return s

    def interior():
        return int(rng.integers(20, LA - 40))

    def deletion(seq, k=3):
        p = interior()
        return bytearray(seq[:p] + seq[p + k:])

    def insertion(seq, k=2):
        p = interior()
        return bytearray(seq[:p] + bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, k)) + seq[p:])

    def subs(seq, k):
        s = bytearray(seq)
        for i in rng.choice(np.arange(10, LA - 10), size=k, replace=False):
            _sub(s, int(i), rng)
        return s

    def n_clear_of(s, ref):
        """one N in s at an interior place where it agrees with ref (the edit stays what it was)"""
        while True:
            i = interior()
            if i < min(len(s), len(ref)) and s[i] == ref[i]:
                return put(s, i)

    def at_residue(seq, off, res, mod, lo=16):
        return lo + (res - off - lo) % mod

    # the special reads: label -> maker(offset of the read in the batch)
    def special(label, off, k=0):
        if label == "x_first_byte":
            return put(A, 0)
        if label == "x_last_byte":
            return put(A, LA - 1)
        if label == "x_res16":      # one N at a batch position of residue k mod 16
            return put(A, at_residue(A, off, k, 16))
        if label == "x_nn_dword":   # NN at batch positions 4 q + 3, 4 q + 4
            return put(A, at_residue(A, off, 3, 4), b"NN")
        if label == "x_run5":
            return put(A, interior(), b"N" * 5)
        if label == "x_run17":
            return put(A, interior(), b"N" * 17)
        if label == "x_all_n":
            return bytearray(b"N" * LA)
        if label == "x_pair_last":
            return put(A, LA - 1)
        if label == "x_pair_first":
            return put(A, 0)
        if label.startswith("x_byte_"):
            b = OTHER_BYTES[("R", "Y", "dash", "n", "star", "high").index(label[7:])]
            return put(A, interior(), b)
        if label == "x_amp_n_at_a":
            return put(A, amp.index("A", 30))
        if label == "x_amp_n_at_c":
            return put(A, amp.index("C", 30))
        if label == "x_hdr_n_at_a_block":
            return put(H, hdr.index("A", HDR_START))
        if label == "x_hdr_n_at_a_outside":
            return put(H, hdr.index("A", 30))
        if label in ("x_sub1_n", "x_sub2_n", "x_sub3_n"):
            return n_clear_of(subs(A, int(label[5])), A)
        if label == "x_indel1_n":
            p = interior()
            return put(A[:p] + A[p + 3:], 10)
        if label == "x_len1":
            return bytearray(b"N")
        if label == "x_len2":
            return bytearray(b"NA") if k % 2 else bytearray(A[:1] + b"N")
        if label == "x_len3":
            return bytearray(A[:1] + b"N" + A[2:3])
        if label.startswith("x_len_mod"):   # a deletion leaving a length of every residue mod 4, one N
            want = int(label[9:])
            return put(deletion(A, (LA - want) % 4 + 4), 60 + k)
        if label == "x_longer":
            return put(insertion(A, 7), 70)
        raise KeyError(label)

    def fill(label):
        if label == "x_fill_exact":
            return put(A, int(rng.integers(0, LA)))
        if label == "x_fill_sub1":
            return n_clear_of(subs(A, 1), A)
        if label == "x_fill_del":
            s = deletion(A, int(rng.integers(1, 8)))
            return put(s, int(rng.integers(0, len(s))))
        if label == "x_fill_hdr":
            return put(H, int(rng.integers(0, LA)))
        raise KeyError(label)

    def plain(label):
        if label == "p_exact":
            return bytearray(A)
        if label == "p_sub1":
            return subs(A, 1)
        if label == "p_del":
            return deletion(A, int(rng.integers(1, 8)))
        if label == "p_ins":
            return insertion(A, int(rng.integers(1, 5)))
        if label == "p_hdr":
            return bytearray(H)
        raise KeyError(label)

    # reads that must carry an exception wherever they fall: the first and the last, and both sides of
    # every boundary
    must = {0, n - 1}
    first_n, last_n = set(), set()   # at the chunk boundaries: N at the read's first / last byte
    for m in BOUNDARIES:
        for b in range(m, n, m):
            must.update((b - 1, b))
            if m != 64:
                last_n.add(b - 1)
                first_n.add(b)
    if n == N_READS:   # the chunks of the pooled groups
        for g0, g1 in zip(POOLED_GROUPS[:-1], POOLED_GROUPS[1:]):
            for b in (g0 + np.cumsum(plan_sizes(g1 - g0, 257))[:-1]).tolist():
                must.update((b - 1, b))
                last_n.add(b - 1)
                first_n.add(b)
    # the special classes on even reads spread over the batch (x_pair_* on two adjacent reads), every one
    # several times so that each lands in several blocks
    plan = {}
    queue = [(lab, k) for k in range(16) for lab in SPECIAL if lab not in ("x_pair_last", "x_pair_first")
             and (lab == "x_res16" or k < 4)]
    slots = [i for i in range(2, n - 2, 2) if i not in must and i + 1 not in must and i - 1 not in must]
    step = max(1, len(slots) // (len(queue) + 8))
    for q, item in enumerate(queue):
        plan[slots[q * step]] = item
    pair_slots = slots[len(queue) * step::step][:8]
    for i in pair_slots:
        plan[i] = ("x_pair_last", 0)
        plan[i + 1] = ("x_pair_first", 0)
    reads, labels, off = [], [], 0
    for i in range(n):
        if i in plan:
            lab, k = plan[i]
            r = special(lab, off, k)
        elif i in first_n or i in last_n:
            # beside a chunk boundary: the exceptions meet across it (last byte | first byte)
            lab = "x_pair_first" if i in first_n else "x_pair_last"
            r = bytearray(A)
            if i in first_n:
                r[0:1] = b"N"
            if i in last_n:
                r[LA - 1:LA] = b"N"
        elif i in must or i % 2 == 0:
            lab = FILL[int(rng.integers(0, len(FILL)))]
            r = fill(lab)
        else:
            lab = PLAIN[(i // 2) % len(PLAIN)]
            r = plain(lab)
        reads.append(bytes(r))
        labels.append(lab)
        off += len(r)
    offs = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=offs[1:])
    buf = np.frombuffer(b"".join(reads), np.uint8).copy()
    return Batch(amp, hdr, reads, labels, buf, offs)


def hamming(a: bytes, b: bytes) -> int:
    return int((np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8)).sum())


def one_indel_of(read: bytes, ref: bytes, kmax: int = 10) -> bool:
    """read is ref with one run of 1 .. kmax residues deleted or inserted"""
    k = abs(len(read) - len(ref))
    if not 1 <= k <= kmax:
        return False
    s, l = (read, ref) if len(read) < len(ref) else (ref, read)
    p = 0
    while p < len(s) and s[p] == l[p]:
        p += 1
    return s[p:] == l[p + k:]


def certifiable(b: Batch, ref: str, known: str | None) -> int:
    """How many reads WITHOUT an exception byte classify's certificates could finish against `ref`: copies
    of it, reads of its length with up to three substitutions, one-indel reads (up to 10 residues), and
    copies of `known`.  (The batch holds no window reads.)  No exception read may be among the certified:
    the certified count of a run can never exceed this."""
    R = ref.upper().encode()
    K = known.upper().encode() if known else None
    exc = b.has_exception()
    total = 0
    for r, x in zip(b.reads, exc):
        if x:
            continue
        u = r.upper()
        if (len(u) == len(R) and hamming(u, R) <= 3) or one_indel_of(u, R) or (K is not None and u == K):
            total += 1
    return total
