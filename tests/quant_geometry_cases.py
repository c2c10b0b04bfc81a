"""Seeded read batches for the quantifier's launch geometries (tests/test_gpu_quant_geometry.py,
tests/test_quant_geometry_cases.py): every shape nw_quant.hip chooses from the amplicon length and
the row stride, 300 to 4,952 bp.

full(La)   C2 parity-mix reads of the whole amplicon with the overhangs, lowercase stretches, IUPAC
           codes and '-' bytes of test_gpu_quant.odd_reads.  The longest read is exactly La + 40, so
           the aligner's stride is (2 La + 40 + 15) & ~15.
short(La)  the WGS shape: reads of 100 to 300 bases cut from a region of La bases at offsets 0,
           La - len and random ones, each with the mix's edits.  The longest read is exactly 300.

Planted on top of both, so that no regime depends on the mix by chance (PLANTED kinds, KIND_MIN
reads each):

  subs_over  9 to 20 substitutions (more than quant_lanes' kQS = 8)      subs_8  exactly 8
  dels_3     3 separate deletions (more than kQD = 2)                    dels_2  exactly 2
  ins_3      3 separate insertions (more than kQI = 2)                   ins_2   exactly 2
  dash       one '-' byte (and two substitutions: one mismatch in 2,000 columns prints 100.0)

A deletion is a run of '-' in align_seq, so a short read's end gaps count: a read cut from inside the
region has two before anything is planted, and gets one more deletion for dels_3 and none for dels_2.

Then, for every multiple m of 256 alignment columns the length has, a deletion and an insertion that
end at m, start at m and straddle m ("end", "start", "over"); a deletion at amplicon position 0 and
one ending at La - 1; insertions before the first and after the last base.

Batch sizes: 1024 reads to 1024 bp, 256 to 2100 bp, 64 above (the aligner above 1024 bp is the
multi-wave exact kernel, one workgroup a read, and the Python oracle walks every column).  Batches
of 256 reads and more give each kind reads of its own and each (multiple, relation) a read of its
own, plus reads that carry one relation at every multiple.  Below 256 reads there is no room for
that: the over-capacity kinds share their reads, so do the at-capacity kinds, and the boundary edits
are one read a relation with every multiple in it (full), or one deletion read and one insertion
read a multiple with the relation cycling over the multiples (short: a 300-base read covers one
multiple).  quant_lanes is off at every length that has fewer than 256 reads, so there the kinds
only vary the counts, not the path.

conditions(case) restates what the batches must hold, from the CPU oracles alone."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np

from crispresso_amd import synth
from oracle import oracle_py
from oracle import quant_oracle as qo
from tests.test_gpu_quant import PARAMS, make_params, odd_reads

PLANTED = ("subs_over", "subs_8", "dels_3", "dels_2", "ins_3", "ins_2", "dash")
OVER = ("subs_over", "dels_3", "ins_3", "dash")          # what quant_lanes leaves to the row path
KIND_MIN = 10
PAD = 40
SHORT_MAX = 300
RELATIONS = ("end", "start", "over")


def batch_size(La: int) -> int:
    return 1024 if La <= 1024 else 256 if La <= 2100 else 64


def full_stride(La: int) -> int:
    return (2 * La + PAD + 15) & ~15


def short_stride(La: int) -> int:
    return (La + SHORT_MAX + 15) & ~15


@dataclass
class Case:
    name: str
    amp: str
    reads: List[str]
    kinds: Dict[str, List[int]]                  # planted kind -> read indices
    marks: Dict[tuple, List[int]] = field(default_factory=dict)   # ("del" | "ins", m, relation) -> read indices
    edges: Dict[str, List[int]] = field(default_factory=dict)     # del_first, del_last, ins_first, ins_last
    sr_fixed: Dict[int, float] = field(default_factory=dict)      # read -> score_repaired (HDR / MIXED for certain)

    @property
    def n(self):
        return len(self.reads)

    def packed(self):
        buf = np.frombuffer("".join(self.reads).encode(), np.uint8).copy()
        off = np.r_[0, np.cumsum([len(s) for s in self.reads])].astype(np.int64)
        return buf, off


# ---- edits on a window of the amplicon ----------------------------------------------------------

def _other(rng, *avoid):
    return str(rng.choice([b for b in "ACGT" if b not in avoid]))


def _apply(w: str, edits):
    """edits: (position in w, 'S' | 'D' | 'I' | '-', size); applied from the right so positions hold."""
    s = list(w)
    for pos, op, arg in sorted(edits, reverse=True):
        if op == "S":
            s[pos] = arg
        elif op == "D":
            del s[pos:pos + arg]
        elif op == "I":
            s[pos:pos] = list(arg)
        else:
            s[pos] = "-"
    return "".join(s)


def _insert_text(w, pos, size, rng):
    """Bases that differ from both neighbours of the insertion point: the gap cannot slide."""
    return "".join(_other(rng, w[pos], w[pos - 1]) for _ in range(size))


def kind_read(w: str, n_end: int, want: dict, rng) -> str:
    """w with want["subs"] substitutions, deletions up to want["dels"] runs in all (n_end of them are
    the read's end gaps), want["ins"] insertions and want["dash"] '-' bytes, at evenly spread sites."""
    nsub, ndel = want.get("subs", 0), max(0, want.get("dels", 0) - n_end) if "dels" in want else 0
    nins, ndash = want.get("ins", 0), want.get("dash", 0)
    k = nsub + ndel + nins + ndash
    sites = np.linspace(8, len(w) - 14, k).astype(int) if k > 1 else np.array([len(w) // 2])
    assert k <= 1 or np.diff(sites).min() >= 4, (len(w), k)
    ops = rng.permutation(["S"] * nsub + ["D"] * ndel + ["I"] * nins + ["-"] * ndash)
    edits = []
    for pos, op in zip(sites.tolist(), ops.tolist()):
        if op == "S":
            edits.append((pos, "S", _other(rng, w[pos])))
        elif op == "D":
            edits.append((pos, "D", int(rng.integers(1, 4))))
        elif op == "I":
            edits.append((pos, "I", _insert_text(w, pos, int(rng.integers(1, 4)), rng)))
        else:
            edits.append((pos, "-", None))
    return _apply(w, edits)


KIND_WANT = {
    "subs_over": lambda rng: {"subs": int(rng.integers(9, 21))},
    "subs_8": lambda rng: {"subs": 8},
    "dels_3": lambda rng: {"dels": 3},
    "dels_2": lambda rng: {"dels": 2},
    "ins_3": lambda rng: {"ins": 3},
    "ins_2": lambda rng: {"ins": 2},
    "dash": lambda rng: {"dash": 1, "subs": 2},      # (one mismatch in 2,000 columns prints 100.0: UNMODIFIED)
}
SHARED = {("subs_over", "dels_3", "ins_3", "dash"): lambda rng: {"subs": int(rng.integers(9, 21)), "dels": 3, "ins": 3,
                                                                  "dash": 1},
          ("subs_8", "dels_2", "ins_2"): lambda rng: {"subs": 8, "dels": 2, "ins": 2}}


def _fixed_deletion(amp, m, rel):
    """(start, size) of a deletion that ends at / starts at / straddles amplicon position m and
    cannot slide: the base after it differs from its first, the base before it from its last."""
    for d in range(2, 12):
        for p in ([m - d] if rel == "end" else [m] if rel == "start" else [m - 1, m - 2, m - 3]):
            if rel == "over" and not (p < m < p + d):
                continue
            if p >= 1 and p + d < len(amp) - 1 and amp[p] != amp[p + d] and amp[p - 1] != amp[p + d - 1]:
                return p, d
    raise AssertionError("no fixed deletion at %d" % m)


def _ins_place(m, rel, shift, size=2):
    """(amplicon position, size) of an insertion whose columns end at / start at / straddle column m
    when `shift` inserted bases precede it; the straddling one is a base longer."""
    if rel == "end":
        return m - size - shift, size
    if rel == "start":
        return m - shift, size
    return m - 1 - shift, size + 1


def multiples(La):
    """The multiples of 256 columns with at least 40 bases after them (an edit nearer the end
    would leave a tail the aligner is free not to align)."""
    return list(range(256, La - 40, 256))


# ---- the two shapes -----------------------------------------------------------------------------

def _plant(case: Case, slots: List[int], window, rng):
    """Replace reads at `slots` (popped from its end) with the planted kinds.  window(kind_with_ins)
    -> (offset, length) of the amplicon piece a planted read covers."""
    amp, La, n = case.amp, len(case.amp), case.n

    def put(read, *groups):
        i = slots.pop()
        case.reads[i] = read
        for g in groups:
            g.append(i)
        return i

    def piece():
        off, ln = window()
        return off, amp[off:off + ln], int(off > 0) + int(off + ln < La)

    for k in PLANTED:
        case.kinds[k] = []
    if n >= 256:
        for k in PLANTED:
            for _ in range(KIND_MIN + 2):
                off, w, n_end = piece()
                put(kind_read(w, n_end, KIND_WANT[k](rng), rng), case.kinds[k])
    else:
        for ks, want in SHARED.items():
            for _ in range(KIND_MIN):
                off, w, n_end = piece()
                put(kind_read(w, n_end, want(rng), rng), *[case.kinds[k] for k in ks])
    return put


@functools.lru_cache(maxsize=None)
def full(La: int, n: int = 0) -> Case:
    n = n or batch_size(La)
    seed = 1000 + La
    rng = np.random.Generator(np.random.PCG64(seed))
    amp, buf, off = odd_reads(La, n, seed, PAD)
    reads = [s[:La + PAD] for s in synth.unpack(buf, off)]
    case = Case("full_%d" % La, amp, reads, {})
    slots = rng.permutation(n).tolist()
    put = _plant(case, slots, lambda: (0, La), rng)
    ms = multiples(La)
    for what in ("del", "ins"):
        for rel in RELATIONS:
            for m in ms:
                case.marks[(what, m, rel)] = []
    if n >= 256:            # one edit a read: the lane path's reads
        for m in ms:
            for rel in RELATIONS:
                p, d = _fixed_deletion(amp, m, rel)
                put(_apply(amp, [(p, "D", d)]), case.marks[("del", m, rel)])
                p, s = _ins_place(m, rel, 0)
                put(_apply(amp, [(p, "I", _insert_text(amp, p, s, rng))]), case.marks[("ins", m, rel)])
    for rel in RELATIONS:   # one relation at every multiple in one read: the row path's reads
        put(_apply(amp, [(p, "D", d) for p, d in (_fixed_deletion(amp, m, rel) for m in ms)]),
            *[case.marks[("del", m, rel)] for m in ms])
        edits, shift = [], 0
        for m in ms:
            p, s = _ins_place(m, rel, shift, 1)       # (19 multiples at 4,952 bp: at most 38 bases)
            edits.append((p, "I", _insert_text(amp, p, s, rng)))
            shift += s
        put(_apply(amp, edits), *[case.marks[("ins", m, rel)] for m in ms])
    for k in ("del_first", "del_last", "ins_first", "ins_last"):
        case.edges[k] = []
    junk = lambda k: "".join(rng.choice(list("ACGT"), k))   # noqa: E731
    for _ in range(2 if n >= 256 else 1):
        put(amp[3:La - 4], case.edges["del_first"], case.edges["del_last"])
        put(junk(PAD // 2) + amp + junk(PAD // 2), case.edges["ins_first"], case.edges["ins_last"])
    for _ in range(3):      # a deletion of 6 % prints below 97: MIXED with score_repaired 97
        p = int(rng.integers(La // 4, La // 2))
        case.sr_fixed[put(amp[:p] + amp[p + max(30, La * 6 // 100):])] = 97.0
    for i in case.kinds["subs_8"][:3]:       # 8 substitutions print below 100: HDR with score_repaired 100
        case.sr_fixed[i] = 100.0
    assert max(map(len, case.reads)) == La + PAD
    return case


@functools.lru_cache(maxsize=None)
def short(La: int, n: int = 0) -> Case:
    n = n or batch_size(La)
    seed = 2000 + La
    rng = np.random.Generator(np.random.PCG64(seed))
    amp = synth.random_amplicon(La, seed)
    reads = []
    for i in range(n):
        ln = int(rng.integers(100, SHORT_MAX - 9))
        o = 0 if i % 8 == 0 else La - ln if i % 8 == 1 else int(rng.integers(0, La - ln + 1))
        b, _ = synth.reads_from(amp[o:o + ln], 1, seed * 4099 + i, synth.PARITY_MIX)
        reads.append(b.tobytes().decode())
    case = Case("short_%d" % La, amp, reads, {})
    slots = rng.permutation(n).tolist()
    turn = [0]

    def window():
        ln = int(rng.integers(260, SHORT_MAX - 11))
        turn[0] += 1
        o = 0 if turn[0] % 8 == 0 else La - ln if turn[0] % 8 == 1 else int(rng.integers(0, La - ln + 1))
        return o, ln

    put = _plant(case, slots, window, rng)
    ms = multiples(La)
    for k, m in enumerate(ms):
        for j, rel in enumerate(RELATIONS):
            if n < 256 and j != k % 3:
                continue
            o = min(m - int(rng.integers(100, 160)), La - 270)
            w = amp[o:o + 270]
            p, d = _fixed_deletion(amp, m, rel)
            put(_apply(w, [(p - o, "D", d)]), case.marks.setdefault(("del", m, rel), []))
            rel2 = RELATIONS[(j + 1) % 3] if n < 256 else rel
            p, s = _ins_place(m, rel2, 0)
            put(_apply(w, [(p - o, "I", _insert_text(amp, p, s, rng))]), case.marks.setdefault(("ins", m, rel2), []))
    for k in ("del_first", "del_last", "ins_first", "ins_last"):
        case.edges[k] = []
    junk = lambda k: "".join(rng.choice(list("ACGT"), k))   # noqa: E731
    put(amp[La // 2:La // 2 + 200], case.edges["del_first"], case.edges["del_last"])
    put(junk(12) + amp[:250], case.edges["ins_first"])
    put(amp[La - 250:] + junk(12), case.edges["ins_last"])
    put(amp[La // 3:La // 3 + SHORT_MAX])                     # the longest read: exactly 300
    for i in case.kinds["subs_8"][:3]:       # a short read prints far below 97: HDR and MIXED for certain
        case.sr_fixed[i] = 100.0
    for i in case.kinds["subs_8"][3:6]:
        case.sr_fixed[i] = 97.0
    assert max(map(len, case.reads)) == SHORT_MAX and min(map(len, case.reads)) >= 80
    return case


# ---- the oracles' view --------------------------------------------------------------------------

@dataclass
class Rows:
    R: List[str]
    M: List[str]
    S: List[str]
    score: np.ndarray
    dash_ins: np.ndarray
    um: np.ndarray
    sr: np.ndarray
    sd: np.ndarray
    aln: np.ndarray
    lens: np.ndarray


def rows_of(aln: np.ndarray, lens: np.ndarray, n_ident: np.ndarray, seed: int, sr_fixed=None) -> Rows:
    """The strings, the printed identity and the test's pre-flag inputs of n alignments.  A read
    whose insertion lies in the column of a '-' byte (the known divergence) is made
    UNMODIFIED, as test_device_ops_lane_path_vs_oracle does."""
    n = len(lens)
    R = [aln[i, 0, :lens[i]].tobytes().decode("latin-1") for i in range(n)]
    M = [aln[i, 1, :lens[i]].tobytes().decode("latin-1") for i in range(n)]
    S = [aln[i, 2, :lens[i]].tobytes().decode("latin-1") for i in range(n)]
    score = np.array([float("%.1f" % (100.0 * a / b)) if b else 0.0 for a, b in zip(n_ident, lens)])
    dash_ins = ((aln[:, 0, :] == ord("-")) & (aln[:, 2, :] == ord("-"))
                & (np.arange(aln.shape[2])[None, :] < np.asarray(lens)[:, None])).any(axis=1)
    rng = np.random.Generator(np.random.PCG64(seed))
    sr = rng.choice([100.0, 99.0, 97.0, 50.0, math.nan], size=n)
    for i, v in (sr_fixed or {}).items():
        sr[i] = v
    return Rows(R, M, S, score, dash_ins, (score == 100) | dash_ins, sr, score - sr, aln, np.asarray(lens))


@functools.lru_cache(maxsize=None)
def oracle_rows(case_fn, La: int, n: int = 0) -> Rows:
    case = case_fn(La, n)
    res, aln = oracle_py.align_batch(case.amp, *case.packed(), nthreads=8)
    return rows_of(aln, res["aln_len"], res["n_ident"], La + 5, case.sr_fixed)


def reference(case: Case, rows: Rows, pname: str):
    prm = make_params(case.amp, PARAMS[pname])
    hdr = prm.expected_hdr
    return prm, qo.process_rows(rows.R, rows.M, rows.S, rows.um, rows.sd if hdr else None, rows.sr if hdr else None, prm)


@functools.lru_cache(maxsize=None)
def oracle_reference(case_fn, La: int, pname: str, n: int = 0):
    return reference(case_fn(La, n), oracle_rows(case_fn, La, n), pname)


def _runs(s):
    return qo._runs(s, "-")


def conditions(case: Case, rows: Rows, refs: Dict[str, dict]) -> dict:
    """Assert what the issue asks of a batch, from the oracle's rows alone; returns the figures
    (per over-capacity kind, the planted reads that are not UNMODIFIED among them)."""
    n, amp = case.n, case.amp
    subs = [m.count(".") for m in rows.M]
    dels = [len(_runs(s)) for s in rows.S]
    inss = [len(_runs(r)) for r in rows.R]
    dash = ["-" in r for r in case.reads]
    holds = {"subs_over": lambda i: 9 <= subs[i], "subs_8": lambda i: subs[i] == 8,
             "dels_3": lambda i: dels[i] >= 3, "dels_2": lambda i: dels[i] == 2,
             "ins_3": lambda i: inss[i] >= 3, "ins_2": lambda i: inss[i] == 2, "dash": lambda i: dash[i]}
    for k in PLANTED:
        good = [i for i in case.kinds[k] if holds[k](i)]
        assert len(good) >= KIND_MIN, (case.name, k, len(good))
    for (what, m, rel), idx in case.marks.items():
        def hit(i):
            for st, en in _runs(rows.S[i] if what == "del" else rows.R[i]):
                if (rel == "end" and en == m) or (rel == "start" and st == m) or (rel == "over" and st < m < en):
                    return True
            return False
        assert idx and all(hit(i) for i in idx), (case.name, what, m, rel)
    for m in multiples(len(amp)):        # every multiple is crossed by a deletion and an insertion
        for what in ("del", "ins"):
            assert any((what, m, rel) in case.marks for rel in RELATIONS), (case.name, what, m)
    for i in case.edges["del_first"]:
        assert _runs(rows.S[i])[0][0] == 0 and rows.R[i][0] != "-"
    for i in case.edges["del_last"]:
        assert _runs(rows.S[i])[-1][1] == len(rows.S[i]) and rows.R[i][-1] != "-"
    for i in case.edges["ins_first"]:
        assert rows.R[i][0] == "-"
    for i in case.edges["ins_last"]:
        assert rows.R[i][-1] == "-"
    assert all(case.edges[k] for k in ("del_first", "del_last", "ins_first", "ins_last"))
    assert (~rows.um).sum() * 4 >= n, (case.name, int((~rows.um).sum()))
    assert rows.dash_ins.sum() * 50 <= n, (case.name, int(rows.dash_ins.sum()))
    for pname, ref in refs.items():
        cls = ref["cls"][~rows.um]
        want = {0, 1} | ({2, 3} if PARAMS[pname].get("hdr") else set())
        if case.name.startswith("short") and not PARAMS[pname].get("guide"):
            # a read shorter than the region has an end deletion inside a window that spans the
            # region, and never prints 100: without a guide's window no short read is UNMODIFIED
            want.discard(0)
            assert not (cls == 0).any()
        assert want <= set(cls.tolist()) | ({0} if rows.um.any() else set()), (case.name, pname)
    over = {k: [i for i in case.kinds[k] if holds[k](i) and not rows.um[i]] for k in OVER}
    return {"over": over, "not_um": int((~rows.um).sum()), "dash_ins": int(rows.dash_ins.sum())}


FULL = (400, 520, 580, 640, 730, 1000, 1393, 1394, 1532, 1533, 1633, 1634, 2709)
SHORT = (1000, 1572, 1573, 1755, 1756, 2083, 3000)
