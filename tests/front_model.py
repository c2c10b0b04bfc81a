"""The front end (crispresso_amd/frontend.py, nwp_prepare) restated on the CPU, and the generator
of its test inputs.

Per pair: ``fastq.quality_pass`` (CORE:296-305), the Trimmomatic restatements
(tests/trim_steps_model.py over oracle/trimmomatic_oracle.py), the FLASH restatement
(oracle/flash_oracle.py), then ``aligner.pack_2bit`` (host C++, no GPU) on the merged text."""
import functools
import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from crispresso_amd import fastq
from crispresso_amd.aligner import PackedReads, pack_2bit
from oracle import flash_oracle
from tests import trim_steps_model as tsm

HERE = os.path.dirname(os.path.abspath(__file__))
NEXTERA = os.path.join(HERE, "golden", "NexteraPE-PE.fa")
FILTERED, TRIMMED, NOT_COMBINED, COMBINED, COMBINED_OUTIE = range(5)
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")

Pair = Tuple[bytes, bytes, bytes, bytes]   # seq1, qual1, seq2, qual2 (single-end: the last two empty)


def rc(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def pack_lists(items: List[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(items) + 1, np.int64)
    np.cumsum([len(x) for x in items], out=off[1:])
    return np.frombuffer(b"".join(items), np.uint8).copy(), off


def packed_inputs(pairs: List[Pair], single_end: bool = False):
    """The six arguments of prepare_packed."""
    s1, off1 = pack_lists([p[0] for p in pairs])
    q1, _ = pack_lists([p[1] for p in pairs])
    if single_end:
        return s1, q1, off1, None, None, None
    s2, off2 = pack_lists([p[2] for p in pairs])
    q2, _ = pack_lists([p[3] for p in pairs])
    return s1, q1, off1, s2, q2, off2


@dataclass
class Expected:
    status: np.ndarray
    src: np.ndarray
    reads: List[bytes]
    quals: List[bytes]
    buf: np.ndarray
    qbuf: np.ndarray
    offsets: np.ndarray
    lens: np.ndarray
    packed: PackedReads
    trim: dict


def expected(pairs: List[Pair], *, min_bp_quality=0, min_single_bp_quality=0, trim=None, single_end=False,
             min_overlap=4, max_overlap=100, allow_outies=True) -> Expected:
    n = len(pairs)
    live = [True] * n
    if min_bp_quality > 0 or min_single_bp_quality > 0:
        a = fastq.quality_pass([p[1] for p in pairs], min_bp_quality, min_single_bp_quality)
        b = a if single_end else fastq.quality_pass([p[3] for p in pairs], min_bp_quality, min_single_bp_quality)
        live = [x and y for x, y in zip(a, b)]
    if trim:
        rec1, rec2 = tsm.run_pairs(trim, pairs, single_end=single_end)
    else:
        rec1 = [(0, len(p[0])) for p in pairs]
        rec2 = [None if single_end else (0, len(p[2])) for p in pairs]
    merger = flash_oracle.Merger(min_overlap=min_overlap, max_overlap=max_overlap, allow_outies=allow_outies)
    status = np.zeros(n, np.uint8)
    src, reads, quals = [], [], []
    tr = {"both": 0, "fwd_only": 0, "rev_only": 0, "dropped": 0}
    for i, (s1, q1, s2, q2) in enumerate(pairs):
        if not live[i]:
            status[i] = FILTERED
            continue
        a, b = rec1[i], rec2[i]
        ok_b = single_end or b is not None
        tr["both" if a is not None and ok_b else "fwd_only" if a is not None else
           "rev_only" if (b is not None and not single_end) else "dropped"] += 1
        if a is None or not ok_b:
            status[i] = TRIMMED
            continue
        w1, wq1 = s1[a[0]:a[0] + a[1]], q1[a[0]:a[0] + a[1]]
        if single_end:
            status[i] = COMBINED
            src.append(i), reads.append(w1), quals.append(wq1)
            continue
        got = merger.merge_pair(w1, wq1, s2[b[0]:b[0] + b[1]], q2[b[0]:b[0] + b[1]])
        if got is None:
            status[i] = NOT_COMBINED
            continue
        status[i] = COMBINED_OUTIE if got[2] else COMBINED
        src.append(i), reads.append(got[0]), quals.append(got[1])
    buf, offsets = pack_lists(reads)
    qbuf, _ = pack_lists(quals)
    lens = np.diff(offsets).astype(np.uint16)
    if len(reads):
        pk = pack_2bit(buf, offsets, nthreads=1)
    else:
        pk = PackedReads(np.zeros(1, np.uint8), offsets, np.zeros(0, np.int64), np.zeros(0, np.uint8), lens)
    return Expected(status, np.array(src, np.int64), reads, quals, buf, qbuf, offsets, lens, pk, tr)


# ---- the packer test's input ----------------------------------------------------------------

PACKER_SEED = 20240611
PACKER_PAIRS = 3500
PACKER_TRIM = ["ILLUMINACLIP:" + NEXTERA + ":0:90:10:0:true", "SLIDINGWINDOW:4:15", "MINLEN:40"]
PACKER_FILTER = dict(min_bp_quality=20, min_single_bp_quality=3)
_PREFIX = b"AGATGTGTATAAGAGACAG"   # PrefixNX/1 and /2 of NexteraPE-PE.fa


def _bases(rng, n: int) -> bytes:
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def packer_pairs(seed: int = PACKER_SEED, n: int = PACKER_PAIRS) -> List[Pair]:
    """Pairs of 40-150 bases cut from 120-260 bp fragments; families: plain (most), unrelated
    mates, fragments shorter than the reads followed by the Nextera adapters (read-through),
    qualities low throughout (the filter), one base below the single-base threshold (the filter),
    a low-quality head (SLIDINGWINDOW drops the read), a low-quality tail (SLIDINGWINDOW cuts
    it); about 3 % N in a tenth of the reads."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for _ in range(n):
        fam = rng.choice(7, p=[0.66, 0.06, 0.08, 0.04, 0.02, 0.05, 0.09])
        frag = _bases(rng, int(rng.integers(120, 261)))
        # the mates overlap by at least 10 bases (a tenth of the pairs: any lengths)
        l1 = int(rng.integers(max(40, len(frag) - 140), 151))
        l2 = int(rng.integers(max(40, len(frag) + 10 - l1), 151))
        if rng.random() < 0.1:
            l1, l2 = (int(x) for x in rng.integers(40, 151, size=2))
        if fam == 2:   # read-through: the fragment ends inside both reads
            frag = frag[:int(rng.integers(45, 118))]
            l1 = l2 = int(rng.integers(120, 151))
            s1 = (frag + rc(_PREFIX) + _bases(rng, 150))[:l1]
            s2 = (rc(frag) + rc(_PREFIX) + _bases(rng, 150))[:l2]
        else:
            s1, s2 = frag[:l1], rc(frag)[:l2]
            if fam == 1:
                s2 = _bases(rng, l2)
        q = [rng.integers(25, 41, size=len(s)) for s in (s1, s2)]
        if fam == 3:
            q = [rng.integers(4, 16, size=len(s)) for s in (s1, s2)]
        elif fam == 4:
            k = int(rng.integers(0, 2))
            q[k][int(rng.integers(0, len(q[k])))] = 2
        elif fam == 5:
            k = int(rng.integers(0, 2))
            q[k][:int(rng.integers(8, 20))] = rng.integers(3, 8)
        elif fam == 6:
            for k in range(2):
                t = int(rng.integers(5, 40))
                q[k][len(q[k]) - t:] = rng.integers(3, 12, size=t)
        seqs = []
        for s in (s1, s2):
            if rng.random() < 0.1:
                a = np.frombuffer(s, np.uint8).copy()
                a[rng.random(len(a)) < 0.03] = ord("N")
                s = a.tobytes()
            seqs.append(s)
        out.append((seqs[0], (q[0] + 33).astype(np.uint8).tobytes(), seqs[1], (q[1] + 33).astype(np.uint8).tobytes()))
    return out


@functools.lru_cache(maxsize=None)
def packer_case():
    pairs = packer_pairs()
    return pairs, expected(pairs, trim=PACKER_TRIM, **PACKER_FILTER)


def floors(e: Expected) -> dict:
    """The counts the packer test's input must reach."""
    off = e.offsets
    return {
        "combined": int(np.sum(e.status >= COMBINED)), "not_combined": int(np.sum(e.status == NOT_COMBINED)),
        "trimmed": int(np.sum(e.status == TRIMMED)), "filtered": int(np.sum(e.status == FILTERED)),
        "outies": int(np.sum(e.status == COMBINED_OUTIE)),
        "exceptions": len(e.packed.exc_pos), "len_mod4": sorted(set((np.diff(off) % 4).tolist())),
        "starts_mid_dword": int(np.sum(off[:-1] % 16 != 0)), "ends_mid_dword": int(np.sum(off[1:] % 16 != 0)),
    }


# ---- the alignment test's input -------------------------------------------------------------

ALIGN_SEED = 77


def align_case(n: int = 3000, seed: int = ALIGN_SEED):
    """(amplicon, pairs): mates of 120 bases from the two ends of edited copies of a 200 bp
    amplicon (synth.reads_from's C2 mix: substitutions, 1-30 bp deletions, insertions), a few
    pairs of unrelated reads."""
    from crispresso_amd import synth

    amp = synth.random_amplicon(200, seed)
    buf, off = synth.reads_from(amp, n, seed + 1)
    rng = np.random.Generator(np.random.PCG64(seed + 2))
    pairs = []
    for i in range(n):
        frag = buf[off[i]:off[i + 1]].tobytes()
        if rng.random() < 0.01:
            frag = _bases(rng, 200)
        s1, s2 = frag[:120], rc(frag)[:120]
        pairs.append((s1, b"I" * len(s1), s2, b"I" * len(s2)))
    return amp, pairs
