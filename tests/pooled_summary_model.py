"""Plain-Python restatements of include/crispr_summary.h for the tests of the pooled summary
(tests/test_pooled_summary_model.py, tests/test_gpu_summary.py): the flags of one nw_stat record,
the 16 slots over per-read results, and small aligned rows to quantify."""
import numpy as np

from crispresso_amd import _lib
from crispresso_amd.aligner import printed_percent

SLOTS = _lib.NWS_SLOT_NAMES
RUN_SUMMARY_KEYS = SLOTS[1:15]          # the slots quantify.run_summary also returns, under the same names


def brute_thresholds(min_identity_score, L):
    """(keep_min[L], unmod_min[L]) by trying every n_ident."""
    keep = next((i for i in range(L + 1) if printed_percent(i, L) > min_identity_score), L + 1)
    unmod = next((i for i in range(L + 1) if printed_percent(i, L) == 100.0), L + 1)
    return keep, unmod


def flags(aln_len, n_ident, stat_flags, keep_min, unmod_min):
    """(pre, keep, n_out_of_range) of nws_flags, record by record."""
    max_cols = len(keep_min) - 1
    pre, keep, bad = [], [], 0
    for L, i, f in zip(aln_len, n_ident, stat_flags):
        L, i, f = int(L), int(i), int(f)
        if not 0 <= L <= max_cols:
            bad += 1
            pre.append(0)
            keep.append(0)
            continue
        keep.append(int(not (f & _lib.NW_FLAG_EMPTY) and i >= keep_min[L]))
        pre.append(_lib.NWQ_PRE_UNMODIFIED if i >= unmod_min[L] else 0)
    return np.array(pre, np.uint8), np.array(keep, np.uint8), bad


def slots(cls, n_mutated, n_inserted, n_deleted, pre, keep):
    """The 16 slots of nws_summary, read by read."""
    out = [0] * 16
    out[0] = len(cls)
    for c, mut, ins, dele, p, k in zip(cls, n_mutated, n_inserted, n_deleted, pre, keep):
        c = int(c)
        if not k:
            continue
        out[1] += 1
        out[2] += bool(int(p) & _lib.NWQ_PRE_UNMODIFIED) or c == 0
        out[3] += c == 1
        out[4] += c == 2
        out[5] += c == 3
        if c in (1, 2, 3):
            base = 6 + 3 * (c - 1)
            out[base] += ins > 0
            out[base + 1] += dele > 0
            out[base + 2] += mut > 0
        out[15] += c < 0
    return [int(x) for x in out]


def slots_of_summary(summary, n):
    """quantify.run_summary's dict as the 16 slots (slot 15 is 0: run_summary has no such rows)."""
    return [n] + [int(summary[key]) for key in RUN_SUMMARY_KEYS] + [0]


def aligned_rows(amp, sub=(), dele=None, ins=None):
    """(aligned amplicon, markup, aligned read): `amp` with the bases at `sub` replaced, the
    bases dele = (start, length) deleted and ins = (position, bases) inserted before position."""
    ref, mk, read = [], [], []
    for p, a in enumerate(amp):
        if ins is not None and p == ins[0]:
            for b in ins[1]:
                ref.append("-")
                mk.append(" ")
                read.append(b)
        if dele is not None and dele[0] <= p < dele[0] + dele[1]:
            ref.append(a)
            mk.append(" ")
            read.append("-")
        elif p in sub:
            ref.append(a)
            mk.append(".")
            read.append("ACGT"["ACGT".index(a) ^ 1])
        else:
            ref.append(a)
            mk.append("|")
            read.append(a)
    return "".join(ref), "".join(mk), "".join(read)
