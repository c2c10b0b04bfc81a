"""The demultiplexing rule of include/crispr_demux.h in plain Python: a dict of windows and a
``Counter`` of votes.  It is the thing to read beside the header; tests/test_demux_model.py holds
it to hand-worked cases and to the needle oracle, tests/test_gpu_demux.py holds the kernels to it.

Reads and amplicons are ``bytes``.
"""
from collections import Counter

NO_HIT, TIE = -1, -2
AMBIGUOUS = -1
COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def window_key(w):
    """The window in upper case (case is ignored), None when it holds a break: a byte that is
    none of A C G T a c g t."""
    key = bytes(w).upper()
    return key if not key.translate(None, b"ACGT") else None


def revcomp_key(key):
    return key.translate(COMPLEMENT)[::-1]


def revcomp(read):
    """The read reversed and complemented: A<->T C<->G a<->t c<->g, every other byte unchanged."""
    return bytes(read).translate(COMPLEMENT)[::-1]


def build_index(amplicons, k):
    """window key -> amplicon index, AMBIGUOUS for a window of two or more distinct amplicons."""
    index = {}
    for g, amp in enumerate(amplicons):
        for p in range(len(amp) - k + 1):
            key = window_key(amp[p:p + k])
            if key is None:
                continue
            if key not in index:
                index[key] = g
            elif index[key] != g:
                index[key] = AMBIGUOUS
    return index


def votes_of(index, read, k, both_strands=True):
    """Counter of (g, strand) over the read's windows."""
    tally = Counter()
    for p in range(len(read) - k + 1):
        key = window_key(read[p:p + k])
        if key is None:
            continue
        g = index.get(key, AMBIGUOUS)
        if g != AMBIGUOUS:
            tally[(g, 0)] += 1
        if both_strands:
            g = index.get(revcomp_key(key), AMBIGUOUS)
            if g != AMBIGUOUS:
                tally[(g, 1)] += 1
    return tally


def decide(tally, min_hits):
    """(which, strand, votes, rival) of one read's tally."""
    ranked = sorted(tally.values(), reverse=True)
    best = ranked[0] if ranked else 0
    rival = ranked[1] if len(ranked) > 1 else 0
    if best < min_hits:
        return NO_HIT, 0, best, rival
    if best == rival:
        return TIE, 0, best, rival
    (g, s), = [pair for pair, n in tally.items() if n == best]
    return g, s, best, rival


def demultiplex(amplicons, reads, k=16, min_hits=2, both_strands=True):
    """The whole result as a dict of lists: per read ``which``, ``strand``, ``votes``, ``rival``;
    per amplicon ``counts``; ``group_offsets``, ``order`` (the input index of each gathered read),
    ``groups`` (per amplicon the oriented reads) and ``n_windows`` / ``n_ambiguous``."""
    index = build_index(amplicons, k)
    out = {"which": [], "strand": [], "votes": [], "rival": []}
    for read in reads:
        g, s, best, rival = decide(votes_of(index, read, k, both_strands), min_hits)
        out["which"].append(g)
        out["strand"].append(s)
        out["votes"].append(best)
        out["rival"].append(rival)
    groups = [[] for _ in amplicons]
    members = [[] for _ in amplicons]
    for r, (g, s) in enumerate(zip(out["which"], out["strand"])):
        if g >= 0:
            members[g].append(r)
            groups[g].append(revcomp(reads[r]) if s else bytes(reads[r]))
    out["counts"] = [len(m) for m in members]
    out["group_offsets"] = [0]
    for m in members:
        out["group_offsets"].append(out["group_offsets"][-1] + len(m))
    out["order"] = [r for m in members for r in m]
    out["groups"] = groups
    out["n_windows"] = len(index)
    out["n_ambiguous"] = sum(1 for g in index.values() if g == AMBIGUOUS)
    return out
