"""The sgRNA counting semantics in plain Python: what crispresso_amd/count.py and the kernels of
crispresso_amd/csrc/nw_count.hip are held to.

Per read ``s`` (bytes, as given, case-sensitive) with a tracrRNA ``T`` of ``m`` bytes and a guide
length ``L``: ``idx`` is the first position of ``T`` in ``s``; a read without it is counted in
``n_reads`` only.  The guide is ``s[idx - L : idx]`` under Python's slice rule, which this file
spells out (:func:`guide_slice`) so that the rule, and not the interpreter, is what the tests
pin.  Without a whitelist every guide is a key, in order of first appearance; with one, only
its keys count and all of them stay, in file order.
"""
from typing import Dict, List, Optional, Sequence, Tuple


def find_first(s: bytes, t: bytes) -> int:
    """The smallest p in [0, len(s) - len(t)] with s[p:p+len(t)] == t, else -1."""
    n, m = len(s), len(t)
    for p in range(0, n - m + 1):
        if s[p:p + m] == t:
            return p
    return -1


def guide_slice(n: int, idx: int, L: int) -> Tuple[int, int]:
    """(start, length) of ``s[idx - L : idx]`` for a read of n bytes."""
    st = idx - L
    if st < 0:
        st = max(0, st + n)
    return (st, idx - st) if st < idx else (st, 0)


def whitelist_keys(lines: Sequence[bytes]) -> List[bytes]:
    """The distinct stripped lines in order of their first position (an empty line is b"")."""
    seen: Dict[bytes, int] = {}
    for line in lines:
        seen.setdefault(bytes(line).strip(), len(seen))
    return list(seen)


def count_model(reads: Sequence[bytes], tracr: bytes, L: int = 20, guides: Optional[Sequence[bytes]] = None):
    """-> dict(guides, counts, first, pos, group_of_read, n_reads, n_found, n_counted).

    ``guides`` is the whitelist (already stripped keys or raw lines); ``first`` is each group's
    smallest read index (-1 for whitelist keys)."""
    keys: Dict[bytes, int] = {}
    counts: List[int] = []
    first: List[int] = []
    fixed = guides is not None
    if fixed:
        for k in whitelist_keys(guides):
            keys[k] = len(counts)
            counts.append(0)
            first.append(-1)
    pos, gor = [], []
    n_found = n_counted = 0
    for r, s in enumerate(reads):
        s = bytes(s)
        idx = find_first(s, tracr)
        pos.append(idx)
        if idx < 0:
            gor.append(-1)
            continue
        n_found += 1
        st, ln = guide_slice(len(s), idx, L)
        g = s[st:st + ln]
        k = keys.get(g)
        if k is None:
            if fixed:
                gor.append(-1)
                continue
            k = keys[g] = len(counts)
            counts.append(0)
            first.append(r)
        counts[k] += 1
        n_counted += 1
        gor.append(k)
    return {"guides": list(keys), "counts": counts, "first": first, "pos": pos, "group_of_read": gor,
            "n_reads": len(reads), "n_found": n_found, "n_counted": n_counted}


def fast_model(reads: Sequence[bytes], tracr: bytes, L: int = 20, guides: Optional[Sequence[bytes]] = None):
    """The same result with the interpreter's own ``find`` and slice (the loop a user of the
    reference runs today; tests/test_count_model.py holds it equal to :func:`count_model`)."""
    keys: Dict[bytes, int] = {}
    counts: List[int] = []
    first: List[int] = []
    fixed = guides is not None
    if fixed:
        for k in whitelist_keys(guides):
            keys[k] = len(counts)
            counts.append(0)
            first.append(-1)
    pos, gor = [], []
    n_found = n_counted = 0
    for r, s in enumerate(reads):
        idx = s.find(tracr)
        pos.append(idx)
        if idx < 0:
            gor.append(-1)
            continue
        n_found += 1
        g = s[idx - L:idx]
        k = keys.get(g)
        if k is None:
            if fixed:
                gor.append(-1)
                continue
            k = keys[g] = len(counts)
            counts.append(0)
            first.append(r)
        counts[k] += 1
        n_counted += 1
        gor.append(k)
    return {"guides": list(keys), "counts": counts, "first": first, "pos": pos, "group_of_read": gor,
            "n_reads": len(reads), "n_found": n_found, "n_counted": n_counted}
