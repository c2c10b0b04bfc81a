"""CPU restatement of cert_indel's one pass over the candidate's two diagonals (nw_band.hip,
cert_indel<true>): the longer sequence l against the shorter s at shift 0 and at shift kab, P = Ls positions,
on 2-bit words as the kernel holds them -- per word both mismatch masks (the odd bit of each base) under one
length mask (0xaaaaaaaa below the last word P >> 4, the partial mask there, 0 past it; both taken once before
the loop), the first nonzero word of shift 0 and the last of shift kab kept with their indices, ctz / clz once
after the loop, the count classes (0, 1, >= 2 mismatches) from popcounts.  Held to the plain definition: the
first mismatching index of shift 0 (P: none), the last of shift kab + 1 (0: none) and both counts capped at 2,
over the P positions.  Every kab 1 .. 10 and every P 1 .. 272 (17 words), on pure indels at the gap positions
where a mask changes word between the two diagonals, indels with a further substitution, unrelated pairs and
sequences without any mismatch.  tests/test_gpu_cert_onepass.py holds the kernel itself to the scans it
replaces and to the oracle."""
import numpy as np
import pytest

M32 = 0xFFFFFFFF
NW_L, NW_S = 18, 17   # words of l and of s the pass reads (l's word t + 1 at t = 16)


def pack2(codes, nwords):
    """2-bit words: base p in bits 2 (p % 16) of word p / 16, zero past the sequence."""
    w = [0] * nwords
    for p, c in enumerate(codes):
        w[p >> 4] |= int(c) << (2 * (p & 15))
    return w


def alignbit(hi, lo, s):
    return (((hi << 32) | lo) >> s) & M32


def ctz(x):
    return (x & -x).bit_length() - 1


def clz(x):
    return 32 - x.bit_length()


def one_pass(lw, sw, kab, P):
    """-> (f0, c0, gk, ck) as the kernel's pass computes them."""
    last = P >> 4
    pm = (0xAAAAAAAA >> (32 - 2 * (P & 15))) if P & 15 else 0
    w0 = wk = 0
    i0 = ik = n0 = nk = 0
    for t in range(17):
        vm = 0xAAAAAAAA if t < last else (pm if t == last else 0)
        zk = alignbit(lw[t + 1], lw[t], 2 * kab) ^ sw[t]
        z0 = lw[t] ^ sw[t]
        mk = (((zk << 1) & M32) | zk) & vm
        m0 = (((z0 << 1) & M32) | z0) & vm
        nk += bin(mk).count("1")
        n0 += bin(m0).count("1")
        if mk:
            wk, ik = mk, t
        if w0 == 0:
            i0, w0 = t, m0
    f0 = 16 * i0 + (ctz(w0) >> 1) if w0 else P
    gk = 16 * ik + ((31 - clz(wk)) >> 1) + 1 if wk else 0
    return f0, min(n0, 2), gk, min(nk, 2)


def plain(l, s, kab, P):
    d0 = [i for i in range(P) if l[i] != s[i]]
    dk = [i for i in range(P) if l[i + kab] != s[i]]
    return (d0[0] if d0 else P), min(len(d0), 2), (dk[-1] + 1 if dk else 0), min(len(dk), 2)


def gap_places(P, kab):
    """Gap positions q in [1, P - 1]: the edges, and q and q + kab on, before and after every multiple of 16."""
    qs = {1, P - 1}
    for m in range(16, P + kab + 1, 16):
        for d in (-1, 0, 1):
            qs.update((m + d, m + d - kab))
    return sorted(q for q in qs if 1 <= q <= P - 1)


def pairs(rng, kab, P):
    """(l, s) code arrays, l of P + kab bases, s of P."""
    s = rng.integers(0, 4, P)
    out = []
    for q in gap_places(P, kab)[:: max(1, P // 48)] or [0]:   # (thinned at the long lengths; edges kept below)
        l = np.concatenate([s[:q], rng.integers(0, 4, kab), s[q:]])
        out.append((l, s))
    for q in (1, P - 1):
        if 1 <= q <= P - 1:
            l = np.concatenate([s[:q], rng.integers(0, 4, kab), s[q:]])
            out.append((l, s))
            for p in {0, q - 1, q + kab, P + kab - 1, (P + kab) // 2}:   # a further substitution
                l2 = l.copy()
                l2[p] = (l2[p] + 1 + rng.integers(0, 3)) % 4
                out.append((l2, s))
    out.append((rng.integers(0, 4, P + kab), s))                      # unrelated
    out.append((np.concatenate([s, rng.integers(0, 4, kab)]), s))     # shift 0 without a mismatch
    out.append((np.concatenate([rng.integers(0, 4, kab), s]), s))     # shift kab without one
    out.append((np.zeros(P + kab, np.int64), np.zeros(P, np.int64)))  # a homopolymer: neither has one
    h = np.concatenate([s[: P // 2], np.full(kab, s[P // 2 - 1] if P > 1 else 0), s[P // 2:]])
    out.append((h, s))                                                # the gap beside an equal base: several places
    return out


@pytest.mark.parametrize("kab", range(1, 11))
def test_one_pass_equals_definition(kab):
    rng = np.random.Generator(np.random.PCG64(1000 + kab))
    checked = 0
    for P in range(1, 273):
        for l, s in pairs(rng, kab, P):
            got = one_pass(pack2(l, NW_L), pack2(s, NW_S), kab, P)
            assert got == plain(l.tolist(), s.tolist(), kab, P), (kab, P, l.tolist(), s.tolist())
            checked += 1
    assert checked > 272 * 10


def test_bases_past_the_shorter_sequence_are_masked():
    """l's bases past P + kab and a read's neighbour in the stream (nonzero words past s) never count."""
    rng = np.random.Generator(np.random.PCG64(7))
    for P in (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 271, 272):
        for kab in (1, 10):
            s = rng.integers(0, 4, P)
            l = np.concatenate([s[: P // 2], rng.integers(0, 4, kab), s[P // 2:]])
            lw = pack2(np.concatenate([l, rng.integers(1, 4, 288 - len(l))]), NW_L)   # junk to the last word
            sw = pack2(np.concatenate([s, rng.integers(1, 4, 272 - P)]), NW_S)
            assert one_pass(lw, sw, kab, P) == plain(l.tolist(), s.tolist(), kab, P), (P, kab)
