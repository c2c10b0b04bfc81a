"""CPU restatement of the table form of classify's one- and two-substitution certificates:
the shifted diagonals' facts of a read that equals the amplicon but at one or two bases, taken from the
amplicon's self-mismatch prefix counts (nw_host.cpp cls_image) and corrected at the substituted bases,
against the brute-force definition (the word passes of nw_band_classify<true, false>) -- for the six calls
the kernel makes, on every one- and two-substitution read of self-mismatch-poor and random amplicons.
tests/test_gpu_sub12_tables.py holds the kernel itself to the word passes and to the oracle."""
import itertools

import numpy as np
import pytest

from crispresso_amd import synth

BASES = "ACGT"


def tables(amp):
    """cls_image's words: word q (0 .. La) holds C_sh[q] = #{i < q: i < La - sh, amp[i] != amp[i + sh]}
    in byte sh - 1, sh = 1, 2, 3 (constant from q = La - sh on; word La: the totals)."""
    La = len(amp)
    words, c = [], [0, 0, 0]
    for q in range(La + 1):
        words.append(c[0] | c[1] << 8 | c[2] << 16)
        for sh in (1, 2, 3):
            if q + sh < La:
                c[sh - 1] += amp[q] != amp[q + sh]
    assert max(c) <= 255
    return words


def brute(amp, read, sgn, sh, qa, qb):
    """-> (tot, ge, le) of diagonal d = sgn * sh over its pairs q in [0, La - sh)."""
    La = len(amp)
    m = [(read[q + sh] != amp[q]) if sgn > 0 else (read[q] != amp[q + sh]) for q in range(max(0, La - sh))]
    return sum(m), any(v for q, v in enumerate(m) if q >= qa), any(v for q, v in enumerate(m) if q <= qb)


def table_form(amp, words, read, subs, sgn, sh, qa, qb):
    """The same from the prefix counts: subs = the substituted bases (one or two), of which the form
    reads only the read's base there."""
    La = len(amp)
    n = max(0, La - sh)
    C = lambda q: (words[min(max(q, 0), La)] >> (8 * (sh - 1))) & 0xFF   # (clamped to [0, La]: constant past n)
    tot = C(La)
    ge_n, le_n = tot - C(qa), C(qb + 1)
    for p in subs:
        q = p - sh if sgn > 0 else p
        if not 0 <= q < n:
            continue
        other = amp[q] if sgn > 0 else amp[q + sh]
        d = int(read[p] != other) - (C(q + 1) - C(q))
        tot += d
        if q >= qa:
            ge_n += d
        if q <= qb:
            le_n += d
    return tot, ge_n > 0, le_n > 0


def calls(La, f, l):
    """The kernel's six calls for a read with first / last substituted base f, l."""
    return [(1, 1, f, l - 2), (-1, 1, f + 1, l - 1), (1, 2, 0, La), (-1, 2, 0, La), (1, 3, 0, La), (-1, 3, 0, La)]


def sub_reads(amp):
    """Every one-substitution read (f, base) and every two-substitution read (f, l, base, base)."""
    La = len(amp)
    for f in range(La):
        for b in BASES:
            if b != amp[f]:
                yield amp[:f] + b + amp[f + 1:], (f,)
    for f, l in itertools.combinations(range(La), 2):
        for b, c in itertools.product(BASES, BASES):
            if b != amp[f] and c != amp[l]:
                yield amp[:f] + b + amp[f + 1:l] + c + amp[l + 1:], (f, l)


def amplicons(La):
    rep = lambda unit: (unit * La)[:La]
    out = [rep("A"), rep("AC"), rep("ACG"), rep("ACGT"), synth.random_amplicon(La, La), synth.random_amplicon(La, 100 + La)]
    if La > 16:   # a 16-base homopolymer followed by another base (a whole word without a self-mismatch)
        out.append(("G" * 16 + "C" + synth.random_amplicon(La, 7))[:La])
    return out


@pytest.mark.parametrize("La", [3, 5, 17, 33])
def test_table_form_equals_brute_force(La):
    n = 0
    for amp in amplicons(La):
        words = tables(amp)
        for read, subs in sub_reads(amp):
            f, l = subs[0], subs[-1]
            for sgn, sh, qa, qb in calls(La, f, l):
                assert table_form(amp, words, read, subs, sgn, sh, qa, qb) == brute(amp, read, sgn, sh, qa, qb), (
                    amp, read, sgn, sh, qa, qb)
                n += 1
    assert n == 6 * len(amplicons(La)) * (3 * La + 9 * La * (La - 1) // 2)


def test_tables_shape():
    """The prefix counts: a homopolymer has none, a period-2 repeat none at shift 2, and each count is the
    number of self-mismatching pairs before q (constant from q = La - sh on)."""
    assert tables("AAAAA") == [0] * 6
    w = tables("ACACAC")
    assert [x & 0xFF for x in w] == [0, 1, 2, 3, 4, 5, 5]
    assert [(x >> 8) & 0xFF for x in w] == [0] * 7
    assert [(x >> 16) & 0xFF for x in w] == [0, 1, 2, 3, 3, 3, 3]
    rng = np.random.Generator(np.random.PCG64(3))
    amp = "".join(BASES[i] for i in rng.integers(0, 4, 256))
    w = tables(amp)
    for sh in (1, 2, 3):
        want = np.concatenate([[0], np.cumsum([amp[q] != amp[q + sh] for q in range(256 - sh)])])
        got = [(x >> (8 * (sh - 1))) & 0xFF for x in w]
        assert got[: 257 - sh] == list(want) and set(got[256 - sh:]) == {int(want[-1])}
