"""nw_band_cert's one-indel certificate with the candidate's two diagonals in one pass (DESIGN.md 4a;
cert_indel<true>) against the scans it replaces (CRISPR_NW_INDEL_ONEPASS=0), and classify's known-copy compare
(its gates, the certificates' precedence, the first-level-skip routing) against the path counts of the commit
before the pass.

The pass: packed input, ops output; the resident pass and the one-call path, each with the switch on and off,
must give the same records, run offsets, runs and path counts bit for bit -- counts too, as a certificate that
is quietly off still leaves correct outputs (the DP takes its reads) -- and every read must equal the CPU oracle
(tests/every_read.py over check_subset; once per case, on the resident pass with the switch on: the other three
runs are held to that one bit for bit).  Amplicons of 40, 100, 241, 250, 255 and 256 bp; 257 bp is left out:
classify's lane path, the only one that queues one-indel candidates, takes amplicons of at most 256 bp (nd <=
64).  Shorter and longer sequence lengths Ls of 16 k - 1, 16 k, 16 k + 1 among them (240 and 239 from 241, 241
and 240 from 250, 255, 256, 33 .. 31 from 40): the last word's partial mask.  The argument of the pass itself:
tests/test_indel_onepass_model.py.

Known copies: nw_set_known with a K of the amplicon's length, one-call path and resident call; every read against
the oracle, path_counts equal to that commit's library's, recorded below.  (Folding the compare into classify's
main-diagonal pass was measured with these cases and not kept; they stay as the compare's pin.)"""
import numpy as np
import pytest

from crispresso_amd import synth
from crispresso_amd.aligner import pack_2bit, pack_reads
from tests.every_read import every_read

pytestmark = pytest.mark.gpu

FIELDS = ("aln_len", "n_ident", "n_sim", "n_gaps", "score", "end_i", "end_j", "flags")
BASES = "ACGT"
SWITCH = "CRISPR_NW_INDEL_ONEPASS"
KMAX = 10


def other(b, rng):
    return [c for c in BASES if c != b][int(rng.integers(3))]


def sub(seq, p, rng):
    return seq[:p] + other(seq[p], rng) + seq[p + 1:]


def deletion(amp, q, k):
    return amp[:q] + amp[q + k:]


def insertion(amp, q, k, rng):
    return amp[:q] + "".join(BASES[i] for i in rng.integers(0, 4, k)) + amp[q:]


def gap_places(Ls, k):
    """Gap positions (index in the shorter sequence): the two edges; q and q + k on, one before and one after
    every multiple of 16 (a mask changes word between the two diagonals there)."""
    qs = {1, Ls - 1}
    for m in range(16, Ls + k + 1, 16):
        for d in (-1, 0, 1):
            qs.update((m + d, m + d - k))
    return sorted(q for q in qs if 1 <= q <= Ls - 1)


def one_indel_reads(amp, rng):
    """Pure deletions and pure insertions, every k 1 .. 10, at gap_places."""
    La, out = len(amp), []
    for k in range(1, KMAX + 1):
        if La - k >= 2:
            out += [deletion(amp, q, k) for q in gap_places(La - k, k)]
        out += [insertion(amp, q, k, rng) for q in gap_places(La, k)]
    return out


def must_fail_reads(amp, rng):
    """A one-indel read with one further substitution: before and after the gap, in the first and in the last
    word, at the last base."""
    La, out = len(amp), []
    for k in range(1, KMAX + 1):
        for q in {max(2, La // 3), max(2, min(La - k - 2, 2 * La // 3))}:
            for r in (deletion(amp, q, k), insertion(amp, q, k, rng)):
                L = len(r)
                gap_end = q + (k if L > La else 0)
                places = {int(rng.integers(0, q)), int(rng.integers(gap_end, L)), int(rng.integers(0, min(16, q))),
                          int(rng.integers(max(gap_end, 16 * ((L - 1) // 16)), L)), L - 1}
                out += [sub(r, p, rng) for p in places]
    return out


def repeat_amplicon(La):
    """A random amplicon with an 8-base homopolymer, a period-2 and a period-3 repeat (where it has the room)."""
    a = synth.random_amplicon(La, 300 + La)
    h = max(4, La // 5)
    a = a[:h] + "A" * 8 + a[h + 8:]
    if La >= 100:
        a = a[:h + 20] + "CACACACACA" + a[h + 30:]
        a = a[:h + 44] + "GTCGTCGTCGTC" + a[h + 56:]
    return a[:La], h


def ambiguous_reads(amp, h, rng):
    """Indels inside the homopolymer and the repeats: several gap positions are valid, the leftmost is chosen."""
    La, out = len(amp), []
    spans = [(h, 8, 1)] + ([(h + 20, 10, 2), (h + 44, 12, 3)] if La >= 100 else [])
    for s, n, per in spans:
        for q in range(s, s + n):
            for k in range(1, min(KMAX, n) + 1):
                out.append(deletion(amp, q, k))
                unit = (amp[s:s + per] * (k // per + 2))
                o = (q - s) % per
                out.append(amp[:q] + unit[o:o + k] + amp[q:])   # the repeat continued: an insertion with ties
    return out


def mixed_wavefronts(amp, rng):
    """Gaps of 1 and of 10 side by side, deletions and insertions interleaved, in this order (not shuffled);
    330 reads: full wavefronts and a partial last one."""
    La, out = len(amp), []
    for i in range(330):
        k = 1 if i % 2 == 0 else KMAX
        q = 1 + int(rng.integers(0, La - k - 1))
        out.append(deletion(amp, q, k) if (i // 2) % 2 == 0 else insertion(amp, q, k, rng))
    return out


def others_in(amp, rng, n):
    """Exact copies, reads with 1 .. 4 substitutions, longer gaps: the other paths share wavefronts."""
    La, out = len(amp), [amp] * n
    for k in (1, 2, 3, 4):
        for _ in range(n):
            r = amp
            for p in rng.choice(La, k, replace=False):
                r = sub(r, int(p), rng)
            out.append(r)
    for _ in range(n):
        q = int(rng.integers(1, max(2, La - 14)))
        out.append(deletion(amp, q, KMAX + 1 if La > 24 else 1))
        out.append(insertion(amp, q, KMAX + 2, rng))
    return out


def shuffled(reads, rng):
    return [reads[i] for i in rng.permutation(len(reads))]


def run(a, pr, n, mode):
    if mode == "call":
        ob = a.align_ops_packed(pr)
    else:
        a.upload_packed(pr)
        a.run_async()
        a.sync()
        ob = a.download_ops(n)
    return ob, (ob.stats.copy(), ob.ops_off.copy(), ob.ops[: int(ob.ops_off[n])].copy()), a.path_counts()


def same(x, y, what):
    for f in FIELDS:
        np.testing.assert_array_equal(x[0][f], y[0][f], err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(x[1], y[1], err_msg=f"{what}: run offsets")
    np.testing.assert_array_equal(x[2], y[2], err_msg=f"{what}: runs")


@pytest.fixture(scope="module")
def aligner(gpu_aligner_factory):
    return gpu_aligner_factory()   # one context for the module's cases


def on_and_off(monkeypatch, a, amp, reads, certified_at_least):
    """-> the path counts (switch on, resident pass).  certified_at_least: reads the batch holds that classify
    and nw_band_cert must finish without the DP (the certificates are not quietly off)."""
    buf, off = pack_reads(reads)
    pr = pack_2bit(buf, off)
    n = len(off) - 1
    a.set_reference(amp)
    monkeypatch.delenv(SWITCH, raising=False)
    ob, ref, c_ref = run(a, pr, n, "resident")
    chk = every_read(amp, buf, off, ob, threads=16)
    print(f"La {len(amp)}: {n} reads, {chk['distinct']} distinct, oracle mismatches {chk['mismatches']}, {c_ref}")
    assert chk["mismatches"] == 0, chk
    counts = {("resident", "on"): c_ref}
    for mode, switch in (("call", "on"), ("resident", "0"), ("call", "0")):
        if switch == "on":
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, switch)
        _, got, counts[mode, switch] = run(a, pr, n, mode)
        same(ref, got, f"{mode}, switch {switch}")
    monkeypatch.delenv(SWITCH, raising=False)
    for mode in ("resident", "call"):
        assert counts[mode, "on"] == counts[mode, "0"], (mode, counts)
        assert counts[mode, "on"]["exact_copies"] >= certified_at_least, (mode, counts, certified_at_least)
    return c_ref


def copies(amp, reads):
    """The batch's exact copies of the amplicon: the floor of exact_copies where no certificate is required."""
    return sum(r == amp for r in reads)


@pytest.mark.parametrize("La", [40, 100, 241, 250, 255, 256])
def test_one_indel_shapes(monkeypatch, aligner, La):
    rng = np.random.Generator(np.random.PCG64(5000 + La))
    amp = synth.random_amplicon(La, 200 + La)
    pure = one_indel_reads(amp, rng)
    reads = shuffled(pure + others_in(amp, rng, 24), rng)
    c = on_and_off(monkeypatch, aligner, amp, reads, copies(amp, reads))
    # a random amplicon: a pure indel misses the certificate only where another alignment scores as much by a
    # chance repeat beside the gap -- far fewer than half of them
    assert c["exact_copies"] >= copies(amp, reads) + len(pure) // 2, (c, len(pure))


@pytest.mark.parametrize("La", [40, 250])
def test_ambiguous_gaps(monkeypatch, aligner, La):
    rng = np.random.Generator(np.random.PCG64(6000 + La))
    amp, h = repeat_amplicon(La)
    reads = shuffled(ambiguous_reads(amp, h, rng) + others_in(amp, rng, 16), rng)
    on_and_off(monkeypatch, aligner, amp, reads, copies(amp, reads))


@pytest.mark.parametrize("La", [40, 100, 250, 256])
def test_must_fail_candidates(monkeypatch, aligner, La):
    rng = np.random.Generator(np.random.PCG64(7000 + La))
    amp = synth.random_amplicon(La, 200 + La)
    reads = shuffled(must_fail_reads(amp, rng) + others_in(amp, rng, 16), rng)
    on_and_off(monkeypatch, aligner, amp, reads, copies(amp, reads))


@pytest.mark.parametrize("La", [100, 250])
def test_mixed_gap_lengths_in_one_wavefront(monkeypatch, aligner, La):
    rng = np.random.Generator(np.random.PCG64(8000 + La))
    amp = synth.random_amplicon(La, 200 + La)
    reads = mixed_wavefronts(amp, rng)
    assert len(reads) % 64 != 0
    c = on_and_off(monkeypatch, aligner, amp, reads, 0)
    assert c["exact_copies"] >= len(reads) // 2, c


# ---- known copies ---------------------------------------------------------------------------------
# path_counts of the library of the commit before this file (00911dd, "Hold exception-byte reads to the oracle;
# close the dual call's byte race") on these batches, one-call path and resident call alike
PARENT_COUNTS = {
    (100, "block"): {'exact_copies': 191, 'band16': 167, 'band32': 0, 'band_fallback': 167, 'wide128': 167,
                     'exact_kernel': 0, 'wide_first': 59},
    (250, "block"): {'exact_copies': 190, 'band16': 168, 'band32': 0, 'band_fallback': 168, 'wide128': 168,
                     'exact_kernel': 0, 'wide_first': 60},
    (256, "block"): {'exact_copies': 190, 'band16': 168, 'band32': 0, 'band_fallback': 168, 'wide128': 168,
                     'exact_kernel': 0, 'wide_first': 60},
    (250, "two_sub"): {'exact_copies': 210, 'band16': 148, 'band32': 0, 'band_fallback': 148, 'wide128': 148,
                     'exact_kernel': 0, 'wide_first': 58},
}


def known_batch(amp, K, rng):
    La = len(amp)
    reads = [K] * 40 + [amp] * 40
    reads += [sub(K, p, rng) for p in (0, La - 1, 15, 16, 17, La // 2) for _ in range(3)]   # K but for one base
    for k in (1, 2):                                     # the certificates' precedence over a known copy
        for _ in range(40):
            r = amp
            for p in rng.choice(La, k, replace=False):
                r = sub(r, int(p), rng)
            reads.append(r)
    for k in (2, 3, 5):                                  # closer to K than to the amplicon: the first-level skip
        for _ in range(30):
            r = K
            for p in rng.choice(La, k, replace=False):
                r = sub(r, int(p), rng)
            reads.append(r)
    for _ in range(30):                                  # and DP reads of other lengths
        q = int(rng.integers(1, La - 12))
        reads += [deletion(K, q, 3), insertion(amp, q, 2, rng), deletion(amp, q, 12)]
    return shuffled(reads, rng)


@pytest.mark.parametrize("La,kind", sorted(PARENT_COUNTS))
def test_known_copies_paths(aligner, La, kind):
    rng = np.random.Generator(np.random.PCG64(9000 + La))
    amp = synth.random_amplicon(La, 200 + La)
    if kind == "block":
        K = synth.hdr_amplicon(amp, 4, start=La // 2 - 5, length=10)
    else:   # two substitutions apart: a copy of K is a two-substitution read, the certificate takes it first
        K = sub(sub(amp, La // 4, rng), 3 * La // 4, rng)
    reads = known_batch(amp, K, rng)
    buf, off = pack_reads(reads)
    pr = pack_2bit(buf, off)
    n = len(off) - 1
    a = aligner
    a.set_reference(amp)
    a.set_known(K)
    try:
        ob = a.align_ops_packed(pr)
        ref = (ob.stats.copy(), ob.ops_off.copy(), ob.ops[: int(ob.ops_off[n])].copy())
        c_call = a.path_counts()
        chk = every_read(amp, buf, off, ob, threads=16)
        ob2 = a.align_ops(None, off, resident=True)
        c_res = a.path_counts()
        same(ref, (ob2.stats, ob2.ops_off, ob2.ops[: int(ob2.ops_off[n])]), "resident call")
    finally:
        a.set_known(None)
    print(f"La {La} {kind}: {n} reads, oracle mismatches {chk['mismatches']}, call {c_call}, resident {c_res}")
    assert chk["mismatches"] == 0, chk
    assert c_call == PARENT_COUNTS[La, kind], c_call
    assert c_res == PARENT_COUNTS[La, kind], c_res
