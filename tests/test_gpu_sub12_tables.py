"""Classify's one- and two-substitution certificates from the amplicon's self-mismatch tables (DESIGN.md 4a;
nw_band_classify<true, true>) against the word passes they replace (CRISPR_NW_SUB12_TABLE=0): the resident
pass and the packed call, each with the switch on and off, must give the same records, run offsets, runs
and path counts bit for bit, with certified reads among them, and every read must equal the CPU oracle
(tests/every_read.py; computed once per case, on the resident pass with the tables -- the other three runs
are held to that one bit for bit).  The argument itself: tests/test_sub12_tables_model.py.

Cases: the smallest at which the table form can go wrong.  La = 33: every one- and two-substitution read of
self-mismatch-poor amplicons (a corrected pair decides the certificate there).  La = 17, 250, 255, 256:
every one-substitution read, and the two-substitution reads whose bases are close together, near either
end or next to a multiple of 16 (the replaced passes' word boundaries, the table's clamps).  Each batch also
holds reads with 0, 3 and 4 substitutions and one indel, so the other paths share wavefronts with them."""
import itertools

import numpy as np
import pytest

from crispresso_amd import synth
from crispresso_amd.aligner import pack_2bit, pack_reads
from tests.every_read import every_read

pytestmark = pytest.mark.gpu

FIELDS = ("aln_len", "n_ident", "n_sim", "n_gaps", "score", "end_i", "end_j", "flags")
BASES = "ACGT"


def others(b):
    return [c for c in BASES if c != b]


def sub(amp, places):
    s = list(amp)
    for p, b in places:
        s[p] = b
    return "".join(s)


def one_sub_reads(amp):
    return [sub(amp, [(f, b)]) for f in range(len(amp)) for b in others(amp[f])]


def mixed_in(amp, rng, n):
    """n each of: exact copies, reads with 3 and with 4 substitutions, one deletion, one insertion."""
    La = len(amp)
    out = [amp] * n
    for k in (3, 4):
        for _ in range(n):
            ps = rng.choice(La, k, replace=False)
            out.append(sub(amp, [(int(p), others(amp[p])[int(rng.integers(3))]) for p in ps]))
    for _ in range(n):
        p, k = int(rng.integers(1, La - 3)), int(rng.integers(1, 3))
        out.append(amp[:p] + amp[p + k:])
        out.append(amp[:p] + "".join(BASES[i] for i in rng.integers(0, 4, k)) + amp[p:])
    return out


def shuffled(reads, rng):
    return [reads[i] for i in rng.permutation(len(reads))]


def exhaustive_batch(amp, seed):
    """Every one- and every two-substitution read (99 + 4,752 at La = 33) and the mixed-in reads."""
    rng = np.random.Generator(np.random.PCG64(seed))
    La = len(amp)
    reads = one_sub_reads(amp)
    for f, l in itertools.combinations(range(La), 2):
        reads += [sub(amp, [(f, b), (l, c)]) for b in others(amp[f]) for c in others(amp[l])]
    assert len(reads) == 3 * La + 9 * La * (La - 1) // 2
    return shuffled(reads + mixed_in(amp, rng, 40), rng)


def edge_batch(amp, seed):
    """Every one-substitution read; every two-substitution read with l - f <= 4; one two-substitution read
    (bases drawn) for every other pair with f or l within 4 of either end or within 1 of a multiple of 16."""
    rng = np.random.Generator(np.random.PCG64(seed))
    La = len(amp)
    edge = lambda p: p < 4 or p >= La - 4 or p % 16 in (15, 0, 1)
    reads = one_sub_reads(amp)
    for f, l in itertools.combinations(range(La), 2):
        if l - f <= 4:
            reads += [sub(amp, [(f, b), (l, c)]) for b in others(amp[f]) for c in others(amp[l])]
        elif edge(f) or edge(l):
            reads.append(sub(amp, [(f, others(amp[f])[int(rng.integers(3))]), (l, others(amp[l])[int(rng.integers(3))])]))
    assert len(reads) <= 24000
    return shuffled(reads + mixed_in(amp, rng, 40), rng)


def poor_amplicons():
    """La = 33: a random amplicon, period 1 / 2 / 3 repeats, an 8-base homopolymer inside a random one."""
    rnd = synth.random_amplicon(33, 33)
    return {"random": rnd, "period1": "A" * 33, "period2": ("AC" * 17)[:33], "period3": "ACG" * 11,
            "homopolymer8": rnd[:11] + "T" * 8 + rnd[19:]}


def edge_amplicon(La):
    """A random amplicon; from 24 bases on with an 8-base homopolymer a third of the way in."""
    rnd = synth.random_amplicon(La, 7 + La)
    h = La // 3
    return rnd if La < 24 else rnd[:h] + "A" * 8 + rnd[h + 8:]


def run(a, amp, pr, n, mode):
    a.set_reference(amp)
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


def on_and_off(monkeypatch, a, amp, reads):
    buf, off = pack_reads(reads)
    pr = pack_2bit(buf, off)
    n = len(off) - 1
    monkeypatch.delenv("CRISPR_NW_SUB12_TABLE", raising=False)
    ob, ref, c_ref = run(a, amp, pr, n, "resident")
    chk = every_read(amp, buf, off, ob, threads=16)
    print(f"La {len(amp)}: {n} reads, {chk['distinct']} distinct, oracle mismatches {chk['mismatches']}, {c_ref}")
    assert chk["mismatches"] == 0, chk
    assert c_ref["exact_copies"] > 0, c_ref   # (the certificates are not vacuously off)
    counts = {("resident", "on"): c_ref}
    for mode, switch in (("call", "on"), ("resident", "0"), ("call", "0")):
        if switch == "on":
            monkeypatch.delenv("CRISPR_NW_SUB12_TABLE", raising=False)
        else:
            monkeypatch.setenv("CRISPR_NW_SUB12_TABLE", switch)
        _, got, counts[mode, switch] = run(a, amp, pr, n, mode)
        same(ref, got, f"{mode}, switch {switch}")
    monkeypatch.delenv("CRISPR_NW_SUB12_TABLE", raising=False)
    for mode in ("resident", "call"):
        assert counts[mode, "on"] == counts[mode, "0"], (mode, counts)
        assert counts[mode, "on"]["exact_copies"] > 0, (mode, counts)


@pytest.mark.parametrize("name", ["random", "period1", "period2", "period3", "homopolymer8"])
def test_exhaustive_33(monkeypatch, aligner, name):
    amp = poor_amplicons()[name]
    on_and_off(monkeypatch, aligner, amp, exhaustive_batch(amp, 33))


@pytest.mark.parametrize("La", [17, 250, 255, 256])
def test_edges(monkeypatch, aligner, La):
    amp = edge_amplicon(La)
    on_and_off(monkeypatch, aligner, amp, edge_batch(amp, La))
