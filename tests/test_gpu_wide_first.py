"""Wide first: DP reads the 16-diagonal band cannot certify -- another length than
the amplicon's, or its length with too many substitutions -- are listed apart by the sort and
aligned on the wide level beside the first level.  Every case checks every read against the CPU
oracle (tests/every_read.py) and the same call with CRISPR_NW_WIDE_FIRST=0 bit for bit."""
import numpy as np
import pytest

from crispresso_amd import synth
from crispresso_amd.aligner import pack_2bit, pack_reads
from tests.every_read import every_read, every_read_multi

pytestmark = pytest.mark.gpu

FIELDS = ("aln_len", "n_ident", "n_sim", "n_gaps", "score", "end_i", "end_j", "flags")
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def amplicon(La, seed):
    """A random amplicon with an 8-base homopolymer a third of the way in."""
    rnd = synth.random_amplicon(La, seed)
    h = La // 3
    return rnd[:h] + "A" * 8 + rnd[h + 8:]


def subs(amp, k, rng):
    s = list(amp)
    for p in rng.choice(len(amp), k, replace=False):
        s[p] = OTHER[s[p]]
    return "".join(s)


def deletion(amp, pos, k):
    return amp[:pos] + amp[pos + k:]


def insertion(amp, pos, k, rng):
    return amp[:pos] + "".join("ACGT"[i] for i in rng.integers(0, 4, k)) + amp[pos:]


def mix_reads(La, seed):
    """~1.5k reads: 0 .. 12 substitutions, deletions of 1 .. 30 and insertions of 1 .. 10 at three
    positions (one in the homopolymer), each also with two substitutions; N and IUPAC reads; two chimeras."""
    rng = np.random.Generator(np.random.PCG64(seed))
    amp = amplicon(La, seed)
    reads = []
    for k in range(13):
        reads += [subs(amp, k, rng) for _ in range(60)]
    for pos in (La // 3 + 2, La // 2, La - 35):
        for k in range(1, 31):
            reads += [deletion(amp, pos, k), subs(deletion(amp, pos, k), 2, rng)]
        for k in range(1, 11):
            reads += [insertion(amp, pos, k, rng), subs(insertion(amp, pos, k, rng), 2, rng)]
    for q in range(12):
        s = list(subs(amp, q, rng))
        s[5 + 3 * q] = "N"
        s[La - 10 - q] = "NRYKMSW"[q % 7]
        reads.append("".join(s))
    reads += ["N" * La, amp[: La // 2] + "N" * 3 + amp[La // 2 + 3:]]
    other = synth.random_amplicon(La, seed + 100)
    reads += [amp[: La // 2] + other[La // 2:], other[: La // 3] + amp[La // 3:]]   # chimeras
    order = rng.permutation(len(reads))
    return amp, [reads[i] for i in order]


def run(a, amp, reads, mode):
    """-> (stats, ops_off, ops, path counts) of the packed call or the resident pass."""
    buf, off = pack_reads(reads)
    pr = pack_2bit(buf, off)
    n = len(off) - 1
    a.set_reference(amp)
    if mode == "call":
        ob = a.align_ops_packed(pr)
    else:
        a.upload_packed(pr)
        a.run_async()
        a.sync()
        ob = a.download_ops(n)
    counts = a.path_counts()
    return buf, off, ob, (ob.stats.copy(), ob.ops_off.copy(), ob.ops[: int(ob.ops_off[n])].copy()), counts


def same(x, y, what):
    for f in FIELDS:
        np.testing.assert_array_equal(x[0][f], y[0][f], err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(x[1], y[1], err_msg=what)
    np.testing.assert_array_equal(x[2], y[2], err_msg=what)


@pytest.fixture(scope="module")
def aligner(gpu_aligner_factory):
    return gpu_aligner_factory()   # one context for the module's cases


def on_and_off(monkeypatch, a, amp, reads, mode, cap=None):
    """The batch with the wide-first list and without: every read against the oracle, the two runs
    bit for bit.  -> the path counts of both."""
    if cap is not None:
        monkeypatch.setenv("CRISPR_NW_WIDE_FIRST_CAP", str(cap))
    monkeypatch.delenv("CRISPR_NW_WIDE_FIRST", raising=False)
    buf, off, ob, on, c_on = run(a, amp, reads, mode)
    chk = every_read(amp, buf, off, ob, threads=16)
    assert chk["mismatches"] == 0, chk
    monkeypatch.setenv("CRISPR_NW_WIDE_FIRST", "0")
    _, _, _, off_, c_off = run(a, amp, reads, mode)
    monkeypatch.delenv("CRISPR_NW_WIDE_FIRST")
    same(on, off_, mode)
    assert c_off["wide_first"] == 0
    for k in ("exact_copies", "band16"):   # the keys' meaning does not depend on the switch
        assert c_on[k] == c_off[k], (k, c_on, c_off)
    assert c_on["wide128"] + c_on["exact_kernel"] == c_on["band_fallback"] >= c_on["wide_first"]
    return c_on, c_off


@pytest.mark.parametrize("mode", ["call", "resident"])
@pytest.mark.parametrize("La", [250, 96])
def test_mix(monkeypatch, aligner, La, mode):
    amp, reads = mix_reads(La, 31 + La)
    c_on, _ = on_and_off(monkeypatch, aligner, amp, reads, mode)
    assert c_on["wide_first"] > 0, c_on


def main_and_shifted(amp, read):
    """Main-diagonal score D0 of an equal-length A C G T read (match 5, mismatch -4) and the
    largest single-diagonal sum over |d| = 8 .. 12."""
    x = np.frombuffer(amp.encode(), np.uint8)
    y = np.frombuffer(read.encode(), np.uint8)
    score = lambda eq: int(np.where(eq, 5, -4).sum())
    best = -(1 << 30)
    for d in range(8, 13):
        best = max(best, score(x[:-d] == y[d:]), score(x[d:] == y[:-d]))
    return score(x == y), best


@pytest.mark.parametrize("mode", ["call", "resident"])
def test_empty_second_sweep(monkeypatch, aligner, mode):
    """Substitutions and single indels on a random amplicon: every read the first level keeps (at most
    5 substitutions) has its diagonals just past the band far below its main diagonal, so the first
    level certifies it, and the wide-first launch holds everything else: the later wide launch and
    the exact kernel take nothing."""
    rng = np.random.Generator(np.random.PCG64(77))
    amp = synth.random_amplicon(250, 77)
    reads = []
    for k in range(13):
        reads += [subs(amp, k, rng) for _ in range(80)]
    for pos in (60, 125, 200):
        for k in range(1, 11):
            reads += [deletion(amp, pos, k), insertion(amp, pos, k, rng)]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    for r in reads:   # the precondition
        if len(r) == len(amp) and sum(p != q for p, q in zip(r, amp)) <= 5:
            d0, shifted = main_and_shifted(amp, r)
            assert shifted < d0, (r, d0, shifted)
    c_on, c_off = on_and_off(monkeypatch, aligner, amp, reads, mode)
    assert c_on["wide_first"] > 0
    assert c_on["band_fallback"] - c_on["wide_first"] == 0 and c_on["exact_kernel"] == 0, c_on


@pytest.mark.parametrize("marked", [63, 64, 65, 500])
def test_cap(monkeypatch, aligner, marked):
    """CRISPR_NW_WIDE_FIRST_CAP=64: a list of at most 64 reads runs beside the first level, a longer
    one joins the first level's list."""
    rng = np.random.Generator(np.random.PCG64(marked))
    amp = synth.random_amplicon(250, 5)
    reads = [subs(amp, 8, rng) for _ in range(marked)] + [subs(amp, 4, rng) for _ in range(100)] + [amp] * 200
    reads = [reads[i] for i in rng.permutation(len(reads))]
    for mode in ("call", "resident"):
        c_on, _ = on_and_off(monkeypatch, aligner, amp, reads, mode, cap=64)
        assert c_on["wide_first"] == (marked if marked <= 64 else 0), (mode, c_on)
        assert c_on["band16"] == marked + 100


def edge_batches():
    rng = np.random.Generator(np.random.PCG64(9))
    amp = amplicon(250, 9)
    few4 = [subs(amp, 4, rng) for _ in range(20)]
    copies = [amp] * 300 + [subs(amp, 1, rng) for _ in range(50)]
    d30 = subs(deletion(amp, 100, 30), 1, rng)
    i10 = subs(insertion(amp, 180, 10, rng), 1, rng)
    seeded = [subs(deletion(amp, 60 + q, 16 + q % 25), 1 + q % 3, rng) for q in range(120)]
    return amp, {
        "one": (copies + few4 + [subs(amp, 9, rng)], 1),
        "odd": (copies + few4 + [subs(amp, 7 + q % 4, rng) for q in range(7)], 7),
        "no_dp": (copies, 0),
        "all_marked": ([subs(amp, 6 + q % 6, rng) for q in range(150)] +
                       [subs(deletion(amp, 40 + q, 11 + q % 15), 1, rng) for q in range(51)], 201),
        "del30_ins10": ([d30, i10], 2),
        # reads with La - Lb >= 16: in the list of a resident pass; a call over so many of them
        # seeds them instead (seeded band) and lists the rest
        "seeded": (copies[:200] + seeded + [subs(amp, 8, rng) for _ in range(11)], None),
    }


@pytest.mark.parametrize("mode", ["call", "resident"])
@pytest.mark.parametrize("case", ["one", "odd", "no_dp", "all_marked", "del30_ins10", "seeded"])
def test_edges(monkeypatch, aligner, case, mode):
    amp, batches = edge_batches()
    reads, want = batches[case]
    c_on, _ = on_and_off(monkeypatch, aligner, amp, reads, mode)
    # (a call over a batch with enough reads of La - Lb >= 16 seeds those instead: fewer in the list)
    if want is None or (mode == "call" and case in ("all_marked", "del30_ins10")):
        assert 0 < c_on["wide_first"] <= (want or len(reads)), c_on
    else:
        assert c_on["wide_first"] == want, c_on


def test_hdr_resident_second_pass(monkeypatch, aligner):
    """The HDR pass over the resident batch: most DP reads are marked, far more than the cap, so the
    list joins the first level's and the chunk runs as without it."""
    amp, hdr, buf, off = synth.c3_workload(5000)
    pr = pack_2bit(buf, off)
    n = len(off) - 1
    a = aligner
    monkeypatch.setenv("CRISPR_NW_WIDE_FIRST_CAP", "16")
    res = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("CRISPR_NW_WIDE_FIRST", sw)
        a.set_reference(amp)
        a.align_ops_packed(pr)
        a.set_reference(hdr)
        ob = a.align_ops(None, off, resident=True)
        res[sw] = (ob.stats.copy(), ob.ops_off.copy(), ob.ops[: int(ob.ops_off[n])].copy())
        counts = a.path_counts()
        assert counts["wide_first"] == 0 and counts["band16"] > 16, counts
        if sw == "1":
            chk = every_read(hdr, buf, off, ob, threads=16)
            assert chk["mismatches"] == 0, chk
    same(res["1"], res["0"], "hdr resident")


def test_dual_call(monkeypatch, aligner):
    amp, hdr, buf, off = synth.c3_workload(5000)
    pr = pack_2bit(buf, off)
    n = len(off) - 1
    a = aligner
    res = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("CRISPR_NW_WIDE_FIRST", sw)
        a.set_reference(amp)
        ob1, ob2 = a.align_dual_packed(pr, hdr)
        res[sw] = [(o.stats.copy(), o.ops_off.copy(), o.ops[: int(o.ops_off[n])].copy()) for o in (ob1, ob2)]
        if sw == "1":
            for ref, ob in ((amp, ob1), (hdr, ob2)):
                chk = every_read(ref, buf, off, ob, threads=16)
                assert chk["mismatches"] == 0, chk
    same(res["1"][0], res["0"][0], "dual pass 0")
    same(res["1"][1], res["0"][1], "dual pass 1")


def test_pooled_call(monkeypatch, aligner):
    amps = synth.pooled_amplicons(4, 5)
    reads, which = [], []
    for g, amp in enumerate(amps):
        b, o = synth.reads_from(amp, 1250, 40 + g, synth.PARITY_MIX)
        reads += synth.unpack(b, o)
        which += [g] * 1250
    buf, off = pack_reads(reads)
    which = np.array(which, np.int32)
    pr = pack_2bit(buf, off)
    n = len(off) - 1
    a = aligner
    res = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("CRISPR_NW_WIDE_FIRST", sw)
        ob = a.align_multi_ops(amps, pr, None, which)
        res[sw] = (ob.stats.copy(), ob.ops_off.copy(), ob.ops[: int(ob.ops_off[n])].copy())
        if sw == "1":
            chk = every_read_multi(amps, buf, off, which, ob, threads=16)
            assert chk["mismatches"] == 0, chk
    same(res["1"], res["0"], "pooled")
