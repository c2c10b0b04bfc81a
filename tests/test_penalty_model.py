"""Classify's certificates away from -gapopen=10 -gapextend=0.5, on the CPU: Python restatements of the
one-substitution, three-substitution and one-indel checks (nw_band.hip), run at every penalty set of
tests/penalty_cases.GRID on which the certificate's gate is open, against the oracle at those penalties.
Every read a restatement accepts must be aligned by the oracle as the certificate writes it.  The GPU
side (tests/test_gpu_penalties.py) holds the kernels to the oracle on the same sets; this file pins the
arguments themselves, and that the grid keeps a set on each side of every gate."""
import numpy as np
import pytest

from oracle import oracle_py
from tests import penalty_cases as pc
from tests.test_certificate_model import certified, three_sub_reads
from tests.test_gpu_indel import SUB, repeat_amplicon

SETS = sorted({(go, ge) for go, ge, _ in pc.GRID})
FLOOR = 300   # reads a model must accept per set, so that bad == 0 says something


def _sets(gate):
    """The grid's sets on which `gate` is open at a length the certificates take (La <= 256)."""
    return [pytest.param(go, ge, id=pc.set_id(go, ge)) for go, ge in SETS if pc.gates_of(go, ge, 200)[gate]]


def _oracle(amp, reads, go, ge):
    buf = np.frombuffer("".join(reads).encode(), np.uint8)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in reads])
    return oracle_py.align_batch(amp, buf, off, oracle_py.params(go, ge), nthreads=4)


def _row(aln, q, k, L):
    return aln[q, k, :L].tobytes().decode()


# ---------------------------------------------------------------- the grid keeps both sides of every gate

def test_grid_straddles_every_gate():
    seen = {}
    for go, ge, La in pc.gpu_lengths():
        for gate, v in pc.gates_of(go, ge, La).items():
            seen.setdefault(gate, set()).add(v)
    for gate in ("band", "sub1", "sub2", "sub3", "window"):
        assert seen[gate] == {True, False}, (gate, seen[gate])
    # the one-indel certificate: off, its smallest gap, a bound set by E (2), by O (5, 9) and by kIndelMax
    assert {0, 1, 2, 5, 9, pc.K_INDEL_MAX} <= seen["indel_kmax"], seen["indel_kmax"]


def test_grid_pairs_sit_half_a_unit_apart():
    """Each certificate gate is straddled by two sets that differ by one scaled unit of gap open."""
    g = {(go, ge): pc.gates_of(go, ge, pc.LA_GATE) for go, ge, _ in pc.GRID}
    for gate, off, on in (("sub1", (4.0, 0.5), (4.5, 0.5)), ("sub2", (8.0, 0.5), (8.5, 0.5)),
                          ("sub3", (9.0, 0.5), (9.5, 0.5)), ("window", (9.0, 0.5), (9.5, 0.5))):
        assert not g[off][gate] and g[on][gate], (gate, g[off], g[on])
    assert g[(19.5, 0.5)]["indel_kmax"] == 1 and g[(20.0, 0.5)]["indel_kmax"] == 0
    for go, ge, La in pc.BAND_EDGE:
        assert pc.gates_of(go, ge, La)["band"] == (La in (896, 177)), (go, ge, La)
    assert not pc.gates_of(0.5, 1.0, pc.LA)["band"] and pc.gates_of(1.0, 1.0, pc.LA)["band"]
    assert pc.gates_of(0.0, 0.0, pc.LA)["band"]


def test_scale_follows_the_oracle():
    for go, ge in SETS + [(10.0, 0.0625)]:
        p = oracle_py.params(go, ge)
        assert (p.scale, p.gap_open, p.gap_extend) == pc.scaled(go, ge)


# ---------------------------------------------------------------- three substitutions

@pytest.mark.parametrize("go,ge", _sets("sub3"))
def test_three_substitution_model(go, ge):
    s, O, E = pc.scaled(go, ge)
    M, X = 5 * s, 4 * s
    rng = np.random.Generator(np.random.PCG64(5))
    amps = [repeat_amplicon(120, 40 + q) for q in range(4)]
    accepted = bad = 0
    for amp in amps:
        sel = [r for r in three_sub_reads(amp, 250, rng) if certified(amp, r, M, X, O, E)]
        accepted += len(sel)
        if not sel:
            continue
        res, _ = _oracle(amp, sel, go, ge)
        La = len(amp)
        ok = ((res["aln_len"] == La) & (res["n_ident"] == La - 3) & (res["n_gaps"] == 0) &
              (res["score"] == M * La - 3 * (M + X)) & (res["end_i"] == La) & (res["end_j"] == La))
        bad += int((~ok).sum())
    assert accepted >= FLOOR, accepted
    assert bad == 0


# ---------------------------------------------------------------- one substitution

def sub1_certified(amp, r):
    """classify, k == 1: a mismatch on each of the diagonals +1 (read base q + 1 against amplicon base q)
    and -1 (read base q against amplicon base q + 1), q <= La - 2."""
    La = len(amp)
    if len(r) != La or sum(a != b for a, b in zip(amp, r)) != 1:
        return False
    return any(r[q + 1] != amp[q] for q in range(La - 1)) and any(r[q] != amp[q + 1] for q in range(La - 1))


def _every_one_sub(amp):
    return [amp[:p] + b + amp[p + 1:] for p in range(len(amp)) for b in "ACGT" if b != amp[p]]


@pytest.mark.parametrize("go,ge", _sets("sub1"))
def test_one_substitution_model(go, ge):
    s, O, E = pc.scaled(go, ge)
    M, X = 5 * s, 4 * s
    accepted = bad = 0
    for La in (1, 2, 3, 5, 17, 60, 130):
        for seed in range(3):
            amp = repeat_amplicon(La, 60 + 7 * La + seed)
            sel = [r for r in _every_one_sub(amp) if sub1_certified(amp, r)]
            accepted += len(sel)
            if not sel:
                continue
            res, _ = _oracle(amp, sel, go, ge)
            ok = ((res["aln_len"] == La) & (res["n_ident"] == La - 1) & (res["n_gaps"] == 0) &
                  (res["score"] == M * (La - 1) - X) & (res["end_i"] == La) & (res["end_j"] == La))
            bad += int((~ok).sum())
    assert accepted >= FLOOR, accepted
    assert bad == 0


# ---------------------------------------------------------------- one indel

def cert_indel(amp, r, M, X, O, E):
    """nw_band.hip cert_indel, statement by statement -> the gap's index gk (runs M gk, the gap, M the
    rest), or None.  s is the shorter of amplicon and read, l the longer."""
    La = len(amp)
    dl = len(r) - La
    kab = abs(dl)
    if kab < 1:
        return None
    dele = dl < 0
    s, l = (r, amp) if dele else (amp, r)
    Ls, Ll = len(s), len(l)
    S = M * Ls - O - (kab - 1) * E

    def mism(lw, sw, sh, P):   # positions i < P with lw[i + sh] != sw[i] (past either end: no mismatch)
        return [i for i in range(max(P, 0)) if i + sh < len(lw) and i < len(sw) and lw[i + sh] != sw[i]]

    def ends(lw, sw, sh, P):
        pos = mism(lw, sw, sh, P)
        return (pos[0], pos[-1] + 1) if pos else (P, 0)

    def cnt(f, g, P):
        return 0 if f == P else (1 if f == g - 1 else 2)

    def enough(lw, sw, sh, P):
        need = 0
        while need <= 2 and not M * (P - need) - X * need < S:
            need += 1
        return need <= 2 and len(mism(lw, sw, sh, P)) >= need

    o = True
    f0, fmax_all, fmax_1, gk = Ls, -1, -1, 0
    for sh in range(kab + 1):
        f, g = ends(l, s, sh, Ls)
        c = cnt(f, g, Ls)
        o = o and M * (Ls - c) - X * c < S
        if sh == 0:
            f0 = f
        if sh > 0:
            o = o and g > (fmax_1 if sh == kab else fmax_all)
        if sh == kab:
            gk = g
        fmax_all = max(fmax_all, f)
        if sh > 0:
            fmax_1 = max(fmax_1, f)
    for sh in range(kab + 1, kab + 4):
        o = o and enough(l, s, sh, Ll - sh)
    for sh in range(1, 4):
        o = o and enough(s, l, sh, Ls - sh)
    return gk if o and 1 <= gk <= f0 else None


def _indel_inputs(amp, k_lo, k_hi, rng, n):
    """Deletions, random insertions and tandem-duplication insertions of k_lo .. k_hi residues."""
    La = len(amp)
    out = []
    for _ in range(n):
        k = int(rng.integers(k_lo, k_hi + 1))
        if La - k - 1 <= 1:
            continue
        p = int(rng.integers(1, La - k - 1))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            out.append(amp[:p] + amp[p + k:])
        elif kind == 1:
            out.append(amp[:p] + "".join(rng.choice(list("ACGT"), k)) + amp[p:])
        elif kind == 2:
            out.append(amp[:p] + amp[max(0, p - k):p].rjust(k, amp[0]) + amp[p:])
        else:
            out.append(amp[:p] + amp[p:p + k].ljust(k, amp[-1]) + amp[p:])
    return out


def _indel_model(go, ge, k_lo, k_hi, n=500):
    """-> (certified, wrong): reads of one gap of k_lo .. k_hi residues the restatement certifies, and those
    of them the oracle aligns otherwise than M gk, gap, M rest with score m Ls - O - (k - 1) E."""
    s, O, E = pc.scaled(go, ge)
    M, X = 5 * s, 4 * s
    rng = np.random.Generator(np.random.PCG64(int(16 * go) * 1009 + int(16 * ge) + k_hi))
    accepted = bad = 0
    for La in (17, 40, 90, 200):
        amp = repeat_amplicon(La, 300 + La)
        reads = sorted(set(_indel_inputs(amp, k_lo, k_hi, rng, n)))
        gks = [cert_indel(amp, r, M, X, O, E) for r in reads]
        sel = [(r, g) for r, g in zip(reads, gks) if g is not None]
        accepted += len(sel)
        if not sel:
            continue
        res, aln = _oracle(amp, [r for r, _ in sel], go, ge)
        for q, (r, gk) in enumerate(sel):
            k = abs(len(r) - La)
            Ls, Ll = min(len(r), La), max(len(r), La)
            if len(r) < La:
                want = (amp, r[:gk] + "-" * k + r[gk:])
            else:
                want = (amp[:gk] + "-" * k + amp[gk:], r)
            rec = res[q]
            ok = (rec["aln_len"] == Ll and rec["n_ident"] == Ls and rec["n_gaps"] == k and
                  rec["score"] == M * Ls - O - (k - 1) * E and rec["end_i"] == La and rec["end_j"] == len(r) and
                  (_row(aln, q, 0, Ll), _row(aln, q, 2, Ll)) == want)
            bad += not ok
    return accepted, bad


def _indel_sets():
    return [pytest.param(go, ge, id=pc.set_id(go, ge)) for go, ge in SETS if pc.gates_of(go, ge, 200)["indel_kmax"] > 0]


@pytest.mark.parametrize("go,ge", _indel_sets())
def test_one_indel_model(go, ge):
    kmax = pc.gates_of(go, ge, 200)["indel_kmax"]
    accepted, bad = _indel_model(go, ge, 1, kmax)
    assert bad == 0, (accepted, bad)
    if (go, ge) == (19.5, 0.5):
        # The gate O + (k - 1) E < 4 m holds by one unit, but the per-read score test of shift 0 cannot:
        # its mismatches are counted up to 2, and m (Ls - 2) - 2 x < m Ls - O needs O < 2 (m + x) = 36.
        # This run certified 0 of about 1,700 reads; only bad == 0 is asserted.
        return
    assert accepted >= FLOOR, accepted


def test_one_indel_model_needs_its_gate():
    """-gapopen=5 -gapextend=2 (scale 1, O 5, E 2: indel_kmax 3): with gaps of four residues the same checks
    certify reads the oracle aligns otherwise -- the gate is what makes the argument true."""
    assert pc.gates_of(5.0, 2.0, 200)["indel_kmax"] == 3
    accepted, bad = _indel_model(5.0, 2.0, 1, 3)
    assert accepted >= FLOOR and bad == 0, (accepted, bad)
    accepted, bad = _indel_model(5.0, 2.0, 4, 4, n=1500)
    assert accepted > 0 and bad >= 1, (accepted, bad)
