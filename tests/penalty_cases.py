"""The -gapopen / -gapextend sets the aligner is held to the oracle at, the gates those sets are chosen
around, and the reads that go with them (tests/test_penalty_model.py on the CPU, tests/test_gpu_penalties.py
on the GPU).  Not a test module.

gates() restates, line for line, what decides the path of a read when the penalties change:
nw_set_params' scale (nw_host.cpp), configure_wave's band gate (nw_host.cpp, "certified diagonal band")
and nw_band_classify's certificate switches (nw_band.hip: sub1_ok, sub2_ok, indel_kmax, sub3_ok, win_ok).
The certificates run in classify, which runs on the band path only, for an A C G T amplicon, ops output."""
from __future__ import annotations

import numpy as np

from crispresso_amd import synth
from tests.test_certificate_model import three_sub_reads
from tests.test_gpu_indel import SUB, indel_reads, sub_reads
from tests.test_gpu_windows import _window_reads as window_reads

K_INDEL_MAX = 10   # nw_band.hip kIndelMax


def scaled(gap_open: float, gap_extend: float):
    """nw_set_params: the smallest scale of 1, 2, 4, 8, 16 at which both penalties are whole -> (scale, O, E)."""
    for s in (1, 2, 4, 8, 16):
        o, e = gap_open * s, gap_extend * s
        if o == int(o) and e == int(e):
            return s, int(o), int(e)
    raise ValueError("penalties are not multiples of 1/16")


def gates(scale: int, O: int, E: int, La: int) -> dict:
    """Which paths are open for an A C G T amplicon of La bases (packed input, ops output, free end gaps)."""
    # configure_wave: diag_hi < 15000, La <= 1024, gap_extend >= 0, gap_open >= gap_extend
    diag_hi = 5 * scale * La + E * (2 * La + 300) + O
    band = La <= 1024 and diag_hi < 15000 and E >= 0 and O >= E
    nd = (La + 3) // 4
    maxsub = 5 * scale            # KernelArgs::band_maxsub
    sc5 = maxsub // 5
    sub1 = band and nd <= 64 and maxsub == 5 * sc5 and O > 4 * sc5 and E >= 0
    mt2, xl = maxsub, 9 * sc5
    sub2 = (sub1 and 2 * O > 2 * xl - mt2 and O > 2 * xl - 2 * mt2 and O > xl - mt2 and xl < 2 * mt2 and
            (2 * xl - mt2) // xl + 1 == 2 and (2 * xl - 2 * mt2) // xl + 1 == 1 and (2 * xl - 3 * mt2) // xl + 1 == 1)
    indel_kmax = 0
    if sub1:
        for k in range(1, K_INDEL_MAX + 1):
            p = (k - 1) * E
            if not (maxsub > p and O > p and O + p < 4 * maxsub):
                break
            indel_kmax = k
    m3, x3 = maxsub, 4 * sc5
    D3 = 3 * (m3 + x3)
    sub3 = (sub2 and x3 < m3 and 4 * m3 + O > D3 and 2 * m3 + 2 * O > D3 and 3 * O > D3 and
            m3 + 2 * O + (m3 + x3) > D3)
    window = band and maxsub == 5 * sc5 and E >= 0 and O > xl and La <= 1024
    return {"band": band, "sub1": sub1, "sub2": sub2, "sub3": sub3, "window": window, "indel_kmax": indel_kmax}


def gates_of(go: float, ge: float, La: int) -> dict:
    return gates(*scaled(go, ge), La)


LA = 250        # the grid's amplicon length ...
LA_GATE = 177   # ... and where a pair of sets straddles a certificate gate (and scale 16 keeps the band)

# (gapopen, gapextend, La): what each reaches is in the comment; the tests take it from gates()
GRID = [
    (10.0, 0.5, LA),              # 2, 20, 1: the default (control)
    (12.0, 1.0, LA),              # 1, 12, 1: scale 1
    (5.5, 0.25, LA_GATE),         # 4, 22, 1: scale 4; sub1 only
    (4.0, 0.5, LA_GATE),          # 2, 8, 1: sub1 off
    (4.5, 0.5, LA_GATE),          # 2, 9, 1: sub1 on
    (8.0, 0.5, LA_GATE),          # 2, 16, 1: sub2 off
    (8.5, 0.5, LA_GATE),          # 2, 17, 1: sub2 on
    (9.0, 0.5, LA_GATE),          # 2, 18, 1: sub3 and window off
    (9.5, 0.5, LA_GATE),          # 2, 19, 1: sub3 and window on
    (19.5, 0.5, LA_GATE),         # 2, 39, 1: one-indel gaps of 1
    (20.0, 0.5, LA_GATE),         # 2, 40, 1: no one-indel certificate
    (10.0, 0.0, LA),              # 1, 10, 0: every gap length ties
    (10.0, 2.5, LA),              # 2, 20, 5: one-indel gaps of up to 2
    (10.0, 5.0, LA),              # 1, 10, 5: of 1
    (1.0, 1.0, LA),               # 1, 1, 1: O = E; no certificate, band on
    (0.0, 0.0, LA),               # 1, 0, 0: free gaps; band on
    (0.5, 1.0, LA),               # 2, 1, 2: O < E: the exact kernels
    (10.0625, 0.0625, LA_GATE),   # 16, 161, 1: scale 16
    (50.0, 5.0, LA),              # 1, 50, 5
    (999.5, 0.5, LA),             # 2, 1999, 1: large O
]
# the band gate's two sides (diag_hi just below / at or above 15000)
BAND_EDGE = [(50.0, 5.0, 896), (50.0, 5.0, 897), (10.0625, 0.0625, 177), (10.0625, 0.0625, 178)]
# every read through the exact int32 kernels
FULL_SETS = [(12.0, 1.0), (10.0, 0.0), (1.0, 1.0), (0.5, 1.0), (999.5, 0.5)]
FULL_LA = (65, 250)
LONG_SETS = [(12.0, 1.0, 1025), (10.0, 0.0, 1025)]
LIVE_SEQUENCE = [(10.0, 0.5), (12.0, 1.0), (10.0, 2.5), (10.0, 0.0625), (10.0, 0.5)]
# ... and two steps more that keep the scale: only gap extend changes (2, 20, 1 -> 2, 20, 5), then only gap open
LIVE_EXTRA = [(10.0, 2.5), (4.0, 2.5)]
POOLED_SET = (5.5, 0.25)
POOLED_LA = (120, 200, 251)


def set_id(go: float, ge: float, La=None) -> str:
    return f"{go:g}/{ge:g}" + (f"@{La}" if La is not None else "")


def gpu_lengths() -> list:
    """Every (gapopen, gapextend, La) the GPU tests run."""
    out = list(GRID) + list(BAND_EDGE) + list(LONG_SETS)
    out += [(go, ge, La) for go, ge in FULL_SETS for La in FULL_LA]
    out += [(go, ge, LA_GATE) for go, ge in LIVE_SEQUENCE + LIVE_EXTRA]
    out += [POOLED_SET + (La,) for La in POOLED_LA]
    return out


COMPLEMENT = str.maketrans("ACGT", "CATG")   # every base changes: A <-> C, G <-> T


def gate_edge_reads(amp: str) -> list:
    """The amplicon, its base-wise "complement" (every pair of the main diagonal mismatches), a poly-C read
    (against a poly-A amplicon every pair of every diagonal mismatches), reads of La - 7 and La + 8 bases
    (the pair sits at the edges of the 16-diagonal band, diagonals -7 .. 8) and an empty read."""
    La = len(amp)
    rng = np.random.Generator(np.random.PCG64(La))
    longer = amp[: La // 2] + "".join(rng.choice(list("ACGT"), 8)) + amp[La // 2:]
    return [amp, amp.translate(COMPLEMENT), "C" * La, amp[: La // 3] + amp[La // 3 + 7:] if La > 7 else amp[:1],
            longer, ""]


def one_indel_reads(amp: str, n: int, seed: int, kmax: int, kmin: int = 1) -> list:
    """One deletion, one insertion of random bases or one tandem duplication of kmin .. kmax residues, away
    from the ends (no read is a window of the amplicon within one substitution)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    La = len(amp)
    out = []
    for _ in range(n):
        k = int(rng.integers(kmin, kmax + 1))
        p = int(rng.integers(20, La - 30))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            out.append(amp[:p] + amp[p + k:])
        elif kind == 1:
            out.append(amp[:p] + "".join(rng.choice(list("ACGT"), k)) + amp[p:])
        else:
            out.append(amp[:p] + amp[p - k:p] + amp[p:])
    return out


def pure_window_reads(amp: str, n: int, seed: int) -> list:
    """Windows of 32 .. La - 16 bases, exact or with one substitution (too short for a one-indel read)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    La = len(amp)
    out = []
    for q in range(n):
        Lb = int(rng.integers(32, La - 15))
        s = int(rng.integers(0, La - Lb + 1))
        r = amp[s:s + Lb]
        if q % 2:
            p = int(rng.integers(0, Lb))
            r = r[:p] + SUB[r[p]] + r[p + 1:]
        out.append(r)
    return out


def certificate_reads(cert: str, amp: str, n: int, seed: int, kmax: int = 1) -> list:
    """A batch made only of one certificate's reads (none equals the amplicon)."""
    if cert in ("sub1", "sub2"):
        return sub_reads(amp, n, seed, int(cert[3]))
    if cert == "sub3":
        return three_sub_reads(amp, n, np.random.Generator(np.random.PCG64(seed)))
    if cert == "indel":
        return one_indel_reads(amp, n, seed, max(kmax, 1))
    if cert == "indel_past":   # one or two residues more than the certificate's largest gap
        return one_indel_reads(amp, n, seed, kmax + 2, kmax + 1)
    if cert == "window":
        return pure_window_reads(amp, n, seed)
    raise ValueError(cert)


def grid_reads(amp: str, seed: int) -> list:
    """About 1,500 reads: the parity mix, one-indel reads (and a few with a substitution), one to three
    substitutions, windows, and the gate-edge reads."""
    rng = np.random.Generator(np.random.PCG64(seed))
    buf, off = synth.reads_from(amp, 300, seed, synth.PARITY_MIX)
    reads = synth.unpack(buf, off)
    reads += indel_reads(amp, 300, seed + 1)
    reads += three_sub_reads(amp, 300, rng)
    reads += sub_reads(amp, 200, seed + 2, 1) + sub_reads(amp, 200, seed + 3, 2)
    reads += window_reads(amp, rng, 200)
    reads += gate_edge_reads(amp)
    return reads


def amplicon_copies(amp: str, reads: list) -> int:
    return sum(r.upper() == amp for r in reads)
