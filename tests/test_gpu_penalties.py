"""The aligner against the oracle across needle's -gapopen / -gapextend (tests/penalty_cases.py): every
set of the grid through the packed call (records and runs) and the rows output, the path counters on
either side of each of classify's certificate gates and of the band's int16 gate, the exact int32 kernels
at other penalties, a long amplicon, one context whose penalties change while it lives, and a pooled call.
Every case asks for exact equality with the oracle at the same penalties (tests/test_penalty_model.py holds
the certificates' arguments to the oracle on the CPU; parity with EMBOSS itself stays unpinned)."""
import functools

import numpy as np
import pytest

from crispresso_amd import _lib, synth
from crispresso_amd.aligner import pack_2bit, pack_reads
from crispresso_amd.needle_options import NeedleOptions
from tests import penalty_cases as pc
from tests.every_read import every_read, every_read_multi
from tests.test_gpu_indel import repeat_amplicon
from tests.test_gpu_parity import assert_same
from tests.test_gpu_wide_first import deletion, subs

pytestmark = pytest.mark.gpu

CERTS = ("sub1", "sub2", "sub3", "indel", "window", "indel_past")


@pytest.fixture
def aligners(gpu_aligner_factory):
    """The session's factory, with the contexts a test made closed when it ends: the factory itself keeps
    every context open until the last test of the session, and this file makes several hundred."""
    made = []

    def make(options=None):
        a = gpu_aligner_factory(options)
        made.append(a)
        return a

    yield make
    for a in made:
        a.close()


def _opts(go, ge):
    return NeedleOptions.parse(f"-gapopen={go} -gapextend={ge}")


def _ids(cases):
    return [pc.set_id(*c) for c in cases]


@functools.lru_cache(maxsize=None)
def _grid_batch(La):
    amp = synth.random_amplicon(La, 4000 + La)
    reads = pc.grid_reads(amp, 4100 + La)
    buf, off = pack_reads(reads)
    return amp, reads, buf, off, pack_2bit(buf, off)


def _subset(reads, step, tail):
    """Every step-th read and the last `tail` (the gate-edge reads)."""
    sel = sorted(set(range(0, len(reads), step)) | set(range(len(reads) - tail, len(reads))))
    return pack_reads([reads[i] for i in sel])


def _aligner(factory, go, ge, amp):
    a = factory(_opts(go, ge))
    a.set_reference(amp)
    assert a.scale == pc.scaled(go, ge)[0]
    return a


def _ops_clean(a, amp, buf, off, pr, p, what):
    ob = a.align_ops_packed(pr)
    assert ob.scale == p.scale
    counts = a.path_counts()
    res = every_read(amp, buf, off, ob, threads=8, oracle_params=p)
    assert res["mismatches"] == 0, (what, res, counts)
    return ob, counts


def _full_exact_reads(factory, monkeypatch, amp, pr):
    """What a run that sends every read to the exact kernels reports for these reads: the default penalties
    with the band switched off.  (The packed call counts the reads the band handed on: none on that path.)"""
    monkeypatch.setenv("CRISPR_NW_KERNEL", "full")
    a = factory()
    a.set_reference(amp)
    a.align_ops_packed(pr)
    n = a.exact_reads()
    monkeypatch.delenv("CRISPR_NW_KERNEL")
    return n


# ---------------------------------------------------------------- every set of the grid, both outputs

@pytest.mark.parametrize("mode", ["ops", "rows"])
@pytest.mark.parametrize("go,ge,La", pc.GRID, ids=_ids(pc.GRID))
def test_grid_set_matches_oracle(aligners, oracle, go, ge, La, mode):
    p = oracle.params(go, ge)
    amp, reads, buf, off, pr = _grid_batch(La)
    a = _aligner(aligners, go, ge, amp)
    assert p.scale == a.scale
    if mode == "ops":
        _, counts = _ops_clean(a, amp, buf, off, pr, p, pc.set_id(go, ge, La))
        print("path counts", pc.set_id(go, ge, La), pc.gates_of(go, ge, La), counts)
        band = pc.gates_of(go, ge, La)["band"]
        assert (a.geometry()["tb_mode"] == "diag-int16") == band
        return
    sbuf, soff = _subset(reads, 5, 6)
    batch = a.align_packed(sbuf, soff, mode="rows")
    assert batch.scale == p.scale
    assert_same(oracle, amp, sbuf, soff, batch, f"rows {pc.set_id(go, ge, La)}", params=p)


# ---------------------------------------------------------------- which path took the reads

@pytest.mark.parametrize("maker", ["random", "repeat"])
@pytest.mark.parametrize("go,ge,La", pc.GRID, ids=_ids(pc.GRID))
def test_path_counters_follow_the_gates(aligners, oracle, monkeypatch, go, ge, La, maker):
    """A batch made only of one certificate's reads, on a fresh aligner (no known sequence): where gates()
    has the certificate on it takes reads (exact_copies counts every read that needed no DP), where it
    is off none leaves the DP -- and every read equals the oracle either way.  The one-indel certificate's
    per-read score test of shift 0 counts mismatches up to 2, so it can pass only when O + (k - 1) E <
    2 (m + x): past that (19.5 / 0.5) the gate is open and nothing can be certified.  A last batch holds
    gaps of indel_kmax + 1 and + 2 residues: none may be certified.  On the amplicon laced with homopolymers
    and tandem repeats (gaps slide, shifted diagonals match locally: the per-read checks decide) a certificate
    that is on need not take a read; one that is off still takes none."""
    s, O, E = pc.scaled(go, ge)
    g = pc.gates(s, O, E, La)
    p = oracle.params(go, ge)
    amp = synth.random_amplicon(La, 4000 + La) if maker == "random" else repeat_amplicon(La, 4050 + La)
    kcert = max([k for k in range(1, g["indel_kmax"] + 1) if O + (k - 1) * E < 2 * 9 * s], default=0)
    seen = {}
    for q, cert in enumerate(CERTS):
        reads = pc.certificate_reads(cert, amp, 320, 4200 + 10 * La + q, g["indel_kmax"] if cert == "indel_past" else kcert)
        assert pc.amplicon_copies(amp, reads) == 0
        buf, off = pack_reads(reads)
        pr = pack_2bit(buf, off)
        a = _aligner(aligners, go, ge, amp)
        _, counts = _ops_clean(a, amp, buf, off, pr, p, (pc.set_id(go, ge, La), cert))
        seen[cert] = counts["exact_copies"]
        on = kcert > 0 if cert == "indel" else (False if cert == "indel_past" else g[cert])
        if on:
            assert counts["exact_copies"] > 0 or maker == "repeat", (cert, g, counts)
        else:   # (no read of these batches is a copy of the amplicon; only the window batch holds windows)
            assert counts["exact_copies"] == 0, (cert, g, counts)
        if not g["band"] and cert == "sub3":
            assert a.geometry()["tb_mode"] in ("full-lds", "full-global")
            assert counts["band16"] + counts["band32"] + counts["wide128"] == 0, counts
            assert a.exact_reads() == _full_exact_reads(aligners, monkeypatch, amp, pr)
    print("certified", maker, pc.set_id(go, ge, La), g, seen)


# ---------------------------------------------------------------- the band's int16 gate, both sides

@pytest.mark.parametrize("go,ge,La", pc.BAND_EDGE, ids=_ids(pc.BAND_EDGE))
def test_band_gate_both_sides(aligners, oracle, monkeypatch, go, ge, La):
    """diag_hi = 5 scale La + E (2 La + 300) + O just below 15000 (the band's halfwords closest to their
    range: M >= -4 scale La on a diagonal of mismatches) and at the first length past it (the exact kernels)."""
    p = oracle.params(go, ge)
    band = pc.gates_of(go, ge, La)["band"]
    for amp in (synth.random_amplicon(La, 4300 + La), "A" * La):
        sub, soff = synth.reads_from(amp, 40, 4400 + La)
        reads = pc.gate_edge_reads(amp) + synth.unpack(sub, soff)
        reads += ["C" * (La - 7), "C" * (La + 8), "C" * (La // 2) + "A" * (La - La // 2)]
        buf, off = pack_reads(reads)
        pr = pack_2bit(buf, off)
        a = _aligner(aligners, go, ge, amp)
        _, counts = _ops_clean(a, amp, buf, off, pr, p, (go, ge, La, amp[:4]))
        print("band gate", pc.set_id(go, ge, La), amp[:4], counts)
        if band:
            assert a.geometry()["tb_mode"] == "diag-int16"
            assert counts["band16"] + counts["band32"] + counts["wide128"] > 0, counts
        else:
            assert a.geometry()["tb_mode"] in ("full-lds", "full-global")
            assert counts["band16"] + counts["band32"] + counts["wide128"] == 0, counts
            assert a.exact_reads() == _full_exact_reads(aligners, monkeypatch, amp, pr)
        batch = a.align_packed(buf, off, mode="rows")
        assert_same(oracle, amp, buf, off, batch, f"band gate rows {pc.set_id(go, ge, La)}", params=p)


# ---------------------------------------------------------------- the exact int32 kernels

@pytest.mark.parametrize("exact", ["multi", "split", "wave"])
@pytest.mark.parametrize("La", pc.FULL_LA)
@pytest.mark.parametrize("go,ge", pc.FULL_SETS, ids=_ids(pc.FULL_SETS))
def test_exact_kernels_at_other_penalties(aligners, oracle, monkeypatch, go, ge, La, exact):
    """CRISPR_NW_KERNEL=full: the multi-wave kernel, the one-wave kernel and the two splitting one list
    (as tests/test_gpu_parity.py::test_exact_kernel_work_list selects them)."""
    monkeypatch.setenv("CRISPR_NW_KERNEL", "full")
    if exact != "wave":
        monkeypatch.setenv("CRISPR_NW_EXACT", "multi:7" if exact == "split" else "multi")
    p = oracle.params(go, ge)
    amp = synth.random_amplicon(La, 4500 + La)
    sub, soff = synth.reads_from(amp, 180, 4600 + La, synth.PARITY_MIX)
    reads = synth.unpack(sub, soff) + pc.gate_edge_reads(amp)
    reads += [amp.lower(), "ACGTRYKMSWBDHVNU", "T-C-A" * 3, "N" * 9, synth.random_amplicon(2 * La + 5, 7),
              amp[:La // 3] + amp[La // 3 + La // 5:], amp[:La // 2] + synth.random_amplicon(La // 5, 8) + amp[La // 2:]]
    buf, off = pack_reads(reads)
    a = _aligner(aligners, go, ge, amp)
    batch = a.align_packed(buf, off)
    assert batch.scale == p.scale
    assert_same(oracle, amp, buf, off, batch, f"exact-{exact} {pc.set_id(go, ge, La)}", params=p)
    assert a.geometry()["tb_mode"] in ("full-lds", "full-global")


@pytest.mark.parametrize("go,ge,La", pc.LONG_SETS, ids=_ids(pc.LONG_SETS))
def test_long_amplicon_at_other_penalties(aligners, oracle, go, ge, La):
    """Past 1024 bp every read takes the multi-wave exact kernel (nw_exact.hip), traceback in HBM."""
    p = oracle.params(go, ge)
    amp = synth.random_amplicon(La, 4700 + La)
    sub, soff = synth.reads_from(amp, 28, 4800 + La, synth.PARITY_MIX)
    reads = synth.unpack(sub, soff) + pc.gate_edge_reads(amp)
    reads += [amp[: La // 3], amp[La // 2:], amp[:100] + amp[400:], "ACGTRYKMSWBDHVNU",
              amp[:La // 2] + synth.random_amplicon(60, 3) + amp[La // 2:], synth.random_amplicon(300, 5)]
    buf, off = pack_reads(reads)
    a = _aligner(aligners, go, ge, amp)
    assert_same(oracle, amp, buf, off, a.align_packed(buf, off), f"long ops {pc.set_id(go, ge, La)}", params=p)
    assert_same(oracle, amp, buf, off, a.align_packed(buf, off, mode="rows"), f"long rows {pc.set_id(go, ge, La)}",
                params=p)


# ---------------------------------------------------------------- penalties changed on a live context

def _bytes(ob):
    n = len(ob.ops_off) - 1
    return ob.stats.tobytes(), ob.ops_off.tobytes(), ob.ops[: int(ob.ops_off[n])].tobytes()


def _set_penalties(a, go, ge):
    a._check(a.lib.nw_set_params(a._h, go, ge, 0, 10.0, 0.5, b"EDNAFULL", _lib.NW_TIE_EMBOSS), "nw_set_params")
    a.options = _opts(go, ge)
    a.scale = int(a.lib.nw_score_scale(a._h))


def test_penalties_change_on_a_live_context(aligners, oracle):
    """nw_set_params on a context that holds an amplicon, its tables and a resident batch (the shared
    tables are keyed by scale and gap extend, the amplicon arena by scale): after every change the packed
    call's bytes equal a fresh context's at those penalties and the oracle's alignments; a resident pass
    against the HDR variant (known copies of the amplicon) runs between two changes; the last step, the
    first step's penalties again, gives the first step's bytes; two steps more change gap extend alone and gap
    open alone (the scale, half of the shared tables' key, stays)."""
    La = pc.LA_GATE   # (10 / 0.0625, scale 16, keeps the band at this length: the tables change with it)
    amp = synth.random_amplicon(La, 4900)
    hdr = synth.hdr_amplicon(amp, 4)
    rng = np.random.Generator(np.random.PCG64(4901))
    sub, soff = synth.reads_from(amp, 300, 4902, synth.PARITY_MIX)
    reads = synth.unpack(sub, soff) + pc.indel_reads(amp, 100, 4903) + pc.sub_reads(amp, 60, 4904, 1)
    reads += pc.sub_reads(amp, 60, 4905, 2) + pc.three_sub_reads(amp, 80, rng) + pc.window_reads(amp, rng, 100)
    reads += [hdr] * 20 + pc.gate_edge_reads(amp)
    buf, off = pack_reads(reads)
    pr = pack_2bit(buf, off)
    a = aligners()
    a.set_reference(amp)
    steps = []
    for step, (go, ge) in enumerate(pc.LIVE_SEQUENCE + pc.LIVE_EXTRA):
        p = oracle.params(go, ge)
        _set_penalties(a, go, ge)
        assert a.scale == p.scale
        ob = a.align_ops_packed(pr)
        fresh = _aligner(aligners, go, ge, amp)
        assert _bytes(ob) == _bytes(fresh.align_ops_packed(pr)), (step, go, ge)
        res = every_read(amp, buf, off, ob, threads=8, oracle_params=p)
        assert res["mismatches"] == 0, (step, go, ge, res, a.path_counts())
        steps.append(_bytes(ob))
        if step == 1:   # a resident pass of the batch against the HDR variant, then the amplicon again
            a.set_reference(hdr)
            fresh.set_reference(hdr)
            got = a.align_ops(None, off, resident=True)
            assert _bytes(got) == _bytes(fresh.align_ops(None, off, resident=True)), "resident"
            res = every_read(hdr, buf, off, got, threads=8, oracle_params=p)
            assert res["mismatches"] == 0, ("resident", res)
            a.set_reference(amp)
    last = len(pc.LIVE_SEQUENCE) - 1
    assert pc.LIVE_SEQUENCE[0] == pc.LIVE_SEQUENCE[last] and steps[0] == steps[last]
    assert steps[0] != steps[1]   # (the penalties do change the batch's bytes: the scale at least)


# ---------------------------------------------------------------- pooled

def test_pooled_call_at_other_penalties(aligners, oracle):
    go, ge = pc.POOLED_SET
    p = oracle.params(go, ge)
    rng = np.random.Generator(np.random.PCG64(5000))
    amps = [synth.random_amplicon(La, 5001 + g) for g, La in enumerate(pc.POOLED_LA)]
    reads, which = [], []
    for g, amp in enumerate(amps):
        for q in range(300):
            r = amp if q % 3 == 0 else subs(amp, 1 + q % 4, rng)
            if q % 5 == 0:
                r = deletion(r, 10 + q % 80, 1 + q % 12)
            reads.append(r)
        reads += pc.gate_edge_reads(amp)
        which += [g] * 306
    which = np.array(which, np.int32)
    buf, off = pack_reads(reads)
    a = aligners(_opts(go, ge))
    ob = a.align_multi_ops(amps, pack_2bit(buf, off), None, which)
    assert ob.scale == p.scale == 4
    res = every_read_multi(amps, buf, off, which, ob, threads=8, oracle_params=p)
    assert res["mismatches"] == 0 and res["reads"] == len(reads), res
