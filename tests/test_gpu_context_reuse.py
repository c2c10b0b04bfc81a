"""One context through every kind of call in turn (nw_host.cpp keeps per-amplicon, per-call and
per-chunk state in it): a pooled call in many chunks, a one-chunk packed call on the seeded band and
the wide-first list, a resident pass with known copies, a dual call, -endweight and back, and the
nw_batch_* API.  After each step the records, run offsets and runs are byte-identical to the same
call made on a fresh context, and every read equals the oracle."""
import numpy as np
import pytest

from crispresso_amd import _lib, synth
from crispresso_amd.aligner import pack_2bit, pack_reads
from oracle import oracle_py
from tests.every_read import every_read, every_read_multi
from tests.test_gpu_wide_first import amplicon, deletion, insertion, subs

pytestmark = pytest.mark.gpu


def _batch_b(amp, rng):
    """1,500 reads of the 200 bp amplicon: 45 (3 %, at least 1 in 64: the share that puts a chunk on
    the seeded band) 20-40 bp shorter, 45 of its length with 6-10 substitutions (the wide-first
    list), the rest copies and light edits."""
    reads = [deletion(amp, 40 + 2 * q, 20 + q % 21) for q in range(45)]
    reads += [subs(amp, 6 + q % 5, rng) for q in range(45)]
    for q in range(1410):
        kind = q % 6
        if kind < 2:
            reads.append(amp)
        elif kind < 4:
            reads.append(subs(amp, 1 + q % 3, rng))
        elif kind == 4:
            reads.append(deletion(amp, 20 + q % 150, 1 + q % 9))
        else:
            reads.append(insertion(amp, 20 + q % 150, 1 + q % 6, rng))
    return [reads[i] for i in rng.permutation(len(reads))]


def _pooled(amps, rng):
    reads, which = [], []
    for g, amp in enumerate(amps):
        for q in range(400):
            r = amp if q % 3 == 0 else subs(amp, 1 + q % 4, rng)
            if q % 5 == 0:
                r = deletion(r, 10 + q % 80, 1 + q % 12)
            reads.append(r)
        which += [g] * 400
    return reads, np.array(which, np.int32)


def _bytes(ob):
    n = len(ob.ops_off) - 1
    return ob.stats.tobytes(), ob.ops_off.tobytes(), ob.ops[: int(ob.ops_off[n])].tobytes()


def _set_params(a, end_weight):
    a._check(a.lib.nw_set_params(a._h, 10.0, 0.5, int(end_weight), 10.0, 0.5, b"EDNAFULL", _lib.NW_TIE_EMBOSS),
             "nw_set_params")


def test_one_context_through_every_call_kind(gpu_aligner_factory, oracle, monkeypatch):
    rng = np.random.Generator(np.random.PCG64(808))
    amp_a, amp_b, amp_c = amplicon(120, 1), amplicon(200, 2), amplicon(251, 3)
    hdr = synth.hdr_amplicon(amp_b, 4)
    assert len(hdr) == len(amp_b)
    amps = [amp_a, amp_b, amp_c]
    preads, which = _pooled(amps, rng)
    pbuf, poff = pack_reads(preads)
    ppr = pack_2bit(pbuf, poff)
    buf, off = pack_reads(_batch_b(amp_b, rng))
    pr = pack_2bit(buf, off)
    n = len(off) - 1
    assert pr.lens is not None and ppr.lens is not None

    def clean(ob, ref, what, params=None):
        chk = every_read(ref, buf, off, ob, threads=16, oracle_params=params)
        assert chk["mismatches"] == 0, (what, chk)

    def pooled(a):
        monkeypatch.setenv("CRISPR_NW_CHUNK", "97")   # several chunks per group: each restores its group's configuration
        ob = a.align_multi_ops(amps, ppr, None, which)
        monkeypatch.delenv("CRISPR_NW_CHUNK")
        return ob

    def packed(a):
        a.set_reference(amp_b)
        return a.align_ops_packed(pr)   # one chunk: the wide-first list is eligible

    def resident(a):
        a.set_reference(hdr)
        return a.align_ops(None, off, resident=True)

    def dual(a):
        a.set_reference(amp_b)
        monkeypatch.setenv("CRISPR_NW_CHUNK", "613")
        obs = a.align_dual_packed(pr, hdr)
        monkeypatch.delenv("CRISPR_NW_CHUNK")
        return obs

    def endweight(a):
        _set_params(a, True)
        a.set_reference(amp_b)
        ob = a.align_ops_packed(pr)
        _set_params(a, False)
        return ob

    def batch_api(a):
        a.set_reference(amp_b)
        a.upload_packed(pr)
        a.run_async()
        a.sync()
        return a.download_ops(n)

    a = gpu_aligner_factory()
    # 1. grouped pooled call
    got = pooled(a)
    fresh = gpu_aligner_factory()
    assert _bytes(got) == _bytes(pooled(fresh)), "pooled"
    chk = every_read_multi(amps, pbuf, poff, which, got, threads=16)
    assert chk["mismatches"] == 0, chk
    # 2. packed call with lengths, one chunk: the seeded band and the wide-first list
    step2 = packed(a)
    counts = a.path_counts()
    print("step 2 path counts:", counts)
    # (1,500 reads: the first level hands its give-ups straight to the wide level, so only the
    # seeded list reaches the 32-diagonal level)
    assert counts["wide_first"] > 0 and counts["band32"] > 0, counts
    fresh = gpu_aligner_factory()
    assert _bytes(step2) == _bytes(packed(fresh)), "packed"
    clean(step2, amp_b, "packed")
    step2 = _bytes(step2)
    # 3. resident pass of that batch against the HDR variant (known copies)
    got = resident(a)
    assert _bytes(got) == _bytes(resident(fresh)), "resident"   # (fresh made the same call 2 just before)
    clean(got, hdr, "resident")
    # 4. dual call
    got = dual(a)
    fresh = gpu_aligner_factory()
    want = dual(fresh)
    assert _bytes(got[0]) == _bytes(want[0]) and _bytes(got[1]) == _bytes(want[1]), "dual"
    clean(got[0], amp_b, "dual pass 0")
    clean(got[1], hdr, "dual pass 1")
    # 5. -endweight (configure leaves the band path after a band configuration), then the defaults again
    got = endweight(a)
    fresh = gpu_aligner_factory()
    assert _bytes(got) == _bytes(endweight(fresh)), "endweight"
    clean(got, amp_b, "endweight", oracle_py.params(10.0, 0.5, True, 10.0, 0.5))
    assert _bytes(packed(a)) == step2, "packed after endweight"
    # 6. nw_batch_upload_packed + run_async + download_ops
    got = batch_api(a)
    fresh = gpu_aligner_factory()
    assert _bytes(got) == _bytes(batch_api(fresh)), "batch API"
    clean(got, amp_b, "batch API")
