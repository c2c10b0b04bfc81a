"""The allele grouping on the host (include/crispr_alleles.h: nwa_group_host,
nwa_reads_have_lower) against a plain dict over (tag, bytes), and crispresso_amd.alleles'
allele_table / merge_allele_tables against quantify.run_summary's df_alleles over the per-read
DataFrame (rows and classes from the CPU oracle).  No GPU."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest

from crispresso_amd import _lib, alleles, quantify, synth
from tests import alleles_cases as ac

FAMILIES = ac.families()


def test_header_and_binding_agree():
    from tests.test_abi import declared_symbols

    assert declared_symbols("crispr_alleles.h", "nwa_") == set(_lib.ALLELE_EXPORTS)
    exported = _lib.exported_symbols()
    assert all(exported[k] for k in _lib.ALLELE_EXPORTS)


def host_group(reads, keep=None, tag=None, cap=None, want_gor=True, nthreads=0):
    lib = _lib.load()
    n = len(reads)
    buf, off = ac.pack(reads)
    keep = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    tag = None if tag is None else np.ascontiguousarray(tag, np.int32)
    cap = n if cap is None else cap
    first = np.full(max(cap, 1), -5, np.int64)
    count = np.full(max(cap, 1), -5, np.int64)
    gor = np.full(max(n, 1), -5, np.int32) if want_gor else None
    ng = ctypes.c_int64(-5)
    rc = lib.nwa_group_host(_lib.ptr(buf), _lib.ptr(off), n, _lib.ptr(keep), _lib.ptr(tag), _lib.ptr(first),
                            _lib.ptr(count), cap, _lib.ptr(gor), ctypes.byref(ng), nthreads)
    k = max(0, min(int(ng.value), cap))
    return rc, first[:k].tolist(), count[:k].tolist(), None if gor is None else gor[:n].tolist(), int(ng.value)


@pytest.mark.parametrize("name", sorted(FAMILIES))
@pytest.mark.parametrize("nthreads", [1, 0])
def test_group_host_equals_dict(name, nthreads):
    reads, keep, tag = FAMILIES[name]
    want = ac.expected_groups(reads, keep, tag)
    rc, first, count, gor, ng = host_group(reads, keep, tag, nthreads=nthreads)
    assert rc == 0 and ng == len(want[0])
    assert (first, count, gor) == want
    assert all(a < b for a, b in zip(first, first[1:]))
    # group_of_read is optional
    rc, first, count, gor, ng = host_group(reads, keep, tag, want_gor=False, nthreads=nthreads)
    assert rc == 0 and (first, count) == want[:2] and gor is None


def test_group_host_many_threads_large():
    """Enough reads for several hash partitions (one table per host thread)."""
    reads = ac.random_reads(20000, 3, pool=900, lengths=(30, 31, 32, 33, 64, 150))
    tag = np.arange(20000, dtype=np.int32) % 2
    want = ac.expected_groups(reads, None, tag)
    rc, first, count, gor, ng = host_group(reads, None, tag, nthreads=4)
    assert rc == 0 and (first, count, gor) == want


def test_capacity_one_short():
    reads, keep, tag = FAMILIES["size5000"]
    want = ac.expected_groups(reads)
    need = len(want[0])
    rc, first, count, gor, ng = host_group(reads, cap=need - 1)
    assert rc == _lib.NW_E_CAPACITY and ng == need
    rc, first, count, gor, ng = host_group(reads, cap=need)
    assert rc == 0 and (first, count, gor) == want
    rc, *_ = host_group(reads, cap=0)
    assert rc == _lib.NW_E_CAPACITY


def test_invalid_counts():
    lib = _lib.load()
    ng = ctypes.c_int64()
    off = np.zeros(2, np.int64)
    buf = np.zeros(4, np.uint8)
    out = np.zeros(1, np.int64)
    for n in (-1, 2 ** 31):
        assert lib.nwa_group_host(_lib.ptr(buf), _lib.ptr(off), n, None, None, _lib.ptr(out), _lib.ptr(out), 1, None,
                                  ctypes.byref(ng), 1) == _lib.NW_E_INVALID
    assert lib.nwa_reads_have_lower(_lib.ptr(buf), _lib.ptr(off), -1, 1) == _lib.NW_E_INVALID


def test_lowercase_kept_apart():
    reads = [b"ACGT", b"acgt", b"ACGT", b"ACGt", b"acgt", b"", b"ACGT"]
    buf, off = ac.pack(reads)
    assert alleles.reads_have_lower(buf, off)
    assert not alleles.reads_have_lower(*ac.pack([b"ACGT", b"NNN-", b"", b"@[`{"]))   # the bytes around a-z
    assert alleles.reads_have_lower(*ac.pack([b"ACGT" * 100 + b"z"]))
    assert not alleles.reads_have_lower(*ac.pack([]))
    g = alleles.group_reads_host(buf, off, want_group_of_read=True)
    assert g.first.tolist() == [0, 1, 3, 5] and g.count.tolist() == [3, 2, 1, 1]
    assert g.group_of_read.tolist() == [0, 1, 0, 2, 1, 3, 0]
    # group_reads without an aligner is the host path
    g2 = alleles.group_reads(None, buf, off)
    assert g2.first.tolist() == g.first.tolist() and g2.count.tolist() == g.count.tolist()


def test_python_wrapper_keep_and_tag():
    reads, keep, tag = FAMILIES["keep_third_tags"]
    buf, off = ac.pack(reads)
    want = ac.expected_groups(reads, keep, tag)
    g = alleles.group_reads_host(buf, off, keep, tag, want_group_of_read=True)
    assert (g.first.tolist(), g.count.tolist(), g.group_of_read.tolist()) == want
    assert len(g) == len(want[0]) and g.collided == 0
    g = alleles.group_reads_host(buf, off, np.zeros(len(reads), bool))
    assert len(g) == 0 and g.group_of_read is None


# ------------------------------------------------------------------ allele_table

@functools.lru_cache(maxsize=None)
def quantified_batch():
    """3,000 PARITY_MIX reads aligned and quantified by the CPU oracle: the ops batch, the
    per-read results ([n][4], as nwq_read holds them), the kept reads (printed identity > 60)
    and the quantified per-read DataFrame of the kept reads."""
    from crispresso_amd.needle import ops_to_dataframe
    from oracle import quant_oracle as qo
    from tests.helpers import ops_from_batch, oracle_batch

    amp = synth.random_amplicon(250, 21)
    buf, off = synth.reads_from(amp, 3000, 22, synth.PARITY_MIX)
    n = len(off) - 1
    ob = ops_from_batch(oracle_batch(amp, buf, off))
    df = ops_to_dataframe(ob, amp, buf, off, [f"r{i}" for i in range(n)], "ref")
    assert len(df) == n
    keep = (df["score_ref"] > 60.0).to_numpy()
    cuts = qo.cut_points(amp, amp[105:125])
    prm = qo.QuantParams(len_amplicon=len(amp), include_idxs=frozenset(qo.include_idxs(len(amp), cuts, 1, 15, 15)))
    um = (df["score_ref"] == 100).to_numpy()
    sel = np.flatnonzero(keep)
    res = qo.process_rows(df["ref_seq"].iloc[sel].tolist(), df["align_str"].iloc[sel].tolist(),
                          df["align_seq"].iloc[sel].tolist(), um[sel], None, None, prm)
    cls = np.where(um[sel], 0, res["cls"])
    rr = np.zeros((n, 4), np.int32)
    rr[sel, 0] = cls
    for c, k in ((1, "n_mutated"), (2, "n_inserted"), (3, "n_deleted")):
        rr[sel, c] = np.where(cls == 0, 0, res[k])
    dfk = df.iloc[sel].copy()
    for k, v in qo.class_flags(res["cls"], um[sel]).items():
        dfk[k] = v
    for c, k in ((1, "n_mutated"), (2, "n_inserted"), (3, "n_deleted")):
        dfk[k] = rr[sel, c].astype(np.int64)
    return amp, buf, off, ob, rr, keep, dfk, cuts


def test_allele_table_equals_run_summary():
    amp, buf, off, ob, rr, keep, dfk, cuts = quantified_batch()
    want = quantify.run_summary(dfk, len(amp), cuts)["df_alleles"]
    groups = alleles.group_reads(None, buf, off, keep=keep)
    assert int(groups.count.sum()) == int(keep.sum()) < len(keep)
    assert len(want) < len(groups) + 1 and len(groups) < int(keep.sum())     # reads repeat; rows are per allele
    got = alleles.allele_table(amp, buf, off, ob, rr, groups)
    pd.testing.assert_frame_equal(got.reset_index(drop=True), want.reset_index(drop=True))
    assert got["#Reads"].sum() == keep.sum() and abs(got["%Reads"].sum() - 100.0) < 1e-9
    # the structured form of nwq_read is accepted too
    got2 = alleles.allele_table(amp, buf, off, ob, rr.copy().view(_lib.NWQ_READ_DTYPE).reshape(-1), groups)
    pd.testing.assert_frame_equal(got2, got)


def test_allele_table_rejects_foreign_results():
    amp, buf, off, ob, rr, keep, dfk, cuts = quantified_batch()
    groups = alleles.group_reads(None, buf, off, keep=keep)
    with pytest.raises(alleles.AlleleError):
        alleles.allele_table(amp, buf, off, ob, rr[:-1], groups)
    bad = rr.copy()
    bad[groups.first[0], 0] = -1
    with pytest.raises(alleles.AlleleError):
        alleles.allele_table(amp, buf, off, ob, bad, groups)


def test_merge_of_split_batch_equals_whole():
    amp, buf, off, ob, rr, keep, dfk, cuts = quantified_batch()
    whole = alleles.allele_table(amp, buf, off, ob, rr, alleles.group_reads(None, buf, off, keep=keep))
    r = np.arange(len(keep))
    parts = [alleles.allele_table(amp, buf, off, ob, rr, alleles.group_reads(None, buf, off, keep=keep & m))
             for m in (r < 1100, (r >= 1100) & (r < 1101), r >= 1101)]
    merged = alleles.merge_allele_tables(parts + [None])
    pd.testing.assert_frame_equal(merged.reset_index(drop=True), whole.reset_index(drop=True))
    assert len(alleles.merge_allele_tables([])) == 0
