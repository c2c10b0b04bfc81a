"""The clip kernel (crispresso_amd/csrc/trim_clip.hip) against oracle/trimmomatic_oracle.py on the
adapter tables of tests/clip_table_cases.py: no prefix pair, no adapter, four prefix pairs, prefixes of
12 to 128 bases and of unequal length, adapters of 24 to 128 bases with all three roles, 16 of them,
qualities up to phred 93.  Every read's keep length must equal the oracle's, through nwt_trim_batch
(paired, single-end, batches larger than the grid, 4,096-base reads behind a 128-base prefix),
nwt_trim_program and the four output files; the tables past the limits are refused and leave the
next call unharmed.  tests/test_clip_table_cases.py holds, on the CPU, that the oracle's answers on
these pairs depend on each of the rules the shapes exercise."""
import ctypes
import gzip

import numpy as np
import pytest

from crispresso_amd import _lib
from crispresso_amd.trim import (TrimError, TrimOptions, TrimProgram, run_trimmomatic_pe, trim_pairs,
                                 trim_program_pairs)
from tests import clip_table_cases as cc
from tests.clip_table_cases import tmo
from tests.test_trim import assert_same

pytestmark = pytest.mark.gpu

SE_SPECS = [cc.DEFAULT, ":1:30:7:1:false"]


@pytest.fixture(scope="module")
def fasta_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("clip_tables")


def options(table, spec, minlen, directory):
    steps = ["ILLUMINACLIP:" + cc.write_fasta(table, directory) + spec] + ([f"MINLEN:{minlen}"] if minlen else [])
    return TrimOptions.from_steps(steps)


def gpu_keeps(plist, o, single_end=False):
    s1, q1, s2, q2 = ([p[i] for p in plist] for i in range(4))
    return trim_pairs(s1, q1, None if single_end else s2, None if single_end else q2, o)


def check(table, spec, directory, what, minlens=(0, 40)):
    k1, k2, _ = cc.oracle(table, spec, directory, what)
    plist = cc.case_list(table, what)
    for minlen in minlens:
        res = gpu_keeps(plist, options(table, spec, minlen, directory))
        assert_same(res, cc.minlen_applied(k1, minlen), cc.minlen_applied(k2, minlen),
                    f"{table} {what} {spec} MINLEN {minlen}")


@pytest.mark.parametrize("spec", cc.SPECS)
@pytest.mark.parametrize("table", cc.TABLES)
def test_gpu_clip_tables_match_oracle(table, spec, fasta_dir):
    o = options(table, spec, 0, fasta_dir)
    n_pp, n_ad = len(cc.prefix_pairs(table)), len({a for a in cc.adapters(table)})
    assert (len(o.prefix_pairs), len(o.adapters)) == (n_pp, n_ad)
    check(table, spec, fasta_dir, "pairs")
    check(table, spec, fasta_dir, "named")


@pytest.mark.parametrize("spec", cc.SPECS)
def test_gpu_clip_full_table_long_reads(spec, fasta_dir):
    """4,096-base mates behind the 128-base prefix: the largest LDS the kernel asks for, on the
    one-wave-per-block launch."""
    k1, k2, _ = cc.oracle("full", spec, fasta_dir, "long")
    assert k1[0] == cc.LONG_FRAGMENT and k2[0] == (cc.LONG_FRAGMENT if spec == cc.DEFAULT else 0)
    assert sorted((int(k1[1]), int(k2[1]))) == [4000, 4096]
    check("full", spec, fasta_dir, "long")
    # short pairs in the same launch
    e1, e2, _ = cc.oracle("full", spec, fasta_dir)
    plist = cc.long_cases() + cc.pairs("full")[:24]
    res = gpu_keeps(plist, options("full", spec, 0, fasta_dir))
    assert_same(res, np.concatenate([k1, e1[:24]]), np.concatenate([k2, e2[:24]]), f"long + short {spec}")


@pytest.mark.parametrize("spec", SE_SPECS)
@pytest.mark.parametrize("table", ["full", "simple_only"])
def test_gpu_clip_tables_single_end(table, spec, fasta_dir):
    """Single-end: the prefix pairs are staged and skipped, the simple scan reads behind the last one."""
    k1, _, counts = cc.oracle(table, spec, fasta_dir, single_end=True)
    assert counts["palindrome"] == 0 and counts["simple1"] >= 30
    for minlen in (0, 40):
        res = gpu_keeps(cc.pairs(table), options(table, spec, minlen, fasta_dir), single_end=True)
        assert res.keep2 is None
        assert_same(res, cc.minlen_applied(k1, minlen), None, f"{table} single-end {spec} MINLEN {minlen}")


def test_gpu_clip_full_table_batch_larger_than_the_grid(fasta_dir):
    """A wavefront takes a second and a third pair through four prefix rounds over the LDS bytes its
    previous pair left behind."""
    try:
        import torch
        cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        cus = 256
    spec = ":1:30:7:1:false"
    e1, e2, _ = cc.oracle("full", spec, fasta_dir)
    pool = cc.pairs("full")
    res = gpu_keeps(pool[:257], options("full", spec, 0, fasta_dir))
    assert_same(res, e1[:257], e2[:257], "batch of 257")
    n = 2 * (4 * 16 * cus) + 5
    assert n > 4 * 16 * cus
    idx = np.random.Generator(np.random.PCG64(17)).integers(0, len(pool), n)
    plist = [pool[j] for j in idx]
    for minlen in (0, 40):
        res = gpu_keeps(plist, options("full", spec, minlen, fasta_dir))
        assert len(res.keep1) == n and len(res.keep2) == n
        assert_same(res, cc.minlen_applied(e1[idx], minlen), cc.minlen_applied(e2[idx], minlen),
                    f"batch of {n} MINLEN {minlen}")


@pytest.mark.parametrize("table", ["full", "unequal_long_prefix"])
def test_gpu_clip_tables_uncut_prefixes(table, fasta_dir):
    """Prefixes of unequal length given as the file has them: the library cuts them itself."""
    spec = ":2:30:10"
    o = options(table, spec, 0, fasta_dir)
    uncut = cc.prefix_pairs(table)
    cut = [min(len(p1), len(p2)) for p1, p2 in uncut]
    assert o.prefix_pairs == [(p1[len(p1) - m:], p2[len(p2) - m:]) for (p1, p2), m in zip(uncut, cut)]
    assert any(len(p1) != len(p2) for p1, p2 in uncut)
    o.prefix_pairs = uncut
    k1, k2, _ = cc.oracle(table, spec, fasta_dir)
    assert_same(gpu_keeps(cc.pairs(table), o), k1, k2, f"{table} uncut prefixes")


@pytest.mark.parametrize("spec", cc.SPECS)
@pytest.mark.parametrize("table", ["full", "unequal_long_prefix"])
def test_gpu_clip_tables_through_the_program_entry(table, spec, fasta_dir):
    """nwt_trim_program with ILLUMINACLIP and MINLEN:40 alone: the same clip through program_run."""
    plist = cc.pairs(table) + cc.case_list(table, "named")
    res = gpu_keeps(plist, options(table, spec, 40, fasta_dir))
    prog = TrimProgram.from_steps(["ILLUMINACLIP:" + cc.write_fasta(table, fasta_dir) + spec, "MINLEN:40"])
    s1, q1, s2, q2 = ([p[i] for p in plist] for i in range(4))
    w = trim_program_pairs(s1, q1, s2, q2, prog)
    assert not w.start1.any() and not w.start2.any()
    assert np.array_equal(np.maximum(w.keep1, 0), res.keep1) and np.array_equal(np.maximum(w.keep2, 0), res.keep2)
    assert np.array_equal(w.keep1 == -1, res.keep1 == 0) and np.array_equal(w.keep2 == -1, res.keep2 == 0)
    k1 = np.concatenate([cc.oracle(table, spec, fasta_dir, what)[0] for what in ("pairs", "named")])
    k2 = np.concatenate([cc.oracle(table, spec, fasta_dir, what)[1] for what in ("pairs", "named")])
    assert_same(res, cc.minlen_applied(k1, 40), cc.minlen_applied(k2, 40), f"{table} {spec}")


@pytest.mark.parametrize("table", ["full", "unequal_long_prefix"])
def test_gpu_clip_tables_files_match_oracle(table, fasta_dir, tmp_path):
    plist = cc.pairs(table)[:120]
    for name, si, qi in (("r1.fastq", 0, 1), ("r2.fastq", 2, 3)):
        with open(tmp_path / name, "wb") as f:
            for i, p in enumerate(plist):
                f.write(b"@read%d/%s\n%s\n+\n%s\n" % (i, name[1].encode(), p[si], p[qi]))
    steps = ["ILLUMINACLIP:" + cc.write_fasta(table, fasta_dir) + ":1:30:7:1:false", "MINLEN:40"]
    names = ("fp.fq.gz", "fu.fq", "rp.fq.gz", "ru.fq")
    gpu = [str(tmp_path / ("gpu_" + n)) for n in names]
    cpu = [str(tmp_path / ("cpu_" + n)) for n in names]
    st_gpu = run_trimmomatic_pe(str(tmp_path / "r1.fastq"), str(tmp_path / "r2.fastq"), gpu, " ".join(steps))
    st_cpu = tmo.run_pe(str(tmp_path / "r1.fastq"), str(tmp_path / "r2.fastq"), cpu, steps)
    assert st_gpu == st_cpu
    assert min(st_cpu["both"], st_cpu["fwd_only"], st_cpu["dropped"]) > 0
    for a, b in zip(gpu, cpu):
        op = gzip.open if a.endswith(".gz") else open
        with op(a, "rb") as fa, op(b, "rb") as fb:
            assert fa.read() == fb.read(), a


def _c_entry(adapters, adapter_off, roles, prefixes, prefix_off):
    """nwt_trim_batch on no reads: the tables are built and checked, nothing is launched."""
    ad = np.frombuffer(adapters, np.uint8).copy()
    pre = np.frombuffer(prefixes, np.uint8).copy()
    ad_off, ro, pre_off = (np.ascontiguousarray(x, dtype=np.int32) for x in (adapter_off, roles, prefix_off))
    params = _lib.NwtParams(0, 90, 10, 0, 1, 0)
    lib = _lib.load()
    rc = lib.nwt_trim_batch(0, ctypes.byref(params), _lib.ptr(ad), _lib.ptr(ad_off), _lib.ptr(ro), len(ro),
                            _lib.ptr(pre), _lib.ptr(pre_off), (len(pre_off) - 1) // 2, None, None, None, None, None,
                            None, 0, None, None, None)
    return rc, lib.nwt_last_error().decode()


def test_gpu_clip_table_refusals(fasta_dir):
    rng = np.random.Generator(np.random.PCG64(23))
    r = lambda k: bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), k))  # noqa: E731
    e1, e2, _ = cc.oracle("full", cc.DEFAULT, fasta_dir)
    full = options("full", cc.DEFAULT, 0, fasta_dir)
    assert len(full.adapters) == 16 and len(full.prefix_pairs) == 4
    assert max(len(a) for a, _ in full.adapters) == 128 and len(full.prefix_pairs[-1][0]) == 128

    def the_limits_still_pass():
        assert_same(gpu_keeps(cc.pairs("full")[:60], full), e1[:60], e2[:60], "full after a refusal")

    one = [b"ACGT" * 10], [b"I" * 40], [b"ACGT" * 10], [b"I" * 40]
    refused = [
        (TrimOptions(simple_threshold=10, adapters=[(r(30), 0) for _ in range(17)]), "more than 16 adapters"),
        (TrimOptions(simple_threshold=10, prefix_pairs=[(r(30), r(30)) for _ in range(5)]), "more than 4 prefix pairs"),
        (TrimOptions(simple_threshold=10, adapters=[(r(129), 0)]), "adapters longer than 128"),
        (TrimOptions(simple_threshold=10, prefix_pairs=[(r(129), r(40))]), "prefixes longer than 128"),
        (TrimOptions(simple_threshold=10, adapters=[(r(40), 0), (r(23), 2)]), "shorter than 24"),
    ]
    for o, message in refused:
        with pytest.raises(TrimError, match=message):
            trim_pairs(*one, o)
        the_limits_still_pass()
    # the limits themselves are taken
    ok = TrimOptions(simple_threshold=10, adapters=[(r(128), 0)], prefix_pairs=[(r(128), r(128))])
    assert trim_pairs(*one, ok).keep1[0] == 40

    a, p = r(60), r(60)
    assert _c_entry(a, [0, 30, 60], [0, 2], p, [0, 20, 40])[0] == 0
    for args, message in (((a, [0, 30, 60], [0, 3], p, [0, 20, 40]), "role"),
                          ((a, [0, 30, 60], [-1, 0], p, [0, 20, 40]), "role"),
                          ((a, [1, 31], [0], p, [0, 20, 40]), "adapter offsets must start at 0"),
                          ((a, [0, 40, 10], [0, 0], p, [0, 20, 40]), "adapter offsets not ascending"),
                          ((a, [0, 30, 60], [0, 0], p, [1, 20, 40]), "prefix offsets must start at 0"),
                          ((a, [0, 30, 60], [0, 0], p, [0, 30, 20]), "prefix offsets not ascending"),
                          ((a, [0, 30, 60], [0, 0], p, [0, 20, 40, 30, 50]), "prefix offsets not ascending")):
        rc, err = _c_entry(*args)
        assert rc == -1 and message in err and err.startswith("nwt_trim_batch"), (args[1:3], args[4], rc, err)
        the_limits_still_pass()
