"""tests/count_model.py (the restatement of CRISPRessoCount's per-read loop) against answers
worked out by hand, and its slice rule against the interpreter's own slicing."""
import numpy as np
import pytest

from tests import count_model as cm

T20 = b"GTTTTAGAGCTAGAAATAGC"


def read_with(n, m, idx, fill=b"c", pat=None):
    """A read of n filler bytes that no pattern of ACGTN can match, the pattern at idx."""
    pat = pat if pat is not None else (T20 * 7)[:m]
    s = bytearray(fill * n)
    s[idx:idx + m] = pat
    assert len(s) == n
    return bytes(s), bytes(pat)


def numbered(n):
    """n bytes that name their own position, so a slice is read off directly."""
    return bytes(48 + (i % 75) for i in range(n))


@pytest.mark.parametrize("idx", range(20, 51))
def test_full_guide(idx):
    """(n, m, L) = (70, 20, 20), idx = 20..50: the 20 bytes before the pattern."""
    s = bytearray(numbered(70).lower().replace(b"g", b"!"))
    s[idx:idx + 20] = T20
    s = bytes(s)
    r = cm.count_model([s], T20, 20)
    assert r["pos"] == [idx] and r["guides"] == [s[idx - 20:idx]] and len(r["guides"][0]) == 20
    assert r["counts"] == [1] and r["first"] == [0] and r["group_of_read"] == [0]
    assert (r["n_reads"], r["n_found"], r["n_counted"]) == (1, 1, 1)


@pytest.mark.parametrize("idx", [0, 1, 19])
def test_pattern_nearer_than_guide_length_gives_the_empty_guide(idx):
    s, t = read_with(70, 20, idx)
    r = cm.count_model([s], t, 20)
    assert r["pos"] == [idx] and r["guides"] == [b""] and r["counts"] == [1]
    assert cm.guide_slice(70, idx, 20) == (50 + idx, 0)


def test_short_read_gives_a_prefix_piece():
    """(15, 5, 20, 3): st = 3 - 20 + 15 = -2 -> 0, the guide is s[0:3]."""
    s, t = read_with(15, 5, 3, pat=b"ACGTA")
    assert cm.guide_slice(15, 3, 20) == (0, 3)
    r = cm.count_model([s], t, 20)
    assert r["pos"] == [3] and r["guides"] == [b"ccc"] == [s[0:3]]


def test_read_longer_than_guide_length_gives_empty():
    """(25, 5, 22, 3): st = 3 - 22 + 25 = 6 >= 3 -> empty."""
    s, t = read_with(25, 5, 3, pat=b"ACGTA")
    assert cm.guide_slice(25, 3, 22) == (6, 0)
    assert cm.count_model([s], t, 22)["guides"] == [b""]


def test_guide_length_zero():
    s, t = read_with(70, 20, 30)
    r = cm.count_model([s, s], t, 0)
    assert r["guides"] == [b""] and r["counts"] == [2] and r["pos"] == [30, 30]
    assert cm.guide_slice(70, 30, 0) == (30, 0)
    assert cm.guide_slice(70, 0, 0) == (0, 0)


def test_first_of_two_patterns_wins():
    s = bytearray(b"c" * 70)
    s[25:30] = b"ACGTA"
    s[50:55] = b"ACGTA"
    r = cm.count_model([bytes(s)], b"ACGTA", 4)
    assert r["pos"] == [25] and r["guides"] == [b"cccc"]
    s[21:25] = b"TTGA"
    assert cm.count_model([bytes(s)], b"ACGTA", 4)["guides"] == [b"TTGA"]


def test_poly_a():
    r = cm.count_model([b"A" * 30], b"AAAA", 20)
    assert r["pos"] == [0] and r["guides"] == [b""]


def test_absent_lowercase_and_cut_off():
    t = b"ACGTA"
    reads = [b"ccccacgtacccc", b"ccccACGT", b"ACG", b"", b"ccACGTAcc"]
    r = cm.count_model(reads, t, 2)
    assert r["pos"] == [-1, -1, -1, -1, 2]
    assert r["group_of_read"] == [-1, -1, -1, -1, 0]
    assert (r["n_reads"], r["n_found"], r["n_counted"]) == (5, 1, 1)
    assert r["guides"] == [b"cc"] and r["first"] == [4]


def test_case_sensitive_keys_in_order_of_first_appearance():
    t = b"GGGG"
    reads = [b"acgtGGGG", b"ACGTGGGG", b"acgtGGGG", b"ANGTGGGG", b"ACGTGGGG", b"acgtGGGG"]
    r = cm.count_model(reads, t, 4)
    assert r["guides"] == [b"acgt", b"ACGT", b"ANGT"]
    assert r["counts"] == [3, 2, 1] and r["first"] == [0, 1, 3]
    assert r["group_of_read"] == [0, 1, 0, 2, 1, 0]


def test_whitelist_rules():
    t = b"GG"
    A8, T8, C8 = b"ACGTACGT", b"TTTTTTTT", b"CCCCCCCC"
    reads = [A8 + t, T8 + t, t, A8 + t, C8 + t, b"xxGG", b"CGTGG"]
    lines = [T8 + b"\n", A8, b"  " + T8 + b"  ", b"\n", b"AAAAAAAA", b"CGT", A8 + b"A"]
    assert cm.whitelist_keys(lines) == [T8, A8, b"", b"AAAAAAAA", b"CGT", A8 + b"A"]
    r = cm.count_model(reads, t, 8, lines)
    # duplicates collapse on the first position, the empty line is the key b"" (the guide of the
    # read that is the pattern alone), zero counts stay, CCCCCCCC and xx are no keys; CGT (a key of
    # another length) is the guide of the 5-byte read: st = 3 - 8 + 5 = 0
    assert r["pos"] == [8, 8, 0, 8, 8, 2, 3]
    assert r["guides"] == [T8, A8, b"", b"AAAAAAAA", b"CGT", A8 + b"A"]
    assert r["counts"] == [1, 2, 1, 0, 1, 0]
    assert r["first"] == [-1] * 6
    assert r["group_of_read"] == [1, 0, 2, 1, -1, -1, 4]
    assert (r["n_reads"], r["n_found"], r["n_counted"]) == (7, 7, 5)


def test_slice_rule_is_pythons():
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(20000):
        n = int(rng.integers(0, 90))
        idx = int(rng.integers(0, n + 1))
        L = int(rng.integers(0, 70))
        s = numbered(n)
        st, ln = cm.guide_slice(n, idx, L)
        assert s[st:st + ln] == s[idx - L:idx], (n, idx, L)


def test_fast_model_equals_model():
    rng = np.random.Generator(np.random.PCG64(4))
    t = b"ACG"
    reads = [bytes(rng.choice(np.frombuffer(b"ACGa", np.uint8), int(rng.integers(0, 40)))) for _ in range(3000)]
    for L in (0, 1, 5, 20):
        for wl in (None, [b"", b"A", b"ACGTA", b"TTACG", b"A"]):
            assert cm.fast_model(reads, t, L, wl) == cm.count_model(reads, t, L, wl)
    assert cm.count_model(reads, t, 5)["n_found"] > 300      # the input is not empty of matches


@pytest.mark.parametrize("m, L", [(5, 20), (33, 19)])
def test_fast_model_equals_model_on_the_gpu_tests_edges(m, L):
    from tests import count_cases as cc

    reads, T, sizes = cc.edge_batch(m, L)
    assert cm.fast_model(reads, T, L) == cm.count_model(reads, T, L)
