"""Known answers of the restatement of Trimmomatic's quality and crop steps
(tests/trim_steps_model.py), which the GPU tests of csrc/trim_steps.hip compare against: hand-worked
records, and per-step counts on the first 1000 records of the reference's test1 files (which also
show that every scanning step acts on dozens of those reads)."""
import functools
import os

import pytest

from tests import trim_steps_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FASTA = os.path.join(GOLDEN, "NexteraPE-PE.fa")
CHAIN_A = "LEADING:3 TRAILING:3 SLIDINGWINDOW:4:15 MINLEN:36"
CHAIN_B = "TRAILING:20 LEADING:20 SLIDINGWINDOW:5:25.5 AVGQUAL:33 MINLEN:50"


def run(steps, quals, seq=None):
    seq = b"A" * len(quals) if seq is None else seq
    return m.run_read(steps.split(), seq, bytes(q + 33 for q in quals))


@pytest.mark.parametrize("steps,quals,expected", [
    ("TRAILING:20", [40], None),
    ("TRAILING:20", [40, 2], None),
    ("TRAILING:20", [2, 40], (0, 2)),
    ("LEADING:20", [], None),
    ("AVGQUAL:20", [], (0, 0)),
    ("SLIDINGWINDOW:4:15", [40, 40, 40, 40, 2, 2, 2, 2, 2, 2], (0, 4)),
    ("SLIDINGWINDOW:5:25.5", [25, 25, 25, 26, 26], None),
    ("SLIDINGWINDOW:5:25.5", [25, 25, 26, 26, 26], (0, 5)),
    ("SLIDINGWINDOW:2:10", [5, 30, 0, 0, 40, 40], (0, 2)),
    ("HEADCROP:2 LEADING:20 CROP:3", [40, 40, 3, 3, 30, 30, 30, 30], (4, 3)),
    ("MINLEN:9 CROP:2", [30] * 8, None),
    ("HEADCROP:8", [30] * 8, None),
    ("CROP:8", [30] * 8, (0, 8)),
    ("CROP:0", [30] * 4, (0, 0)),
])
def test_known_answers(steps, quals, expected):
    assert run(steps, quals) == expected


def test_upper_case_n_counts_as_quality_zero():
    # every window that holds the N totals 120 < 140: the first is window 3, so 3 + 4 - 1 = 6
    # bases stay, and base 5 is at Q40, so the walk back stops at once
    assert run("SLIDINGWINDOW:4:35", [40] * 12, b"AAAAAANAAAAA") == (0, 6)
    assert run("SLIDINGWINDOW:4:35", [40] * 12, b"AAAAAAnAAAAA") == (0, 12)
    assert run("LEADING:30", [40] * 4, b"NNAn") == (2, 2)
    assert run("TRAILING:30", [40] * 4, b"AnNN") == (0, 2)
    assert run("AVGQUAL:21", [40] * 4, b"NNAA") is None
    assert run("AVGQUAL:20", [40] * 4, b"NNAA") == (0, 4)


def test_a_window_total_equal_to_the_requirement_passes():
    assert run("SLIDINGWINDOW:4:15", [15] * 9) == (0, 9)
    assert run("SLIDINGWINDOW:4:15", [15] * 8 + [14]) == (0, 8)


def test_the_walk_back_stops_at_one_base():
    assert run("SLIDINGWINDOW:4:15", [93, 14, 14, 14, 14, 14]) == (0, 1)
    assert run("SLIDINGWINDOW:4:15", [2, 93, 14, 14, 14, 14]) == (0, 2)


@functools.lru_cache(maxsize=None)
def golden(mate):
    return m.read_fastq(os.path.join(GOLDEN, f"test1_L001_R{mate}_001.fastq.gz"))[:1000]


@pytest.mark.parametrize("chain,mate,changed,dropped,moved", [
    (CHAIN_A, 1, [0, 0, 226, 0], [0, 0, 0, 0], 0),
    (CHAIN_A, 2, [0, 0, 205, 0], [0, 0, 0, 56], 0),
    (CHAIN_B, 1, [193, 34, 268, 0, 0], [0, 0, 3, 14, 11], 29),
    (CHAIN_B, 2, [163, 139, 147, 0, 0], [0, 0, 143, 64, 2], 21),
])
def test_golden_counts_per_step(chain, mate, changed, dropped, moved):
    steps = chain.split()
    counts = ([0] * len(steps), [0] * len(steps))
    recs = [m.run_read(steps, s, q, counts=counts) for _, s, q in golden(mate)]
    assert len(recs) == 1000
    assert counts[0] == changed and counts[1] == dropped
    assert sum(r is not None and r[0] > 0 for r in recs) == moved


def test_golden_pairs_clip_then_chain():
    pairs = [(a[1], a[2], b[1], b[2]) for a, b in zip(golden(1), golden(2))]
    o1, o2 = m.run_pairs("ILLUMINACLIP:" + FASTA + ":0:90:10:0:true " + CHAIN_A, pairs)
    both = sum(x is not None and y is not None for x, y in zip(o1, o2))
    fwd = sum(x is not None and y is None for x, y in zip(o1, o2))
    rev = sum(x is None and y is not None for x, y in zip(o1, o2))
    assert (both, fwd, rev, 1000 - both - fwd - rev) == (845, 21, 51, 83)
