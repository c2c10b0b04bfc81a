"""tests/demux_model.py (the demultiplexing rule of include/crispr_demux.h in plain Python) held
to hand-worked cases and to the needle oracle: the rule itself is pinned where no GPU is needed.
tests/test_gpu_demux.py holds the kernels to this model."""
from tests import demux_cases as dc
from tests import demux_model as dm

# k = 8.  A0 and A2 share the window ACGGTTCA (A0's last, A2's first): 15 windows, 14 distinct,
# one of them AMBIGUOUS.
A0 = b"ACGTACGGTTCA"       # ACGTACGG CGTACGGT GTACGGTT TACGGTTC ACGGTTCA*
A1 = b"TTGACCAGTAGC"       # TTGACCAG TGACCAGT GACCAGTA ACCAGTAG CCAGTAGC
A2 = b"ACGGTTCAGGAT"       # ACGGTTCA* CGGTTCAG GGTTCAGG GTTCAGGA TTCAGGAT
TOY = [A0, A1, A2]


def one(read, **kw):
    out = dm.demultiplex(TOY, [read], **dict(dict(k=8, min_hits=2), **kw))
    return out["which"][0], out["strand"][0], out["votes"][0], out["rival"][0]


def test_toy_index():
    index = dm.build_index(TOY, 8)
    assert len(index) == 14
    assert index[b"ACGGTTCA"] == dm.AMBIGUOUS and [k for k, g in index.items() if g == dm.AMBIGUOUS] == [b"ACGGTTCA"]
    assert index[b"ACGTACGG"] == 0 and index[b"CCAGTAGC"] == 1 and index[b"TTCAGGAT"] == 2
    # the amplicon set alone: any order gives the same windows, renumbered
    back = dm.build_index(TOY[::-1], 8)
    assert {k: (g if g < 0 else 2 - g) for k, g in back.items()} == index
    # a repeat inside one amplicon stays that amplicon
    assert dm.build_index([b"ACGTACGTACGTACGT"], 8) == {b"ACGTACGT": 0, b"CGTACGTA": 0, b"GTACGTAC": 0, b"TACGTACG": 0}


def test_toy_votes_by_hand():
    # the whole of A0: four of its five windows vote, the shared one does not
    assert dm.votes_of(dm.build_index(TOY, 8), A0, 8) == {(0, 0): 4}
    assert one(A0) == (0, 0, 4, 0)
    # the reverse complement of A1: all five windows on strand 1
    assert dm.revcomp(A1) == b"GCTACTGGTCAA"
    assert one(dm.revcomp(A1)) == (1, 1, 5, 0)
    assert one(dm.revcomp(A1), both_strands=False) == (dm.NO_HIT, 0, 0, 0)
    # ACGGTTCA (ambiguous) CGGTTCAG GGTTCAGG: two votes for A2
    assert one(b"ACGGTTCAGG") == (2, 0, 2, 0)
    assert one(b"acggTTCAgg") == (2, 0, 2, 0)
    # the ambiguous window alone never votes
    assert one(b"ACGGTTCA") == (dm.NO_HIT, 0, 0, 0)
    assert one(b"ACGGTTCA", min_hits=1) == (dm.NO_HIT, 0, 0, 0)


def test_tie_no_hit_short_and_empty():
    # A0[:9] + A1[3:]: ACGTACGG CGTACGGT for A0, ACCAGTAG CCAGTAGC for A1, nothing between
    chimera = A0[:9] + A1[3:]
    assert chimera == b"ACGTACGGTACCAGTAGC"
    assert one(chimera) == (dm.TIE, 0, 2, 2)
    assert one(chimera, min_hits=3) == (dm.NO_HIT, 0, 2, 2)
    # three windows against two: assigned, the rival reported
    assert one(A0[:10] + A1[3:]) == (0, 0, 3, 2)
    assert one(b"ACGTACG") == (dm.NO_HIT, 0, 0, 0)          # k - 1 bases
    assert one(b"") == (dm.NO_HIT, 0, 0, 0)
    assert one(b"ACGTACGG") == (dm.NO_HIT, 0, 1, 0)         # one window, min_hits 2
    assert one(b"ACGTACGG", min_hits=1) == (0, 0, 1, 0)
    assert one(b"GGGGGGGGGGGGGGGG") == (dm.NO_HIT, 0, 0, 0)


def test_break_bytes():
    # position 8 of A0 broken: only the first window is left
    for b in (b"N", b"-", b"n", b"R", b"\x00"):
        read = A0[:8] + b + A0[9:]
        assert one(read) == (dm.NO_HIT, 0, 1, 0), b
        assert one(read, min_hits=1) == (0, 0, 1, 0), b
    # a break in an amplicon: its windows there are no keys
    index = dm.build_index([b"ACGTACGGNTCAGGATC"], 8)
    assert sorted(index) == [b"ACGTACGG", b"TCAGGATC"]
    assert dm.window_key(b"ACGTNCGT") is None and dm.window_key(b"acgtacgt") == b"ACGTACGT"
    # the reverse complement keeps every other byte
    assert dm.revcomp(b"AaCcGgTtN-x") == b"x-NaAcCgGtT"


def test_palindrome_is_a_tie():
    amps, reads = dc.palindrome()
    out = dm.demultiplex(amps, reads)
    pal = amps[0]
    assert dm.revcomp(pal) == pal
    n = len(pal) - 16 + 1
    assert (out["which"][0], out["votes"][0], out["rival"][0]) == (dm.TIE, n, n)      # every window on both strands
    assert out["which"][1] == dm.TIE and out["votes"][1] == out["rival"][1] == 90 - 15
    assert out["which"][2:4] == [1, 1] and out["strand"][2:4] == [0, 1]
    assert out["which"][4] == dm.TIE and out["which"][5] == dm.TIE


def test_gathered_groups():
    reads = [dm.revcomp(A1), A0, b"ACGGTTCA", b"ACGGTTCAGG", dm.revcomp(A0), A1[:10].lower() + b"N"]
    out = dm.demultiplex(TOY, reads, k=8)
    assert out["which"] == [1, 0, dm.NO_HIT, 2, 0, 1] and out["strand"] == [1, 0, 0, 0, 1, 0]
    assert out["counts"] == [2, 2, 1] and out["group_offsets"] == [0, 2, 4, 5] and out["order"] == [1, 4, 0, 5, 3]
    assert out["groups"] == [[A0, A0], [A1, A1[:10].lower() + b"N"], [b"ACGGTTCAGG"]]
    assert (out["n_windows"], out["n_ambiguous"]) == (14, 1)


def test_ambiguity_constructions():
    cases = dc.ambiguity()
    amps, reads = cases["identical"]
    out = dm.demultiplex(amps, reads)
    assert out["which"][:4] == [dm.NO_HIT] * 4 and out["votes"][:4] == [0] * 4          # every window of a is ambiguous
    assert out["which"][4:] == [2, 2] and out["n_ambiguous"] == 250 - 15
    amps, reads = cases["reverse_complement"]
    out = dm.demultiplex(amps, reads)
    assert out["which"][:4] == [dm.TIE] * 4 and out["votes"][0] == out["rival"][0] == 235
    assert dm.demultiplex(amps, reads, both_strands=False)["which"][:4] == [0, 1, 0, 1]
    amps, reads = cases["three_bases"]
    out = dm.demultiplex(amps, reads)
    # only the windows over a substituted base tell the two apart: 16 at each of bases 40, 120, 200
    assert out["which"][0] == 0 and out["votes"][0] == 48 and out["rival"][0] == 0
    assert out["which"][2] == 1 and out["votes"][2] == 48
    assert out["which"][8] == 0 and out["votes"][8] == 11                                 # a[30:60]: the windows from 30..40 hold base 40
    assert out["which"][10] == dm.NO_HIT and out["votes"][10] == 0                        # a[60:110]: shared, ambiguous
    amps, reads = cases["bridge"]
    out = dm.demultiplex(amps, reads)
    assert out["which"][0] == 0 and out["votes"][0] == 125 - 15 + 15                       # b's own half, and over the junction
    assert out["which"][4] == 2 and out["votes"][4] == 15                                  # the bridge: only its junction
    assert out["which"][8] == dm.NO_HIT                                                    # b[125:]: shared with the bridge


def test_oracle_acceptance():
    """For every assigned read (which, strand) is among the pairs oracle_py.score ranks highest
    (no tolerance); at most 2 % of the reads are left unassigned."""
    amps, reads = dc.acceptance()
    out = dm.demultiplex(amps, reads, k=16, min_hits=2)
    unassigned = sum(1 for g in out["which"] if g < 0)
    bad = dc.oracle_disagreements(out["which"], out["strand"])
    print(f"disagreements with the oracle: {len(bad)}; unassigned {unassigned} of {len(reads)}")
    assert bad == []
    assert unassigned <= 0.02 * len(reads)


def test_unrelated_amplicons_all_assigned():
    amps, reads, source = dc.unrelated()
    assert len(reads) == 3600
    out = dm.demultiplex(amps, reads)
    print(f"smallest vote: {min(out['votes'])}; largest rival: {max(out['rival'])}")
    assert out["which"] == source
    assert out["strand"] == [i % 2 for i in range(len(reads))]
    assert min(out["votes"]) >= 86
