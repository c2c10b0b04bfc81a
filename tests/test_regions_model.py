"""The two restatements of the reference's CIGAR walk and slice (tests/regions_model.py) agree on
every case of tests/regions_cases.py, hold the hand-computed cases of the reference's quirk, and
hold a golden recorded from the reference's own functions (tests/golden/make_wgs_golden.py)."""
import gzip
import json
import os

import pytest

from tests import regions_cases as rc
from tests import regions_model as rm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgs_positions.json.gz")
CASES = {
    "cigar_edges": rc.cigar_edges, "slice_edges": rc.slice_edges, "record_filter": rc.record_filter,
    "many_regions_one_record": rc.many_regions_one_record, "many_records_one_region": lambda: rc.many_records_one_region(300),
    "random": lambda: rc.random_case(200, 40), "table_past_lds": lambda: rc.table_past_lds(600),
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("eqx", [False, True])
def test_models_agree(name, eqx):
    refs, records, regions = CASES[name]()
    if name == "slice_edges":
        records = [r for r in records if r["name"] != b"long"] + [rc.rec("long", 1, 1, "700M")]
        regions = [g for g in regions if g[0] == 0] + [(1, 1, 700), (1, 2, 699), (1, 700, 1), (1, 1, 701)]
    a = rm.extract(records, regions, eqx, rm.walk_ops)
    b = rm.extract(records, regions, eqx, rm.walk_list)
    assert not rc.mismatches(a, b)
    assert sum(map(len, a["hits"])) > 0
    for r in records:          # every (bpstart, bpend) near the record, hit or not, st / en one by one
        for s in range(r["pos"] - 2, r["pos"] + 12):
            for e in (r["pos"], r["pos"] + 3, s):
                assert rm.walk_ops(r["pos"], r["cigar"], s, e, eqx) == rm.walk_list(r["pos"], r["cigar"], s, e, eqx)


def test_hand_computed_cases():
    N = None
    assert rm.positions(100, "5=3X2M") == [100, 101]
    assert rm.positions(100, "15=") == []
    assert rm.positions(100, "5=3X2M", eqx=True) == list(range(100, 110))
    want = [N, N, N, 100, 101, 102, 103, N, N, 104, 105, 106, 107, 109, 110, 111]
    assert rm.positions(100, rc.CIGAR_A) == want
    for walk in (rm.walk_ops, rm.walk_list):
        assert walk(100, rc.CIGAR_A, 101, 109) == (True, 4, 13)
        assert walk(100, rc.CIGAR_A, 101, 108)[0] is False          # 108 lies in the D gap
        assert walk(100, "5=3X2M", 100, 101) == (True, 0, 1)
        assert walk(100, "5=3X2M", 100, 109, True) == (True, 0, 9)
        assert walk(100, "15=", 100, 100)[0] is False
        assert walk(100, "*", 100, 100)[0] is False


def test_slice_rule_and_names():
    r = rc.rec("n", 0, 60, "20M", seq="ACGTACGTAC", qual=list(range(10)))
    got = rm.extract([r, r], [(0, 64, 77), (0, 75, 79), (0, 66, 66), (0, 66, 62)])["hits"]
    assert [h[3] for h in got[0]] == [b"ACGTAC"] * 2 and got[0][0][1:3] == (4, 17)       # en cut to l_seq
    assert got[0][0][4] == b"%&'()*" and [h[5] for h in got[0]] == [b"n_1", b"n_2"]
    assert [h[3] for h in got[1]] == [b"", b""] and [h[3] for h in got[2]] == [b"", b""]    # st past l_seq; en == st
    assert [h[3] for h in got[3]] == [b"", b""] and len(got[3]) == 2                        # en < st still counts
    assert rm.fastq(got[2]) == b"@n_1\n\n+\n\n@n_2\n\n+\n\n"


def test_golden_from_the_reference():
    rows = json.loads(gzip.open(GOLDEN).read())["rows"]
    assert len(rows) >= 150 and sum(1 for r in rows if r[4]) >= 50 and sum(1 for r in rows if not r[4]) >= 50
    assert {"5=3X2M", "15=", "3S4M2I4M1D3M2H", "4M2P4M", "*"} <= {r[1] for r in rows}
    for pos, cigar, s, e, hit, st, en in rows:
        for walk in (rm.walk_ops, rm.walk_list):
            got = walk(pos, cigar, s, e)
            assert got[0] == hit, (pos, cigar, s, e)
            if hit:
                assert got[1:] == (st, en), (pos, cigar, s, e)
