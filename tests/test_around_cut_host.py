"""alleles.around_cut_from_alleles / merge_around_cut_tables against what the reference's
get_dataframe_around_cut returned for the hand-built df_alleles of tests/around_cut_cases.py
(tests/golden/around_cut/cases.json, recorded by tests/golden/make_around_cut_golden.py).  No GPU."""
import json
import os

import numpy as np
import pandas as pd
import pytest

from crispresso_amd import alleles
from tests import around_cut_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "around_cut", "cases.json")) as f:
    CASES = {c["name"]: c for c in json.load(f)}
ORDER = ["#Reads", "Aligned_Sequence", "Reference_Sequence"]


def in_defined_order(frame):
    """The frame (Aligned_Sequence a column) sorted by #Reads descending, then the two windows."""
    return frame.sort_values(by=ORDER, ascending=[False, True, True], kind="stable").reset_index(drop=True)


def assert_around_equal(got, want):
    """Both re-sorted by the defined order: the strings, Unedited and #Reads equal, %Reads to
    rtol 1e-9 (the reference sums a group's %Reads, here it is #Reads / total * 100)."""
    g, w = in_defined_order(got.reset_index()), in_defined_order(want.reset_index())
    assert len(g) == len(w)
    for col in ("Aligned_Sequence", "Reference_Sequence"):
        assert g[col].tolist() == w[col].tolist()
    assert g["Unedited"].astype(bool).tolist() == w["Unedited"].astype(bool).tolist()
    assert g["#Reads"].astype(np.int64).tolist() == w["#Reads"].astype(np.int64).tolist()
    np.testing.assert_allclose(g["%Reads"].to_numpy(float), w["%Reads"].to_numpy(float), rtol=1e-9, atol=0)


def assert_form(got):
    assert got.index.name == "Aligned_Sequence"
    assert list(got.columns) == alleles.AROUND_COLUMNS
    assert got["Unedited"].dtype == bool and got["#Reads"].dtype == np.int64
    flat = got.reset_index()
    pd.testing.assert_frame_equal(flat, in_defined_order(flat))           # the returned order is the defined one


def test_cases_cover_the_list():
    """Every recorded combination is one the case file still generates, and the list holds an
    exception, a clipped stop, a negative start, an empty window and a merged window."""
    assert sorted(CASES) == sorted(cc.case_id(b, c, o) for b, c, o in cc.combos())
    expects = [c["expect"] for c in CASES.values()]
    assert any("error" in e for e in expects)
    assert any("" in e.get("Aligned_Sequence", []) for e in expects)
    plain = CASES["plain-cut30-off20"]
    assert len(plain["expect"]["#Reads"]) < len(plain["alleles"]["#Reads"])
    top = max(range(len(plain["expect"]["#Reads"])), key=lambda i: plain["expect"]["#Reads"][i])
    assert plain["expect"]["Unedited"][top] and plain["expect"]["#Reads"][top] >= 5


@pytest.mark.parametrize("name", sorted(CASES))
def test_around_cut_from_alleles_equals_reference(name):
    case = CASES[name]
    df = pd.DataFrame(case["alleles"])
    if "error" in case["expect"]:
        with pytest.raises(alleles.AlleleError, match="allele"):
            alleles.around_cut_from_alleles(df, case["cut_point"], case["offset"])
        return
    got = alleles.around_cut_from_alleles(df, case["cut_point"], case["offset"])
    assert_form(got)
    want = pd.DataFrame(case["expect"]).set_index("Aligned_Sequence")
    assert_around_equal(got, want)


def test_ref_positions_rule():
    assert alleles.ref_positions("--AC-gRN-T") == [-1, -1, 0, 1, -2, -2, -2, 2, -3, 3]
    for b in cc.batches():
        for rd in b.distinct:
            assert alleles.ref_positions(b.rows(rd)[1]) == cc.positions(b.rows(rd)[1])


@pytest.mark.parametrize("cut,offset", [(30, 20), (0, 20), (59, 1)])
def test_merge_halves_equals_whole(cut, offset):
    b = cc.batches()[0]
    cols = b.alleles()
    df = pd.DataFrame(cols)
    # two halves of the batch: the reads of every allele split between them (an allele with
    # one read falls into one half only)
    halves = []
    for part in (0, 1):
        h = df.copy()
        h["#Reads"] = [(c + 1 - part) // 2 for c in cols["#Reads"]]
        h = h[h["#Reads"] > 0]
        h["%Reads"] = h["#Reads"] / h["#Reads"].sum() * 100.0
        halves.append(alleles.around_cut_from_alleles(h, cut, offset))
    whole = alleles.around_cut_from_alleles(df, cut, offset)
    merged = alleles.merge_around_cut_tables(halves)
    assert_form(merged)
    pd.testing.assert_frame_equal(merged, whole)
    empty = alleles.merge_around_cut_tables([])
    assert len(empty) == 0 and list(empty.columns) == alleles.AROUND_COLUMNS
