#!/usr/bin/env python3
"""Golden vectors for the allele table around a cut site, from the REFERENCE's own code.

What runs: ``compute_ref_positions`` (CRISPResso/CRISPRessoCORE.py:2055-2067),
``get_row_around_cut`` and ``get_dataframe_around_cut`` (CORE:801-836), taken out of the
reference's file by name with ``ast`` and executed unchanged (the module itself does not import
without Bio), on the hand-built ``df_alleles`` of tests/around_cut_cases.py: every batch at
every (cut point, offset) of ``combos()``.  Only the inputs and what the reference returned (or
the exception it raised) are written: tests/golden/around_cut/cases.json.
Run:  python tests/golden/make_around_cut_golden.py   (needs /root/reference; CPU only)
"""
from __future__ import annotations

import ast
import json
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/CRISPResso/CRISPRessoCORE.py"
NAMES = ("compute_ref_positions", "get_row_around_cut", "get_dataframe_around_cut")
sys.path.insert(0, ROOT)

from tests import around_cut_cases as cc  # noqa: E402


def reference_functions() -> dict:
    with open(REF) as f:
        tree = ast.parse(f.read())
    found = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name in NAMES:
            assert node.name not in found, node.name
            found[node.name] = node
    assert set(found) == set(NAMES), sorted(found)
    ns = {"np": np, "pd": pd}
    mod = ast.Module(body=[found[k] for k in NAMES], type_ignores=[])
    exec(compile(mod, REF, "exec"), ns)
    return ns


def main():
    if not os.path.exists(REF):
        sys.exit("needs /root/reference")
    ns = reference_functions()
    cases = []
    for b, cut, offset in cc.combos():
        cols = b.alleles()
        df = pd.DataFrame(cols)
        df["ref_positions"] = df["Reference_Sequence"].apply(ns["compute_ref_positions"]).apply(list)
        try:
            out = ns["get_dataframe_around_cut"](df, cut, offset).reset_index()
            expect = {"Aligned_Sequence": out["Aligned_Sequence"].tolist(),
                      "Reference_Sequence": out["Reference_Sequence"].tolist(),
                      "Unedited": [bool(x) for x in out["Unedited"]],
                      "%Reads": [float(x) for x in out["%Reads"]],
                      "#Reads": [int(x) for x in out["#Reads"]]}
        except ValueError:
            expect = {"error": "ValueError"}
        cases.append({"name": cc.case_id(b, cut, offset), "cut_point": cut, "offset": offset, "alleles": cols,
                      "expect": expect})
    os.makedirs(os.path.join(HERE, "around_cut"), exist_ok=True)
    with open(os.path.join(HERE, "around_cut", "cases.json"), "w") as f:
        json.dump(cases, f, indent=0)
    err = sum("error" in c["expect"] for c in cases)
    print(f"around_cut: {len(cases)} cases, {err} of them the exception")


if __name__ == "__main__":
    main()
