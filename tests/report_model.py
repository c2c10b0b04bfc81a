"""A restatement of the per-group report (crispresso_amd/report.py, nws_mask_pre and nws_histograms
of include/crispr_summary.h) in plain numpy and pandas, written from the reference's output code
(CRISPRessoCORE.py:3739-3749, 3805-3963) and from the header: what the kernels count, what a
kept-reads DataFrame looks like to ``quantify.run_summary``, and every file's bytes from the same
integers.  No GPU."""
import io

import numpy as np
import pandas as pd

from crispresso_amd import _lib, quantify
from crispresso_amd.report import GroupReport

VECTOR_FILES = {            # file stem -> the quantifier's vector
    "effect_vector_insertion_NHEJ": "effect_vector_insertion",
    "effect_vector_deletion_NHEJ": "effect_vector_deletion",
    "effect_vector_substitution_NHEJ": "effect_vector_mutation",
}
CODING_FILES = {
    "effect_vector_insertion_noncoding": "effect_vector_insertion_noncoding",
    "effect_vector_deletion_noncoding": "effect_vector_deletion_noncoding",
    "effect_vector_substitution_noncoding": "effect_vector_mutation_noncoding",
}
HDR_FILES = {
    "effect_vector_insertion_mixed_hdr_nhej": "effect_vector_insertion_mixed",
    "effect_vector_deletion_mixed_hdr_nhej": "effect_vector_deletion_mixed",
    "effect_vector_substitution_mixed_hdr_nhej": "effect_vector_mutation_mixed",
    "effect_vector_insertion_HDR": "effect_vector_insertion_hdr",
    "effect_vector_deletion_HDR": "effect_vector_deletion_hdr",
    "effect_vector_substitution_HDR": "effect_vector_mutation_hdr",
}


def mask_pre(pre, keep):
    """nws_mask_pre: a dropped read's byte becomes UNMODIFIED alone."""
    pre, keep = np.asarray(pre, np.uint8), np.asarray(keep, np.uint8)
    return np.where(keep != 0, pre, np.uint8(_lib.NWQ_PRE_UNMODIFIED)).astype(np.uint8)


def histograms(cls, n_mutated, n_inserted, n_deleted, keep, bins):
    """nws_histograms: ((ins, del, mut, indel), n_out_of_range) by np.bincount over the reads with
    keep != 0 and cls >= 0 whose three sizes all lie in [0, bins)."""
    cls, keep = np.asarray(cls, np.int64), np.asarray(keep)
    m, i, d = (np.asarray(x, np.int64) for x in (n_mutated, n_inserted, n_deleted))
    counted = (keep != 0) & (cls >= 0)
    inside = (m >= 0) & (m < bins) & (i >= 0) & (i < bins) & (d >= 0) & (d < bins)
    sel = counted & inside
    out = (np.bincount(i[sel], minlength=bins), np.bincount(d[sel], minlength=bins), np.bincount(m[sel], minlength=bins),
           np.bincount(i[sel] - d[sel] + bins - 1, minlength=2 * bins - 1))
    return tuple(x.astype(np.int64) for x in out), int((counted & ~inside).sum())


def kept_frame(cls, n_mutated, n_inserted, n_deleted, unmodified_in=None):
    """The quantified DataFrame of kept reads run_summary takes: one row per read, the class
    columns from cls (0 .. 3) and the input UNMODIFIED flag."""
    cls = np.asarray(cls)
    um = np.zeros(len(cls), bool) if unmodified_in is None else np.asarray(unmodified_in, bool)
    return pd.DataFrame({
        "align_seq": ["A"] * len(cls), "ref_seq": ["A"] * len(cls), "UNMODIFIED": um | (cls == 0), "NHEJ": cls == 1,
        "HDR": cls == 2, "MIXED": cls == 3, "n_mutated": np.asarray(n_mutated, np.int64),
        "n_inserted": np.asarray(n_inserted, np.int64), "n_deleted": np.asarray(n_deleted, np.int64)})


def slots_of(cls, n_mutated, n_inserted, n_deleted, n_reads=None):
    """nws_summary's 16 slots of kept reads alone (no input UNMODIFIED flag)."""
    cls = np.asarray(cls)
    s = [len(cls) if n_reads is None else n_reads, len(cls), int((cls == 0).sum()), int((cls == 1).sum()),
         int((cls == 2).sum()), int((cls == 3).sum())]
    for k in (1, 2, 3):
        for col in (n_inserted, n_deleted, n_mutated):
            s.append(int(((cls == k) & (np.asarray(col) > 0)).sum()))
    return np.array(s + [int((cls < 0).sum())], np.int64)


def synthetic_totals(L, seed, coding=False, hdr=False):
    """Totals in unpack_totals' shape: small random counts with zeros among them, so that the
    average-size vectors meet 0 / 0 and x / 0."""
    rng = np.random.Generator(np.random.PCG64(seed))
    vec = {}
    for name in quantify.VECTOR_NAMES:
        used = ("hdr" not in name and "mixed" not in name or hdr) and ("noncoding" not in name or coding)
        vec[name] = rng.integers(0, 4, L).astype(np.int64) * (rng.random(L) < 0.6) if used else np.zeros(L, np.int64)
    vec["avg_vector_ins_all"] = rng.integers(0, 30, L).astype(np.int64)
    vec["avg_vector_del_all"] = rng.integers(0, 30, L).astype(np.int64)
    ctr = {k: int(rng.integers(0, 9)) if coding else 0 for k in quantify.COUNTER_NAMES}
    return {"vectors": vec, "counters": ctr, "hist_inframe": {}, "hist_frameshift": {}}


def report_of(name, amplicon, cut_points, cls, n_mutated, n_inserted, n_deleted, totals, n_reads=None, coding=False,
              hdr=False, bins=None):
    """A GroupReport from kept reads: the slots and histograms the kernels would give."""
    bins = len(amplicon) + 1 if bins is None else bins
    (hi, hd, hm, hx), bad = histograms(cls, n_mutated, n_inserted, n_deleted, np.ones(len(cls), np.uint8), bins)
    assert bad == 0
    return GroupReport(name, amplicon, list(cut_points), len(cls) if n_reads is None else n_reads,
                       slots_of(cls, n_mutated, n_inserted, n_deleted, n_reads), totals, hi, hd, hm, hx,
                       has_coding_seq=coding, has_expected_hdr=hdr)


def vector_bytes(vector) -> bytes:
    """save_vector_to_file (CORE:3739-3749) into memory."""
    buf = io.BytesIO()
    np.savetxt(buf, np.vstack([np.arange(len(vector)) + 1, vector]).T, fmt=["%d", "%.18e"], delimiter="\t", newline="\n",
               header="amplicon position\teffect", footer="", comments="# ")
    return buf.getvalue()


def expected_files(rep: GroupReport, frames) -> dict:
    """{file name: bytes} of the whole folder, from the report's integers and the four tables
    (``frames``: run_summary's output on the kept reads)."""
    s = [int(x) for x in rep.slots]
    v = {k: np.asarray(a, np.float64) for k, a in rep.totals["vectors"].items()}
    c = rep.totals["counters"]
    n_total = s[1]
    files = {}
    files["Quantification_of_editing_frequency.txt"] = (
        "Quantification of editing frequency:\n\t- "
        f"Unmodified:{s[2]} reads\n"
        f"\t- NHEJ:{s[3]} reads ({s[6]} reads with insertions, {s[7]} reads with deletions, {s[8]} reads with substitutions)\n"
        f"\t- HDR:{s[4]} reads ({s[9]} reads with insertions, {s[10]} reads with deletions, {s[11]} reads with substitutions)\n"
        f"\t- Mixed HDR-NHEJ:{s[5]} reads ({s[12]} reads with insertions, {s[13]} reads with deletions, "
        f"{s[14]} reads with substitutions)\n\n"
        f"Total Aligned:{n_total} reads ").encode()
    files["Mapping_statistics.txt"] = (f"READS IN INPUTS:{rep.n_reads}\nREADS AFTER PREPROCESSING:{rep.n_reads}"
                                       f"\nREADS ALIGNED:{n_total}").encode()
    stems = dict(VECTOR_FILES)
    if rep.has_coding_seq:
        files["Frameshift_analysis.txt"] = (
            "Frameshift analysis:\n\t"
            f"Noncoding mutation:{c['non_modified_non_frameshift']} reads\n\t"
            f"In-frame mutation:{c['modified_non_frameshift']} reads\n\t"
            f"Frameshift mutation:{c['modified_frameshift']} reads\n").encode()
        files["Splice_sites_analysis.txt"] = (
            "Splice sites analysis:\n\t"
            f"Unmodified:{n_total - c['splicing_sites_modified']} reads\n\t"
            f"Potential splice sites modified:{c['splicing_sites_modified']} reads\n").encode()
        stems.update(CODING_FILES)
    if rep.has_expected_hdr:
        stems.update(HDR_FILES)
    for stem, key in stems.items():
        files[stem + ".txt"] = vector_bytes(v[key])
    files["effect_vector_combined.txt"] = vector_bytes(100.0 * v["effect_vector_any"] / float(n_total))
    with np.errstate(divide="ignore", invalid="ignore"):
        avg_ins = v["avg_vector_ins_all"] / (v["effect_vector_insertion"] + v["effect_vector_insertion_hdr"]
                                             + v["effect_vector_insertion_mixed"])
        avg_del = v["avg_vector_del_all"] / (v["effect_vector_deletion"] + v["effect_vector_deletion_hdr"]
                                             + v["effect_vector_deletion_mixed"])
    for a in (avg_ins, avg_del):
        a[np.isnan(a)] = 0
        a[np.isinf(a)] = 0
    files["position_dependent_vector_avg_insertion_size.txt"] = vector_bytes(avg_ins)
    files["position_dependent_vector_avg_deletion_size.txt"] = vector_bytes(avg_del)
    for key, name in (("df_indels", "indel_histogram.txt"), ("df_insertion", "insertion_histogram.txt"),
                      ("df_deletion", "deletion_histogram.txt"), ("df_substitution", "substitution_histogram.txt")):
        files[name] = frames[key].to_csv(index=None, sep="\t").encode()
    return files


def read_quantification(path) -> list:
    """Slots 1 .. 5 read the way CRISPRessoPooled's summary reads the file
    (CRISPRessoPooledCORE.py:1326-1349): by line position, the integer after each line's label."""
    import re

    with open(path) as f:
        lines = f.read().split("\n")
    labels = {1: r"Unmodified:(\d+)", 2: r"NHEJ:(\d+)", 3: r"HDR:(\d+)", 4: r"Mixed HDR-NHEJ:(\d+)",
              6: r"Total Aligned:(\d+) reads"}
    got = {k: int(re.findall(pattern, lines[k])[0]) for k, pattern in labels.items()}
    assert lines[5] == "" and len(lines) == 7
    return [got[6], got[1], got[2], got[3], got[4]]
