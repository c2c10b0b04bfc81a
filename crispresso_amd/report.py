"""The per-target result folder of a resident run: what CRISPRessoPooled and CRISPRessoWGS leave
as ``CRISPResso_on_<name>`` (CRISPRessoPooledCORE.py:882-913, CRISPRessoWGSCORE.py:718-747), from
the integers :func:`crispresso_amd.demux.summarize_pooled` and
:func:`crispresso_amd.regions.summarize_regions` hand to their ``reports`` callback.

Host code only: a :class:`GroupReport` holds one group's exact integers (``nws_summary``'s 16
slots, the quantifier's totals over the kept reads, ``nws_histograms``' four size histograms),
:func:`tables` makes the four histogram tables of :func:`crispresso_amd.quantify.run_summary` of
them, :func:`write_report` the files CRISPRessoCompare and CRISPRessoPooledWGSCompare read
(CRISPRessoCompareCORE.py:39-49) and the rest of the reference's text output.  With the callers'
``alleles=True`` a report also carries the allele table and the tables around the cut sites, made
from the resident batch without a read's text on the host (:mod:`crispresso_amd.alleles`;
upper case, as the whole resident path is), and ``Alleles_frequency_table.txt`` and
``Alleles_frequency_table_around_cut_site_for_<sgRNA>.txt`` are written too.  The plots and the
pickles are not written.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np

from . import quantify

HISTOGRAM_FILES = (("df_indels", "indel_histogram.txt"), ("df_insertion", "insertion_histogram.txt"),
                   ("df_deletion", "deletion_histogram.txt"), ("df_substitution", "substitution_histogram.txt"))


class ReportError(ValueError):
    """A report that cannot be written: no read of the group passed the identity filter."""


@dataclass
class GroupReport:
    """One summarized group.  ``slots``: ``nws_summary``'s 16 integers (``_lib.NWS_SLOT_NAMES``).
    ``totals``: :meth:`crispresso_amd.quantify.GpuQuantifier.unpack_totals` of the quantifier's
    pass over the kept reads (vectors, counters and the two frameshift histograms).  ``hist_ins``,
    ``hist_del``, ``hist_mut``: int64 ``[bins]``, the kept reads with that ``n_inserted``,
    ``n_deleted``, ``n_mutated``; ``hist_indel``: int64 ``[2 bins - 1]``, entry ``d + bins - 1``
    the kept reads with ``n_inserted - n_deleted == d``.  ``alleles``: the group's ``df_alleles``
    (:func:`crispresso_amd.alleles.resident_allele_table`) or None; ``around_cut``: a list of
    ``(sgRNA, cut_point, frame)``, one per pair of ``zip(guides, cut_points)`` as the reference
    pairs them (CRISPRessoCORE.py:3643-3654: a guide with two matches gets the file of its first
    cut point only, and later guides get the cut points that follow), or None."""

    name: str
    amplicon: str
    cut_points: Sequence[int]
    n_reads: int                       # the group's size, filtered reads included
    slots: np.ndarray
    totals: Dict
    hist_ins: np.ndarray
    hist_del: np.ndarray
    hist_mut: np.ndarray
    hist_indel: np.ndarray
    has_coding_seq: bool = False
    has_expected_hdr: bool = False
    alleles: Optional["pd.DataFrame"] = None
    around_cut: Optional[list] = None

    @property
    def n_total(self) -> int:
        return int(self.slots[1])


def folder_name(name: str) -> str:
    """``CRISPResso_on_<clean_filename(name)>``: the name CRISPRessoPooledWGSCompare looks up
    (CRISPRessoPooledWGSCompareCORE.py:243-246)."""
    from .demux import clean_filename

    return "CRISPResso_on_%s" % clean_filename(name)


def tables(report: GroupReport) -> Dict:
    """``df_indels``, ``df_insertion``, ``df_deletion``, ``df_substitution``: equal to what
    :func:`crispresso_amd.quantify.run_summary` makes of the kept reads' DataFrame.  The
    histograms are expanded to one value per read (four int64 columns of the group's size on the
    host) and go through the same helper, so numpy's closed last bin and its percentile are
    numpy's own."""
    bins = len(report.hist_ins)
    sizes = np.arange(bins, dtype=np.int64)
    indel = np.repeat(np.arange(-(bins - 1), bins, dtype=np.int64), report.hist_indel)
    return quantify.size_tables(indel, np.repeat(sizes, report.hist_ins), np.repeat(sizes, report.hist_del),
                                np.repeat(sizes, report.hist_mut), len(report.amplicon), report.cut_points)


def save_vector(path: str, vector) -> None:
    """One vector along the amplicon as the reference's ``save_vector_to_file`` writes it
    (CRISPRessoCORE.py:3739-3749): position + 1 and the value, ``%d`` and ``%.18e``."""
    v = np.asarray(vector, dtype=np.float64)
    np.savetxt(path, np.column_stack([np.arange(len(v)) + 1, v]), fmt=["%d", "%.18e"], delimiter="\t",
               header="amplicon position\teffect", comments="# ")


def average_sizes(size_sums, *counts) -> np.ndarray:
    """CORE:2876-2890: the size sums over the summed counts, nan and inf set to 0."""
    den = np.sum([np.asarray(c, dtype=np.float64) for c in counts], axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = np.asarray(size_sums, dtype=np.float64) / den
    avg[~np.isfinite(avg)] = 0
    return avg


def quantification_text(slots) -> str:
    """Quantification_of_editing_frequency.txt (CORE:3805-3832) from the 16 slots."""
    s = [int(x) for x in slots]
    lines = ["Quantification of editing frequency:", "\t- Unmodified:%d reads" % s[2]]
    for label, n, k in (("NHEJ", s[3], 6), ("HDR", s[4], 9), ("Mixed HDR-NHEJ", s[5], 12)):
        lines.append("\t- %s:%d reads (%d reads with insertions, %d reads with deletions, %d reads with substitutions)"
                     % (label, n, s[k], s[k + 1], s[k + 2]))
    return "\n".join(lines) + "\n\nTotal Aligned:%d reads " % s[1]


def write_report(folder: str, report: GroupReport) -> list:
    """The group's files into ``folder`` (created), in the reference's formats; returns their
    names.  Always: Quantification_of_editing_frequency.txt, Mapping_statistics.txt (the reads in
    input and after preprocessing are both the group's size), the NHEJ and combined effect
    vectors, the two average-size vectors and the four histogram tables.  With a coding sequence
    the frameshift and splice-site counts and the noncoding vectors; with an Expected_HDR the HDR
    and mixed vectors.  With ``report.alleles`` Alleles_frequency_table.txt (the columns through
    ``%Reads``, no index; CORE:3835), and for every entry of ``report.around_cut``
    Alleles_frequency_table_around_cut_site_for_<sgRNA>.txt (the index kept; CORE:3649); with
    both None not a byte more than without them.  A report without a kept read raises :class:`ReportError`: the reference
    stops such a run (CORE:2027)."""
    n_total = report.n_total
    if n_total == 0:
        raise ReportError(f"{report.name}: zero sequences aligned, no report is written")
    os.makedirs(folder, exist_ok=True)
    written = []

    def text(name: str, body: str) -> None:
        with open(os.path.join(folder, name), "wt", encoding="utf-8") as f:
            f.write(body)
        written.append(name)

    def vector(name: str, v) -> None:
        save_vector(os.path.join(folder, name + ".txt"), v)
        written.append(name + ".txt")

    v, c = report.totals["vectors"], report.totals["counters"]
    text("Quantification_of_editing_frequency.txt", quantification_text(report.slots))
    text("Mapping_statistics.txt", "READS IN INPUTS:%d\nREADS AFTER PREPROCESSING:%d\nREADS ALIGNED:%d"
         % (report.n_reads, report.n_reads, n_total))
    if report.has_coding_seq:
        text("Frameshift_analysis.txt",
             "Frameshift analysis:\n\tNoncoding mutation:%d reads\n\tIn-frame mutation:%d reads\n\tFrameshift mutation:%d reads\n"
             % (c["non_modified_non_frameshift"], c["modified_non_frameshift"], c["modified_frameshift"]))
        text("Splice_sites_analysis.txt",
             "Splice sites analysis:\n\tUnmodified:%d reads\n\tPotential splice sites modified:%d reads\n"
             % (n_total - c["splicing_sites_modified"], c["splicing_sites_modified"]))
        vector("effect_vector_insertion_noncoding", v["effect_vector_insertion_noncoding"])
        vector("effect_vector_deletion_noncoding", v["effect_vector_deletion_noncoding"])
        vector("effect_vector_substitution_noncoding", v["effect_vector_mutation_noncoding"])
    vector("effect_vector_insertion_NHEJ", v["effect_vector_insertion"])
    vector("effect_vector_deletion_NHEJ", v["effect_vector_deletion"])
    vector("effect_vector_substitution_NHEJ", v["effect_vector_mutation"])
    vector("effect_vector_combined", 100.0 * np.asarray(v["effect_vector_any"], dtype=np.float64) / float(n_total))
    vector("position_dependent_vector_avg_insertion_size",
           average_sizes(v["avg_vector_ins_all"], v["effect_vector_insertion"], v["effect_vector_insertion_hdr"],
                         v["effect_vector_insertion_mixed"]))
    vector("position_dependent_vector_avg_deletion_size",
           average_sizes(v["avg_vector_del_all"], v["effect_vector_deletion"], v["effect_vector_deletion_hdr"],
                         v["effect_vector_deletion_mixed"]))
    frames = tables(report)
    for key, name in HISTOGRAM_FILES:
        frames[key].to_csv(os.path.join(folder, name), index=None, sep="\t")
        written.append(name)
    if report.has_expected_hdr:
        vector("effect_vector_insertion_mixed_hdr_nhej", v["effect_vector_insertion_mixed"])
        vector("effect_vector_deletion_mixed_hdr_nhej", v["effect_vector_deletion_mixed"])
        vector("effect_vector_substitution_mixed_hdr_nhej", v["effect_vector_mutation_mixed"])
        vector("effect_vector_insertion_HDR", v["effect_vector_insertion_hdr"])
        vector("effect_vector_deletion_HDR", v["effect_vector_deletion_hdr"])
        vector("effect_vector_substitution_HDR", v["effect_vector_mutation_hdr"])
    if report.alleles is not None:                  # CORE:3835
        report.alleles.loc[:, :"%Reads"].to_csv(os.path.join(folder, ALLELES_FILE), sep="\t", header=True, index=None)
        written.append(ALLELES_FILE)
    for sgrna, _, frame in report.around_cut or ():  # CORE:3643-3654 (a guide met twice writes its file twice)
        name = around_cut_file(sgrna)
        frame.to_csv(os.path.join(folder, name), sep="\t", header=True)
        if name not in written:
            written.append(name)
    return written


ALLELES_FILE = "Alleles_frequency_table.txt"


def around_cut_file(sgrna: str) -> str:
    return "Alleles_frequency_table_around_cut_site_for_%s.txt" % sgrna


def guide_cut_pairs(guide_seq: Optional[str], cut_points: Sequence[int]) -> list:
    """``zip(sg_rna_sequences, cut_points)`` as the reference pairs them (CORE:1290-1341,
    3643): the guides are the comma-separated, upper-cased sgRNAs in the order given, the cut
    points every match of every guide in that order; the shorter list ends the pairing."""
    guides = [g for g in (guide_seq or "").strip().upper().split(",")] if guide_seq else []
    return list(zip(guides, [int(c) for c in cut_points]))
