/* crispr_alleles.h -- C ABI of the MI355X allele grouping.
 *
 * Replaces the per-read half of CRISPResso's allele table (the groupby over one DataFrame
 * row per read, CRISPResso/CRISPRessoCORE.py:2923-2946).  An alignment is a function of the
 * read's bytes, and align_seq without its '-' is the read, so within one batch against one
 * amplicon (or amplicon + HDR pair) the reference's groups are the groups of byte-identical
 * reads: they are found in HBM on the batch the aligner left there (nw_batch_device_ops,
 * include/crispr_nw.h), and only one representative per group gets its strings built.
 *
 * Group key = (tag, length, bytes); two kept reads are in one group iff all three are equal.
 * Groups come in order of first appearance: first[g] is the smallest read index of group g
 * and strictly increases with g; count[g] is the group's size.  The result is a function of
 * the input alone (no atomic ordering shows in it).
 *
 * The binding a maintainer adds is crispresso_amd/alleles.py (ctypes).  Error codes are the
 * NW_E_* of include/crispr_nw.h.
 */
#ifndef CRISPR_ALLELES_H
#define CRISPR_ALLELES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nwa_ctx nwa_ctx;

/* CRISPR_NWA_HASH_BITS=k (0..64, default 64) is read here: only the low k bits of every
 * read's hash are kept (before the hash is forced nonzero), so that tests can drive the probe
 * chains and the collided path on small inputs. */
int nwa_create(int device, nwa_ctx** out);
void nwa_destroy(nwa_ctx* c);
const char* nwa_last_error(const nwa_ctx* c);

/* Groups of the n reads of a device-resident batch of this context's GPU: read r is the
 * bytes at d_reads + d_offsets[r] - reads_bias, length d_offsets[r + 1] - d_offsets[r]
 * (nw_batch_device_ops' reads: upper case; N, '-' and IUPAC bytes are ordinary bytes).
 * keep (uint8 [n]: 0 drops the read), tag (int32 [n]: part of the key; pooled runs pass
 * ref_of_read) and group_of_read (int32 [n] out: the read's group, -1 when not kept) are
 * HOST arrays or NULL.  first / count: int64 HOST arrays of capacity cap; *n_groups = the
 * number of groups.  NW_E_CAPACITY with *n_groups = the number needed when cap is short
 * (nothing else written); NW_E_INVALID for n < 0 or n > 2^31 - 1; n == 0 gives zero groups.
 * kernel_ms (may be NULL): device time of the call's kernels.  Synchronous. */
int nwa_group_device(nwa_ctx* c, const uint8_t* d_reads, const int64_t* d_offsets, int64_t reads_bias, int64_t n,
                     const uint8_t* keep, const int32_t* tag, int64_t* first, int64_t* count, int64_t cap,
                     int32_t* group_of_read, int64_t* n_groups, float* kernel_ms);

/* Reads of the last nwa_group_device whose bytes differed from the first read of their hash
 * (equal hashes, different reads): they were copied back and grouped exactly on the host. */
int64_t nwa_last_collided(const nwa_ctx* c);

/* Device time of the last nwa_group_device by phase: ms[0] hash, ms[1] insert, ms[2] verify,
 * ms[3] compaction (scan, group emit, group_of_read).  A diagnostic (scripts/bench_alleles.py). */
int nwa_phase_times(const nwa_ctx* c, float* ms);

/* Reads one step of the hash / verify launch takes at its full grid (16 blocks of 4 wavefronts
 * per CU, one read per wavefront): a batch of more than twice as many gives every wavefront
 * several.  A diagnostic (tests). */
int64_t nwa_reads_per_step(const nwa_ctx* c);

/* The same contract on host text (read r = reads[offsets[r] .. offsets[r + 1])), case
 * sensitive; no GPU, no context.  nthreads <= 0: the process's host threads. */
int nwa_group_host(const char* reads, const int64_t* offsets, int64_t n, const uint8_t* keep, const int32_t* tag,
                   int64_t* first, int64_t* count, int64_t cap, int32_t* group_of_read, int64_t* n_groups,
                   int32_t nthreads);

/* 1 when any byte of the n reads is 'a'..'z', else 0 (negative: NW_E_INVALID).  The 2-bit
 * pack and the device bytes are upper case: device grouping would merge "acgt" with "ACGT"
 * while align_seq keeps the text, so such batches are grouped by nwa_group_host. */
int nwa_reads_have_lower(const char* reads, const int64_t* offsets, int64_t n, int32_t nthreads);

/* The allele table around a cut site (get_row_around_cut / get_dataframe_around_cut,
 * CRISPRessoCORE.py:801-836) of a device-resident ops-mode batch, per cut point, without a
 * string for any full-length allele (crispresso_amd/csrc/nw_windows.hip).
 *
 * d_ops / d_ops_off / d_stats / d_reads / d_offsets / reads_bias: nw_batch_device_ops' DEVICE
 * arrays of the n reads (runs type << 28 | length, their offsets, the nw_stat records, the read
 * bytes); awidth: the columns parse_needle_output keeps (needle -awidth3).  amplicon: HOST
 * bytes, amp_len of them, every one of A C G T N.  cut_points: HOST int32 [n_cuts], each in
 * [0, amp_len); 1 <= offset <= 64; amp_len <= 16384.  Anything else is NW_E_UNSUPPORTED: the
 * caller takes allele_table + around_cut_from_alleles (crispresso_amd/alleles.py).  keep / tag:
 * HOST arrays or NULL, as nwa_group_device takes them.  read_results: the HOST [n][4] int32
 * array of nwq_read (cls first; cls == 0 is UNMODIFIED).
 *
 * The window of a kept read for cut point p is columns [cut_idx - offset + 1, cut_idx + offset + 1)
 * of its aligned-read row and of its reference row, both cut to min(aln_len, awidth) columns,
 * under Python's slice rules (a negative start counts from the end, a stop past the end is
 * clipped); cut_idx is the column that holds amplicon base p.  Windows are grouped by
 * (tag, length, both rows) in order of first appearance, exactly (collided records go through
 * nwa_group_device's host path).
 *
 * *n_no_cut = the kept (cut point, read) pairs whose first min(aln_len, awidth) columns do not
 * hold base p (the reference's ValueError), *first_no_cut = the smallest such read (-1: none).
 * When there is one, NW_OK is returned, n_groups is all zero and nothing is kept for
 * nwa_windows_fetch.  Otherwise n_groups[k] = the groups of cut point k, kept on the context
 * until its next nwa_windows_device.  Cut points beyond what one launch takes are looped here.
 * Synchronous. */
int nwa_windows_device(nwa_ctx* c, const uint32_t* d_ops, const int64_t* d_ops_off, const void* d_stats,
                       const uint8_t* d_reads, const int64_t* d_offsets, int64_t reads_bias, int64_t n, int32_t awidth,
                       const char* amplicon, int32_t amp_len, const int32_t* cut_points, int32_t n_cuts, int32_t offset,
                       const uint8_t* keep, const int32_t* tag, const int32_t* read_results, int32_t want_group_of_read,
                       int64_t* n_groups, int64_t* n_no_cut, int64_t* first_no_cut);

/* The groups of cut point k of the last nwa_windows_device into HOST arrays (any may be NULL):
 * win uint8 [groups][2][2 * offset] (the aligned-read row, then the reference row, zero-padded
 * past win_len), win_len int32, first / count int64, unedited uint8 (some read of the group has
 * cls == 0), group_of_read int32 [n] (-1: not kept; NW_E_STATE unless want_group_of_read was set). */
int nwa_windows_fetch(const nwa_ctx* c, int32_t k, uint8_t* win, int32_t* win_len, int64_t* first, int64_t* count,
                      uint8_t* unedited, int32_t* group_of_read);

/* nwa_windows_device with the keep flags and the results in HBM: d_keep (uint8 [n], non-zero
 * = kept, or NULL) and d_results (nwq_read [n]) are DEVICE arrays, as a resident summary leaves
 * them (nws_flags, nwq_run_device_ops); the kept count comes from a device reduction and
 * cls == 0 is tested on the device.  tag stays a HOST array or NULL.  Everything else (limits,
 * NW_E_UNSUPPORTED cases, the no-cut report, nwa_windows_fetch) as nwa_windows_device: the two
 * share one body.  Synchronous. */
int nwa_windows_resident(nwa_ctx* c, const uint32_t* d_ops, const int64_t* d_ops_off, const void* d_stats,
                         const uint8_t* d_reads, const int64_t* d_offsets, int64_t reads_bias, int64_t n, int32_t awidth,
                         const char* amplicon, int32_t amp_len, const int32_t* cut_points, int32_t n_cuts, int32_t offset,
                         const uint8_t* d_keep, const int32_t* tag, const int32_t* d_results, int32_t want_group_of_read,
                         int64_t* n_groups, int64_t* n_no_cut, int64_t* first_no_cut);

/* Records of the last nwa_windows_device / nwa_windows_resident that went through the exact host
 * path, over its cut points. */
int64_t nwa_windows_collided(const nwa_ctx* c);

/* Device time of the last nwa_windows_device: ms[0] extract, ms[1] grouping (hash .. compaction),
 * ms[2] unedited + gather.  A diagnostic (scripts/bench_around_cut.py). */
int nwa_windows_times(const nwa_ctx* c, float* ms);

/* The allele table's rows (CRISPRessoCORE.py:2923-2946) of a device-resident ops-mode batch
 * whose keep flags and results are in HBM as well: no read's text is needed on the host
 * (crispresso_amd/csrc/nw_allele_rows.hip).
 *
 * d_ops .. reads_bias, n, awidth, amplicon (HOST bytes, any; copied to the device), amp_len: as
 * nwa_windows_device takes them.  d_keep: DEVICE uint8 [n], non-zero = kept, or NULL (all
 * kept).  d_results: DEVICE nwq_read [n].
 *
 * The kept reads are grouped by their bytes exactly as nwa_group_device groups them (no tag):
 * groups in order of first appearance; reads whose hash collided go through the exact host path.
 * For the first read of every group one wavefront walks the read's runs and writes the
 * aligned-read row and the reference row, cut to cols = min(aln_len, awidth) columns, into a
 * DEVICE buffer [groups][2][*row_stride], zero-padded past cols; *row_stride is the largest cols
 * rounded up to 16 (at least 16).  The same launch gathers cols, the group's first read and
 * size, and the first read's nwq_read.  The device bytes are upper case, as the whole resident
 * path is.
 *
 * NW_E_INVALID (nothing kept for nwa_table_fetch, *n_groups = 0) when the runs of a group's
 * first read do not end at the end of its bytes and of the amplicon, hold an unknown run type or
 * fewer columns than cols (nw_expand_ops_subset refuses the same runs); such a byte is never
 * loaded.  A kept read without a byte and without a run has cols = 0 and is not an error.
 * n == 0 or nothing kept: zero groups.  The result is a function of the input alone.  Kept on
 * the context until its next nwa_table_device.  Synchronous. */
int nwa_table_device(nwa_ctx* c, const uint32_t* d_ops, const int64_t* d_ops_off, const void* d_stats,
                     const uint8_t* d_reads, const int64_t* d_offsets, int64_t reads_bias, int64_t n, int32_t awidth,
                     const char* amplicon, int32_t amp_len, const uint8_t* d_keep, const int32_t* d_results,
                     int64_t* n_groups, int32_t* row_stride);

/* The groups of the last nwa_table_device into HOST arrays (any may be NULL): rows uint8
 * [groups][2][row_stride] (the aligned-read row, then the reference row), cols int32, first /
 * count int64, results int32 [groups][4] (the first read's nwq_read). */
int nwa_table_fetch(nwa_ctx* c, uint8_t* rows, int32_t* cols, int64_t* first, int64_t* count, int32_t* results);

/* Reads of the last nwa_table_device that went through the exact host path. */
int64_t nwa_table_collided(const nwa_ctx* c);

/* Device time of the last nwa_table_device: ms[0] grouping (hash .. compaction), ms[1] the column
 * and row kernels.  A diagnostic (scripts/bench_pooled_alleles.py). */
int nwa_table_times(const nwa_ctx* c, float* ms);

#ifdef __cplusplus
}
#endif
#endif
