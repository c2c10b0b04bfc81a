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

#ifdef __cplusplus
}
#endif
#endif
