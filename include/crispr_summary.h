/* crispr_summary.h -- C ABI of the MI355X per-amplicon summary of the pooled amplicon mode.
 *
 * CRISPRessoPooled ends in SAMPLES_QUANTIFICATION_SUMMARY.txt (CRISPRessoPooledCORE.py:1315-1416):
 * per amplicon the reads aligned and their shares of Unmodified, NHEJ, HDR and Mixed.  Between
 * the aligner's records and that table the reference does two things per read on the host: the
 * identity filter on the PRINTED identity (CRISPRessoCORE.py:1997-2014: score_ref =
 * float("%.1f" % (100 n_ident / aln_len)), kept iff > min_identity_score, UNMODIFIED iff == 100)
 * and the counts over the quantified rows (CORE:2025, 2866-2869, 3751-3803).  Both are done here
 * on the resident group: nws_flags makes the quantifier's `pre` flags and the `keep` mask from
 * the nw_stat records, nws_summary counts the quantifier's nwq_read records into 16 integers.
 *
 * The device never formats a float.  The printed identity is non-decreasing in n_ident at a
 * fixed aln_len, so both tests are thresholds on n_ident, read from two host-built tables
 * indexed by aln_len (crispresso_amd.demux.identity_thresholds):
 *   keep_min[L]  = the smallest n_ident whose printed identity is > min_identity_score, L + 1 if none;
 *   unmod_min[L] = the smallest n_ident that prints 100.0, L + 1 if none.
 *
 * The binding is crispresso_amd/demux.py (ctypes).  Error codes are the NW_E_* of crispr_nw.h.
 */
#ifndef CRISPR_SUMMARY_H
#define CRISPR_SUMMARY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nws_ctx nws_ctx;

/* The slots of nws_summary's output.  All but NWS_N are counted over the kept reads. */
enum {
    NWS_N = 0,               /* n, the records given */
    NWS_TOTAL = 1,           /* n_total: the kept reads */
    NWS_UNMODIFIED = 2,      /* pre & NWQ_PRE_UNMODIFIED or cls == 0 (quantify._result_tuple's column) */
    NWS_MODIFIED = 3,        /* n_modified: cls == 1 (NHEJ) */
    NWS_REPAIRED = 4,        /* n_repaired: cls == 2 (HDR) */
    NWS_MIXED = 5,           /* n_mixed_hdr_nhej: cls == 3 */
    NWS_NHEJ_INSERTED = 6,   /* 6..14: nhej / hdr / mixed x reads with n_inserted > 0, n_deleted > 0, */
    NWS_NHEJ_DELETED = 7,    /*        n_mutated > 0, in quantify.run_summary's order */
    NWS_NHEJ_MUTATED = 8,
    NWS_HDR_INSERTED = 9,
    NWS_HDR_DELETED = 10,
    NWS_HDR_MUTATED = 11,
    NWS_MIXED_INSERTED = 12,
    NWS_MIXED_DELETED = 13,
    NWS_MIXED_MUTATED = 14,
    NWS_NOT_ALIGNED = 15,    /* kept reads with cls < 0 */
    NWS_SLOTS = 16
};

#define NWS_MAX_COLS (1 << 20)

int nws_create(int device, nws_ctx** out);
void nws_destroy(nws_ctx* c);
const char* nws_last_error(const nws_ctx* c);

/* The two threshold tables, HOST int32 [max_cols + 1] indexed by aln_len, copied to the device.
 * 0 <= max_cols <= NWS_MAX_COLS, else NW_E_UNSUPPORTED.  Replaces the previous tables.  Synchronous. */
int nws_set_identity(nws_ctx* c, const int32_t* keep_min, const int32_t* unmod_min, int32_t max_cols);

/* One lane per nw_stat record (include/crispr_nw.h) of d_stats (DEVICE, n records, 16-byte aligned
 * as nw_batch_device_ops gives them, else NW_E_INVALID):
 *   keep = !(flags & NW_FLAG_EMPTY) && n_ident >= keep_min[aln_len]
 *   pre  = NWQ_PRE_UNMODIFIED iff n_ident >= unmod_min[aln_len], else 0
 * written to d_keep and d_pre (DEVICE uint8 [n]).  A record whose aln_len lies outside
 * [0, max_cols] is counted in *n_out_of_range (may be NULL), gets keep = 0 and pre = 0, and makes
 * the call return NW_E_INVALID (the other records' outputs are written all the same).  n == 0
 * returns zeros and launches nothing.  NW_E_STATE before nws_set_identity.  kernel_ms may be NULL.
 * Synchronous. */
int nws_flags(nws_ctx* c, const void* d_stats, int64_t n, uint8_t* d_pre, uint8_t* d_keep, int64_t* n_out_of_range,
              float* kernel_ms);

/* The 16 slots above from d_reads (DEVICE nwq_read [n], include/crispr_quant.h, 16-byte aligned), d_pre and d_keep
 * (DEVICE uint8 [n]) into out (HOST int64 [NWS_SLOTS]).  Ballot and popcount within a wavefront,
 * a sum within the block, then one integer atomic per counter per block: integer sums, so the
 * result is a function of the input alone.  n == 0 returns zeros and launches nothing.
 * kernel_ms may be NULL.  Synchronous. */
int nws_summary(nws_ctx* c, const void* d_reads, const uint8_t* d_pre, const uint8_t* d_keep, int64_t n, int64_t* out,
                float* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif
