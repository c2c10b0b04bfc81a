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
 * A row with an Expected_HDR amplicon compares two printed identities of different aln_len; for
 * it nws_printed and nws_flags_dual compute the printed value in tenths by integers (below).
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

/* ---- rows with an Expected_HDR amplicon: two printed identities per read ----------------------
 *
 * For such a row every read is aligned to the amplicon and to the Expected_HDR amplicon, and the
 * reference tests score_ref and score_repaired, both PRINTED (CORE:1849-1856, 536-548, 2014).  Their
 * alignment lengths differ, so thresholds on n_ident per aln_len do not do; the device computes the
 * printed value itself, in tenths, without formatting a float:
 *   t, r = divmod(1000 n_ident, aln_len); tenths = t when 2 r < aln_len, t + 1 when 2 r > aln_len,
 *   and t + tie_up[t] on a rounding midpoint (2 r == aln_len), where the double is the correctly
 *   rounded (2 t + 1) / 20 and what "%.1f" makes of it depends on t alone.
 * aln_len == 0 prints 0.  crispresso_amd.demux.printed_tables builds the host values.
 *
 * nws_set_printed: tie_up HOST uint8 [1000] of 0 / 1 (kept as 128 bytes of bits on the device),
 * keep_tenths = the smallest tenths whose value is > min_identity_score, hdr_tenths = the smallest
 * whose value is >= hdr_perfect_alignment_threshold, both in [0, 1001] (1001: none), else
 * NW_E_INVALID.  Replaces the previous values.  Synchronous. */
int nws_set_printed(nws_ctx* c, const uint8_t* tie_up, int32_t keep_tenths, int32_t hdr_tenths);

/* One lane per nw_stat record of d_stats (DEVICE, n records, 16-byte aligned): the printed identity
 * in tenths, 0 .. 1000, into d_tenths (DEVICE uint16 [n]); 0xFFFF for a record with NW_FLAG_EMPTY.
 * A record with aln_len outside [0, NWS_MAX_COLS] or n_ident outside [0, aln_len] is counted in
 * *n_out_of_range (may be NULL), gets 0xFFFF, and makes the call return NW_E_INVALID with the other
 * outputs written.  n == 0 launches nothing.  NW_E_STATE before nws_set_printed.  Synchronous. */
int nws_printed(nws_ctx* c, const void* d_stats, int64_t n, uint16_t* d_tenths, int64_t* n_out_of_range,
                float* kernel_ms);

/* nws_flags for a row with an Expected_HDR amplicon.  One lane per read: ref = the tenths of its
 * record in d_stats_ref (the pass against the amplicon), rep = d_tenths_rep[r] (nws_printed of the
 * pass against the Expected_HDR amplicon; 0xFFFF: no repaired score, every test on it is false):
 *   keep = !(flags & NW_FLAG_EMPTY) && (ref >= keep_tenths || rep >= keep_tenths)
 *   pre  = NWQ_PRE_UNMODIFIED iff ref == 1000
 *        | NWQ_PRE_HDR   iff ref < rep && rep >= hdr_tenths
 *        | NWQ_PRE_MIXED iff ref < rep && rep <  hdr_tenths
 * A read whose record is out of range as for nws_printed, or whose rep is neither <= 1000 nor
 * 0xFFFF, is counted in *n_out_of_range, gets keep = 0 and pre = 0, and makes the call return
 * NW_E_INVALID (the other outputs are written).  n == 0 launches nothing.  NW_E_STATE before
 * nws_set_printed.  Synchronous. */
int nws_flags_dual(nws_ctx* c, const void* d_stats_ref, const uint16_t* d_tenths_rep, int64_t n, uint8_t* d_pre,
                   uint8_t* d_keep, int64_t* n_out_of_range, float* kernel_ms);

/* ---- per-group reports: the identity filter on the quantifier's input, the size histograms ------
 *
 * The reference drops the reads below min_identity_score before it quantifies (CORE:1869, 2025), so
 * its effect vectors, frameshift counters and histograms hold kept reads only.  It also skips a row
 * that is UNMODIFIED before it touches any of them (CORE:480-481), and so does every path of the
 * quantifier for a read whose pre has NWQ_PRE_UNMODIFIED.  A dropped read handed to the quantifier
 * as UNMODIFIED therefore adds nothing to the totals: masking pre is masking the read.
 *
 * nws_mask_pre: one lane per read, d_pre_q[r] = d_keep[r] ? d_pre[r] : NWQ_PRE_UNMODIFIED (the HDR
 * and MIXED bits of a dropped read are cleared).  d_pre, d_keep, d_pre_q DEVICE uint8 [n]; d_pre_q
 * may be d_pre itself.  n == 0 launches nothing.  kernel_ms may be NULL.  Synchronous. */
int nws_mask_pre(nws_ctx* c, const uint8_t* d_pre, const uint8_t* d_keep, int64_t n, uint8_t* d_pre_q,
                 float* kernel_ms);

#define NWS_MAX_BINS 65536

/* The size histograms of a report (CORE:2345-2365, 2903-2905) from d_reads (DEVICE nwq_read [n],
 * 16-byte aligned) and d_keep (DEVICE uint8 [n]) into out (HOST int64 [5 * bins - 1]):
 *   ins [bins], del [bins], mut [bins]: the counts of n_inserted, n_deleted, n_mutated;
 *   indel [2 * bins - 1]: entry d + bins - 1 counts d = n_inserted - n_deleted.
 * Only reads with keep != 0 and cls >= 0 are counted.  A counted read with any of the three values
 * outside [0, bins) is counted in *n_out_of_range (may be NULL) and in no histogram, and makes the
 * call return NW_E_INVALID (the other reads' counts are written all the same).  1 <= bins <=
 * NWS_MAX_BINS, else NW_E_UNSUPPORTED; the caller passes max(len_amplicon, longest read) + 1.
 * Integer sums (LDS atomics per block for the low bins, one 64-bit atomic per non-zero bin per
 * block): the result is a function of the input alone.  n == 0 returns zeros and launches nothing.
 * kernel_ms may be NULL.  Synchronous. */
int nws_histograms(nws_ctx* c, const void* d_reads, const uint8_t* d_keep, int64_t n, int32_t bins, int64_t* out,
                   int64_t* n_out_of_range, float* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif
