/* crispr_demux.h -- C ABI of the MI355X pooled-amplicon demultiplexing.
 *
 * Replaces the bowtie2 step of CRISPRessoPooled's ONLY_AMPLICONS mode
 * (CRISPResso/CRISPRessoPooledCORE.py:843-878): the index of the amplicons, the mapping of every
 * read, and the split of the mapped reads into one set per amplicon.  It is not bowtie2 (no seed
 * extension, no random tie-break, no MAPQ, no soft clipping, no genome); it is the rule below,
 * deterministic, restated in tests/demux_model.py.
 *
 * Parameters: k, the window length, 8 <= k <= 31 (a window is an exact 2k-bit key); min_hits >= 1;
 * both_strands.
 *
 * Bases: A C G T a c g t map to 0..3 (case is ignored, as in the packer).  Any other byte is a
 * break: a window that contains a break casts no vote, in an amplicon or in a read.
 *
 * Index: every break-free length-k window of every amplicon's forward strand maps to that
 * amplicon's index g.  A window that occurs in two or more distinct amplicons maps to AMBIGUOUS
 * and never votes; repeats inside one amplicon stay g.  The index is a function of the amplicon
 * set alone (insertion order does not show in it).
 *
 * Votes, for a read of n bytes and every p in [0, n - k]: if w = read[p .. p + k) is break-free
 * and indexed to g, it is one vote for (g, strand 0); with both_strands, if the reverse
 * complement of w is indexed to g', it is one vote for (g', strand 1).  A palindromic window
 * votes on both strands.
 *
 * Decision: best = the largest vote count over all (g, s) pairs; rival = the largest count over
 * all other pairs (the same amplicon on the other strand is a rival);
 *   which = g, strand = s   iff best >= min_hits and best > rival;
 *   which = NWD_NO_HIT      when best < min_hits (reads shorter than k, the empty read);
 *   which = NWD_TIE         otherwise.
 * votes (= best) and rival are returned per read for all three outcomes; strand is 0 for a read
 * that is not assigned.
 *
 * Gathered output: group g holds the reads with which == g in ascending input index.  A strand-1
 * read's bytes are reversed and complemented (A<->T C<->G a<->t c<->g, every other byte
 * unchanged): what bowtie2's SAM field 10 would hold, the amplicon's orientation.  Strand-0 reads
 * are copied as given.
 *
 * The result is a function of the input alone (no atomic ordering shows in it).  The binding is
 * crispresso_amd/demux.py (ctypes).  Error codes are the NW_E_* of include/crispr_nw.h.
 */
#ifndef CRISPR_DEMUX_H
#define CRISPR_DEMUX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nwd_ctx nwd_ctx;

#define NWD_NO_HIT (-1)
#define NWD_TIE (-2)
#define NWD_MIN_K 8
#define NWD_MAX_K 31
#define NWD_MAX_REFS 65535
#define NWD_MAX_REF_BASES (1 << 24)
#define NWD_MAX_READ 4096
#define NWD_MAX_TALLY_SLOTS 256

/* Read here, so that tests reach the edges on small inputs:
 *   CRISPR_NWD_CHUNK=<reads>       reads per chunk (default: chunks of about 64 MiB of text);
 *   CRISPR_NWD_TALLY_SLOTS=<s>     (1..NWD_MAX_TALLY_SLOTS, default 64) distinct (amplicon, strand)
 *                                  candidates a read's tally holds on the device; a read with
 *                                  more is decided by the exact path (nwd_last_fallback). */
int nwd_create(int device, nwd_ctx** out);
void nwd_destroy(nwd_ctx* c);
const char* nwd_last_error(const nwd_ctx* c);

/* Builds the index of n_refs amplicons in HBM: amplicon g = refs[ref_offsets[g] ..
 * ref_offsets[g + 1]) (HOST memory, offsets int64 [n_refs + 1] ascending).  1 <= n_refs <=
 * NWD_MAX_REFS, ref_offsets[n_refs] - ref_offsets[0] <= NWD_MAX_REF_BASES, NWD_MIN_K <= k <=
 * NWD_MAX_K; anything else is NW_E_UNSUPPORTED.  *n_windows = distinct windows in the index,
 * *n_ambiguous = those of them that map to AMBIGUOUS (either may be NULL).  Replaces the
 * context's previous index.  Synchronous. */
int nwd_set_amplicons(nwd_ctx* c, const uint8_t* refs, const int64_t* ref_offsets, int64_t n_refs, int32_t k,
                      int64_t* n_windows, int64_t* n_ambiguous);

/* Assigns n reads held in HOST memory: read r = reads[offsets[r] .. offsets[r + 1]), offsets
 * int64 [n + 1] ascending, 0 <= n <= 2^31 - 1.  A read longer than NWD_MAX_READ bases (the front
 * end's limit) or min_hits < 1 is NW_E_UNSUPPORTED; a call before nwd_set_amplicons NW_E_STATE.
 *
 * Per-read outputs (HOST, each may be NULL): which int32 [n] (g, NWD_NO_HIT or NWD_TIE), strand
 * uint8 [n], votes / rival int32 [n].  counts int64 [n_refs] (may be NULL): reads assigned to
 * each amplicon.  *n_assigned + *n_tie + *n_no_hit = n (each may be NULL).  n == 0 returns zeros
 * without touching the GPU.  kernel_ms (may be NULL): device time of the call's kernels.  The
 * reads and the decisions stay on the device for nwd_gather until the next call.  Synchronous. */
int nwd_assign(nwd_ctx* c, const uint8_t* reads, const int64_t* offsets, int64_t n, int32_t min_hits,
               int32_t both_strands, int32_t* which, uint8_t* strand, int32_t* votes, int32_t* rival,
               int64_t* counts, int64_t* n_assigned, int64_t* n_tie, int64_t* n_no_hit, float* kernel_ms);

/* nwd_assign on the merged reads the front end left in HBM (a live nwp_result of nwp_prepare /
 * nwp_prepare_records, include/crispr_front.h), with no upload: the dense text is copied device to
 * device into the context's text buffer, behind the event recorded after the front end's packer,
 * in nwd_assign's layout and nwd_assign's chunks (CRISPR_NWD_CHUNK applies), and assigned by the
 * same kernel.  A read whose tally overflowed is copied down alone and decided by the host path.
 * Read r is the result's read r (its offsets are nwp_fetch's); n is its m.  Outputs as nwd_assign.
 * Afterwards nwd_gather, nwd_pack and nwd_adopt_group behave exactly as after nwd_assign of the
 * same text, and the result may be released at once.  A null or released result, or one on
 * another device, is NW_E_INVALID; a call before nwd_set_amplicons NW_E_STATE; m == 0 returns
 * zeros without touching the GPU.  Synchronous. */
int nwd_assign_prepared(nwd_ctx* c, const struct nwp_result* res, int32_t min_hits, int32_t both_strands,
                        int32_t* which, uint8_t* strand, int32_t* votes, int32_t* rival, int64_t* counts,
                        int64_t* n_assigned, int64_t* n_tie, int64_t* n_no_hit, float* kernel_ms);

/* The assigned reads of the last nwd_assign, grouped: group_offsets int64 [n_refs + 1] (group g
 * is the gathered reads group_offsets[g] .. group_offsets[g + 1]), order int64 [n_assigned] the
 * input index of each gathered read, text_offsets int64 [n_assigned + 1] into text [text_cap],
 * the gathered bytes (strand-1 reads reverse-complemented on the device).  *needed (may be NULL)
 * = the bytes text must hold; when text_cap is short the call returns NW_E_CAPACITY with
 * *needed, group_offsets, order and text_offsets written (each may be NULL).  Synchronous. */
int nwd_gather(nwd_ctx* c, int64_t* group_offsets, int64_t* order, uint8_t* text, int64_t* text_offsets,
               int64_t text_cap, int64_t* needed);

/* The grouped reads of the last nwd_assign as a packed batch in HBM, without the gathered text:
 * exactly what nw_pack_reads (include/crispr_nw.h) makes of nwd_gather's text and text_offsets.
 * Position text_offsets[j] + p is base p of gathered read j (a strand-1 read reversed and
 * complemented on the fly).  The 2-bit stream holds 16 bases a dword, base i in bits 2 (i % 4) of
 * byte i / 4, A C T G = 0 1 2 3; every byte that is none of A C G T a c g t is an exception
 * (position and the byte itself, ascending; complementing leaves such a byte as it is) and gives
 * 0 bits, as does a position past the end.  The stream is defined up to byte
 * (text_offsets[n_assigned] + 3) / 4.
 *
 * Host outputs, each may be NULL: group_offsets, order and text_offsets as nwd_gather gives them;
 * lens uint16 [n_assigned]; group_exc int64 [n_refs + 1]: group g's exceptions are the slots
 * group_exc[g] .. group_exc[g + 1] of the list; *n_exc their number; *kernel_ms the device time of
 * the packer's kernels.  NW_E_STATE before nwd_set_amplicons; 2^32 or more gathered bytes are
 * NW_E_UNSUPPORTED.  With no assigned read it returns zeros and launches nothing.  The packed
 * arrays stay in HBM until the next nwd_assign or nwd_set_amplicons (nwd_gather and
 * nwd_adopt_group leave them alone).  The result is a function of the input alone.  Synchronous. */
int nwd_pack(nwd_ctx* c, int64_t* group_offsets, int64_t* order, int64_t* text_offsets, uint16_t* lens,
             int64_t* group_exc, int64_t* n_exc, float* kernel_ms);

/* The last nwd_pack's stream and exception list copied to the HOST (for tests): packed [cap]
 * bytes, exc_pos int64 [n_exc], exc_byte uint8 [n_exc] (each may be NULL).  *needed (may be NULL)
 * = (text_offsets[n_assigned] + 3) / 4; a shorter cap is NW_E_CAPACITY with *needed written and
 * nothing copied.  NW_E_STATE before nwd_pack. */
int nwd_fetch_packed(nwd_ctx* c, uint8_t* packed, int64_t cap, int64_t* exc_pos, uint8_t* exc_byte, int64_t* needed);

/* Makes group g of the last nwd_pack the resident batch of the aligner context `ctx`, as
 * nw_batch_upload_packed would from the host: the group's lengths, its slice of the exception
 * list and its part of the shared stream are copied device to device on ctx's stream, behind the
 * packer.  Nothing crosses PCIe but the group's few group-base offsets.  ctx needs a reference
 * and NW_OUT_OPS (else NW_E_STATE, as nw_batch_upload_packed) and must be on this context's
 * device (NW_E_INVALID).  g outside [0, n_refs) or a group without reads is NW_E_INVALID; a call
 * before nwd_pack NW_E_STATE.  A refusal leaves both contexts as they were.  Adopting a group
 * does not change the packed arrays: groups may be adopted in any order, any number of times. */
int nwd_adopt_group(nwd_ctx* c, struct nw_ctx* ctx, int64_t g);

/* Reads of the last nwd_assign with more distinct candidates than the tally holds: they were
 * decided by the exact path on the host (the same rule). */
int64_t nwd_last_fallback(const nwd_ctx* c);

/* Times of the last nwd_assign, summed over its chunks: ms[0] device ms of the assign kernel,
 * ms[1] the host's wall ms in the chunks' uploads; ms[2] device ms of the last index build,
 * ms[3] of the last gather kernel.  A diagnostic (scripts/bench_demux.py). */
int nwd_phase_times(const nwd_ctx* c, float* ms);

#ifdef __cplusplus
}
#endif
#endif
