/* crispr_count.h -- C ABI of the MI355X sgRNA counting.
 *
 * Replaces the per-read loop of CRISPRessoCount (CRISPResso/CRISPRessoCountCORE.py:320-347):
 * str.find of the tracrRNA, the slice before it, a dict increment.  Per read s of n bytes and
 * a pattern T of m bytes:
 *
 *   idx   = the smallest p in [0, n - m] with s[p .. p + m) == T (case-sensitive), else the
 *           read counts in the read total and nowhere else;
 *   guide = s[idx - L : idx] under Python's slice rule: st = idx - L; if st < 0 then
 *           st = max(0, st + n); guide = s[st .. idx) when st < idx, else the empty key.
 *
 * Without a whitelist every guide is a key and the groups come in order of first appearance
 * (the dict's insertion order); with one, a guide counts only when it is a key, and every
 * distinct key is returned in the order of its first line, the zero counts too.
 *
 * The result is a function of the input alone (no atomic ordering shows in it).  The binding a
 * maintainer adds is crispresso_amd/count.py (ctypes).  Error codes are the NW_E_* of
 * include/crispr_nw.h.
 */
#ifndef CRISPR_COUNT_H
#define CRISPR_COUNT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nwc_ctx nwc_ctx;

#define NWC_MAX_PATTERN 128
#define NWC_MAX_GUIDE 64

/* Read here, so that tests reach the edges on small inputs:
 *   CRISPR_NWC_CHUNK=<reads>   reads per chunk (default: chunks of about 64 MiB of text);
 *   CRISPR_NWC_HASH_BITS=k     (0..64, default 64) only the low k bits of every key's hash are
 *                              kept (before the hash is forced nonzero): probe chains and the
 *                              collided path. */
int nwc_create(int device, nwc_ctx** out);
void nwc_destroy(nwc_ctx* c);
const char* nwc_last_error(const nwc_ctx* c);

/* Counts the guides of n reads held in HOST memory: read r = reads[offsets[r] .. offsets[r + 1]),
 * offsets int64 [n + 1] ascending, 0 <= n <= 2^31 - 1, every read shorter than 2^31 bytes.
 * pattern: m bytes, 1 <= m <= NWC_MAX_PATTERN; 0 <= guide_length <= NWC_MAX_GUIDE; anything
 * else is NW_E_UNSUPPORTED.  The whitelist is n_wl >= 0 keys, key k = wl_bytes[wl_offsets[k] ..
 * wl_offsets[k + 1]) (duplicates collapse onto their first position; a key longer than
 * guide_length stays at zero); n_wl < 0: no whitelist.
 *
 * Per-read outputs (HOST, may be NULL): pos int32 [n] = idx or -1; group_of_read int32 [n] = the
 * index of the read's group in the returned order, -1 when the read is not counted.
 * *n_found = reads with idx >= 0; *n_counted = reads counted in a group.
 *
 * Groups: first / count int64 [cap] (first = the group's smallest read index, increasing; -1
 * for every whitelist key), key_offsets int64 [cap + 1] into key_bytes [key_cap].
 * *n_groups and *n_key_bytes are what the result needs; when cap or key_cap is short the call
 * returns NW_E_CAPACITY with everything but the groups written, and nwc_fetch_groups hands the
 * groups out without a second count.  n == 0 gives zero groups (with a whitelist: its keys, all
 * zero) without touching the GPU.  kernel_ms (may be NULL): device time of the call's kernels.
 * Synchronous. */
int nwc_count(nwc_ctx* c, const uint8_t* reads, const int64_t* offsets, int64_t n, const uint8_t* pattern,
              int32_t m, int32_t guide_length, const uint8_t* wl_bytes, const int64_t* wl_offsets, int64_t n_wl,
              int64_t* first, int64_t* count, int64_t* key_offsets, uint8_t* key_bytes, int64_t cap,
              int64_t key_cap, int32_t* pos, int32_t* group_of_read, int64_t* n_groups, int64_t* n_key_bytes,
              int64_t* n_found, int64_t* n_counted, float* kernel_ms);

/* The groups of the last nwc_count of this context (kept until the next call). */
int nwc_fetch_groups(const nwc_ctx* c, int64_t* first, int64_t* count, int64_t* key_offsets, uint8_t* key_bytes,
                     int64_t cap, int64_t key_cap);

/* Reads of the last nwc_count whose key differed from the key their hash's slot holds (equal
 * hashes, different guides): they were taken off the counts and grouped exactly on the host.
 * Always 0 with a whitelist (that path compares the key before it counts). */
int64_t nwc_last_collided(const nwc_ctx* c);

/* Times of the last nwc_count, summed over its chunks: device ms of ms[0] find, ms[1] insert,
 * ms[2] publish, ms[3] verify (or the whitelist lookup), ms[4] the group compaction; ms[5] the
 * host's wall ms in the chunks' uploads.  A diagnostic (scripts/bench_count.py). */
int nwc_phase_times(const nwc_ctx* c, float* ms);

#ifdef __cplusplus
}
#endif
#endif
