/* crispr_front.h -- C ABI of the MI355X read front end: raw reads to a resident aligner batch.
 *
 * CRISPResso filters reads by quality (CRISPResso/CRISPRessoCORE.py:162-308), trims them with
 * Trimmomatic (CORE:1585-1640), merges pairs with FLASH (CORE:1655-1677) and hands the merged
 * file to the aligner.  nwp_prepare is those steps in one call on one upload: the quality filter,
 * the clip and steps kernels of crispr_trim.h, the merge kernel of crispr_flash.h on the trimmed
 * windows, and a device packer that leaves the surviving reads in HBM as nw_pack_reads +
 * nw_batch_upload_packed (crispr_nw.h) would have: the context then runs nw_batch_run_async,
 * nw_batch_download_ops, nw_batch_device_ops with nothing uploaded in between.  nwp_prepare_records
 * is the same call on records the FASTQ ingest (crispr_ingest.h) already left in HBM.
 *
 * The binding is crispresso_amd/frontend.py (ctypes).
 */
#ifndef CRISPR_FRONT_H
#define CRISPR_FRONT_H

#include <stdint.h>

#include "crispr_flash.h"
#include "crispr_ingest.h"
#include "crispr_nw.h"
#include "crispr_trim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per input read (pair): what became of it.  Single-end survivors are NWP_COMBINED. */
enum { NWP_FILTERED = 0, NWP_TRIMMED = 1, NWP_NOT_COMBINED = 2, NWP_COMBINED = 3, NWP_COMBINED_OUTIE = 4 };

enum { NWP_MS_FILTER = 0, NWP_MS_CLIP = 1, NWP_MS_STEPS = 2, NWP_MS_MERGE = 3, NWP_MS_PACK = 4, NWP_MS_COUNT = 5 };

typedef struct nwp_params {
    /* The quality filter: a read is kept iff sum(q - 33) >= min_avg_quality * len and
     * min(q - 33) >= min_single_quality (integers: equal to the reference's float64 mean for
     * reads up to 4096 bases and thresholds up to 93); a pair iff both mates are.  Both <= 0:
     * no filter. */
    int32_t min_avg_quality;
    int32_t min_single_quality;
    /* The trim program, as nwt_trim_program's arguments: clip == NULL: no ILLUMINACLIP;
     * n_steps == 0 and no clip: no trim. */
    const nwt_params* clip;
    const uint8_t* adapters;
    const int32_t* adapter_off;
    const int32_t* adapter_role;
    int32_t n_adapters;
    const uint8_t* prefixes;
    const int32_t* prefix_off;
    int32_t n_prefix_pairs;
    const nwt_step* steps;
    int32_t n_steps;
    /* The merge (paired input only). */
    nwf_params flash;
    int32_t want_quals;  /* keep the dense qualities for nwp_fetch */
} nwp_params;

typedef struct nwp_result {
    int64_t n;        /* input reads (pairs) */
    int64_t m;        /* reads of the batch: the merged pairs, or the surviving single-end reads */
    int64_t total;    /* their bases */
    int64_t n_exc;    /* bytes other than A C G T a c g t among them */
    int64_t counts[5];            /* reads per NWP_* status */
    int64_t trim[4];              /* Trimmomatic's summary over the unfiltered pairs: both, forward only,
                                     reverse only, dropped (single-end: surviving, 0, 0, dropped) */
    float kernel_ms[NWP_MS_COUNT];
    void* handle;     /* the call's device arrays, for nwp_fetch; nwp_release frees them */
} nwp_result;

/* Reads as nwt_trim_program: pair i = seq1/qual1[off1[i] .. off1[i+1]) and seq2/qual2[off2[i] ..
 * off2[i+1]); seq2 == NULL: single-end (filter, trim, pack; no merge).  A pair is merged only if
 * the filter kept it and both mates survive the trim; the batch is the combined pairs in input
 * order (single-end: the surviving reads' windows, bytes as given).
 *
 * ctx must have a reference and NW_OUT_OPS (else NW_E_STATE, as nw_batch_upload_packed).  On
 * return the context holds the batch exactly as nw_batch_upload_packed(nw_pack_reads(text)) would
 * leave it (the copies are device-to-device on the context's stream, after an event recorded
 * behind the front end's kernels).  m == 0: the context's batch is untouched.
 *
 * Returns 0, NW_E_STATE, or -1 invalid arguments, -3 unsupported (a read longer than 4096, the
 * refusals of nwt_trim_program, 2^32 or more bytes of reads), -4 HIP error; nwp_last_error()
 * describes it (the context's nw_last_error for an error of the adoption). */
int nwp_prepare(nw_ctx* ctx, const nwp_params* params, const uint8_t* seq1, const uint8_t* qual1, const int64_t* off1,
                const uint8_t* seq2, const uint8_t* qual2, const int64_t* off2, int64_t n, nwp_result* out);

/* nwp_prepare on records the FASTQ ingest left on the context's device (crispr_ingest.h), with
 * nothing uploaded: the first n records of r1 (r2 == NULL: single-end), or the first
 * n = min(n1, n2) of each mate.  The records are only read, and only during the call.
 *
 * The ingest's results stand in for nwp_prepare's checks of the reads: -1 when a flag is set among
 * the records the call would use (the message names the first flagged record, its mate and the
 * reason), -3 when the longest sequence of either file exceeds 4096 bases.  Everything else is as
 * nwp_prepare. */
int nwp_prepare_records(nw_ctx* ctx, const nwp_params* params, const nwi_records* r1, const nwi_records* r2,
                        nwp_result* out);

/* Copies of the result into caller-owned host arrays; any pointer may be NULL.  status [n];
 * offsets [m + 1] from 0; lens [m]; src [m]: the input index of each batch read; text [total];
 * quals [total] (want_quals); packed [(total + 3) / 4]: byte-identical to nw_pack_reads on
 * (text, offsets); exc_pos / exc_byte [n_exc], ascending. */
int nwp_fetch(const nwp_result* res, uint8_t* status, int64_t* offsets, uint16_t* lens, int64_t* src, uint8_t* text,
              uint8_t* quals, uint8_t* packed, int64_t* exc_pos, uint8_t* exc_byte);

/* Frees the result's device arrays (the context keeps its batch). */
void nwp_release(nwp_result* res);

/* Message of the last failed nwp_* call in this thread. */
const char* nwp_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
