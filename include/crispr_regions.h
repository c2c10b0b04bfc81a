/* crispr_regions.h -- C ABI of the MI355X BAM-to-target reads: a BAM's records become the reads
 * of every target region (CRISPRessoWGS), of every reference (CRISPRessoPooled, amplicon mode) or
 * of every region the records themselves span (CRISPRessoPooled, genome mode: nwr_discover below).
 *
 * Replaces the per-read loop of write_trimmed_fastq / get_reference_positions
 * (CRISPResso/CRISPRessoWGSCORE.py:166-221) and the `samtools view -F 4 | awk` demultiplex of
 * CRISPRessoPooledCORE.py:870-878.
 *
 * The CIGAR walk gives every query base a reference position or none.  pos is BAM's pos + 1; in
 * the order of the ops:
 *   M           the next len query bases sit on pos, pos + 1, ...; pos += len
 *   I, S        the next len query bases sit on nothing
 *   D, N        pos += len
 *   H, P, =, X  nothing: neither side advances (the reference's regular expression cannot match
 *               '=' and its if-chain has no branch for X; NWR_EQX_AS_MATCH treats both as M)
 * A record hits region (ref_id, bpstart, bpend) iff flag & 4 == 0, its reference is ref_id, and
 * both bpstart and bpend are positions of one of its query bases.  st / en are the query indices
 * of bpstart / bpend (the positions increase strictly, so both are unique); the read is
 * seq[st:en] and qual[st:en] under Python's slice rule (cut to l_seq, empty when en <= st; an
 * empty read is still a hit).  A region's hits come in record order; regions may overlap or
 * repeat, each is independent.  With NWR_BY_REFERENCE every record with flag & 4 == 0 and
 * ref_id >= 0 goes to its reference's set whole (st = 0, en = l_seq).
 *
 * The one deliberate difference: a hit of a record without sequence (l_seq == 0) or without
 * qualities (first quality byte 0xFF), where SAM text has "*" and the reference slices the "*",
 * is dropped and counted in n_no_seq.
 *
 * Sequence bytes are "=ACMGRSVTWYHKDBN"[nibble] as stored (no strand handling), qualities are
 * stored + 33.  The result is a function of the input alone.  More than 65535 CIGAR ops (the CG
 * tag) are not looked up: the record is walked by the ops of its core CIGAR.  The binding is
 * crispresso_amd/regions.py (ctypes).  Error codes are the NW_E_* of include/crispr_nw.h.
 *
 * NWR_PACKED (nwr_extract and nwr_discover; combines freely with the other flags): the reads stay
 * in HBM as the aligner's batch.  Hits, st / en, region order, n_no_seq, n_hits, n_bytes and
 * nwr_fetch_regions with its stats are exactly what the same call without the flag gives; no
 * ASCII base and no quality is written to HBM or copied to the host, and nwr_fetch with a
 * non-NULL text or quals is NW_E_STATE (its other arrays are served as before).  The result owns,
 * in HBM and until nwr_release, what nw_pack_reads (include/crispr_nw.h) makes of the text /
 * text_offsets of the unflagged call, made straight from the BAM's 4-bit codes:
 *   the stream      base i in bits 2 (i % 4) of byte i / 4, A C T G = 0 1 2 3 (BAM codes 1 2 8 4),
 *                   defined up to byte (n_bytes + 3) / 4, bits past the end 0;
 *   the exceptions  ascending by position: every base whose BAM code is not 1, 2, 4 or 8, its byte
 *                   the upper-case letter of "=MRSVWYHKDBN", 0 bits in the stream;
 *   lens            uint16 per hit.
 * The order is the result's own: region-major, record order within a region, across all chunks
 * of the call.  A hit longer than 65535 bases, or 2^32 or more bases in the call, is
 * NW_E_UNSUPPORTED (the message names the record or the count).  The result stays valid after
 * nwr_destroy of the context that made it, and the context may run further calls while it lives.
 */
#ifndef CRISPR_REGIONS_H
#define CRISPR_REGIONS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nwr_ctx nwr_ctx;
typedef struct nwr_bam nwr_bam;

#define NWR_MAX_REGIONS (1 << 20)
#define NWR_BY_REFERENCE 1
#define NWR_EQX_AS_MATCH 2
#define NWR_PACKED 4

typedef struct nwr_region {
    int64_t bpstart, bpend; /* 1-based, as in SAM text and the reference's region file */
    int32_t ref_id;         /* index into the BAM's references; no record is on any other value */
    int32_t reserved;
} nwr_region;

typedef struct nwr_result {
    int64_t n_regions; /* the call's regions (NWR_BY_REFERENCE: the BAM's references) */
    int64_t n_hits;
    int64_t n_bytes;   /* bytes of text (and of quals) */
    int64_t n_no_seq;  /* hits dropped because their record has no sequence or no qualities */
    float kernel_ms;   /* device time of the call's kernels */
    float upload_ms;   /* host wall time in the chunks' uploads */
    void* handle;
} nwr_result;

/* Reads a BAM from `path`, or from the mem_len bytes at `mem` when path is NULL: BGZF (the blocks
 * inflated in parallel on the host's thread pool, each block's CRC-32 and size checked; the
 * empty EOF block is optional) or an already uncompressed BAM stream.  The header is parsed and
 * every record is validated: block_size >= 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 +
 * l_seq, the record ends inside the stream, -1 <= ref_id < n_ref.  Anything else (bad magic, a
 * truncated block, a CRC or size mismatch, a record past the end) is NW_E_INVALID with a message
 * in err (err_cap bytes, may be NULL); an unreadable path is NW_E_STATE.  Uses no GPU. */
int nwr_read_bam(const char* path, const uint8_t* mem, int64_t mem_len, nwr_bam** out, char* err, int64_t err_cap);
void nwr_bam_free(nwr_bam* b);
int64_t nwr_bam_count(const nwr_bam* b);
/* The uncompressed stream; record i is the bytes [offsets[i], offsets[i + 1]) of it, from its
 * block_size field on (offsets: int64 [count + 1]). */
const uint8_t* nwr_bam_data(const nwr_bam* b, int64_t* nbytes);
const int64_t* nwr_bam_offsets(const nwr_bam* b);
int32_t nwr_bam_n_ref(const nwr_bam* b);
/* The reference names, each ended by a NUL, one after the other; their lengths. */
const char* nwr_bam_ref_names(const nwr_bam* b, int64_t* nbytes);
const int32_t* nwr_bam_ref_lens(const nwr_bam* b);
const char* nwr_bam_text(const nwr_bam* b, int64_t* nbytes);

/* CRISPR_NWR_CHUNK=<records> is read here: records per chunk (default: chunks of about 256 MiB
 * of records), so that tests reach the chunk edges on small inputs. */
int nwr_create(int device, nwr_ctx** out);
void nwr_destroy(nwr_ctx* c);
const char* nwr_last_error(const nwr_ctx* c);

/* The reads of every region (n_regions <= NWR_MAX_REGIONS, any order; ignored with
 * NWR_BY_REFERENCE) from the records of `bam` (only a validated nwr_bam is ever uploaded).
 * flags: NWR_BY_REFERENCE, NWR_EQX_AS_MATCH.  The BAM is processed in chunks of whole records;
 * a chunk whose output reaches 2^32 bytes or 2^30 hits, or more regions than NWR_MAX_REGIONS,
 * is NW_E_UNSUPPORTED.  Fills *res; the result stays with res->handle until nwr_release.  Zero
 * records or zero regions give an empty result without touching the GPU.  Synchronous. */
int nwr_extract(nwr_ctx* c, const nwr_bam* bam, const nwr_region* regions, int64_t n_regions, int32_t flags,
                nwr_result* res);

/* Copies the result into the caller's arrays (any may be NULL): region_offsets int64
 * [n_regions + 1], the hits of region g (the caller's order) are [region_offsets[g],
 * region_offsets[g + 1]); per hit src int64 (the record's index in the BAM), st / en int32 (the
 * query indices before the cut to l_seq, saturated at 2^31 - 1); text_offsets int64 [n_hits + 1]
 * into text and quals (n_bytes each). */
int nwr_fetch(const nwr_result* res, int64_t* region_offsets, int64_t* src, int32_t* st, int32_t* en,
              int64_t* text_offsets, uint8_t* text, uint8_t* quals);
void nwr_release(nwr_result* res);

/* CRISPRessoPooled's genome mode (CRISPRessoPooledCORE.py:1045-1082: `samtools view -F 4 | awk |
 * sort | awk`): nobody names the regions, the records do.  A record takes part iff flag & 4 == 0,
 * ref_id >= 0 and it has a sequence and qualities.  Its span: pos is BAM's pos + 1, bpstart =
 * bpend = pos, then in the order of the ops
 *   S           bpstart -= len while bpend == pos (nothing has advanced yet, whatever H or I came
 *               before; every leading S does so), else bpend += len
 *   I, H        nothing
 *   M, D, N, P  bpend += len
 *   =, X and the op codes 9-15: the reference splits the CIGAR text on [MIDNSHP], so a maximal
 *               run of these ops and the op after it are one op to it: of the kind of the op
 *               after the run (M at the CIGAR's end), of the length of the run's first op; the
 *               other lengths are lost.  5=3X2M at 100 gives 100..105, 10M5= 100..115, 3S5=2M
 *               97..105.  With NWR_EQX_AS_MATCH, = and X are M and the codes 9-15 are nothing.
 * No CIGAR gives (pos, pos); bpstart may be zero or negative.  A region is a distinct (ref_id,
 * bpstart, bpend); the result's regions come in ascending (ref_id, bpstart, bpend), compared as
 * numbers, a region's reads in record order, whole (st = 0, en = l_seq), bases as stored.
 *
 * Three deliberate differences from the reference: (1) a record without sequence or qualities is
 * dropped and counted in n_no_seq (the reference writes its "*"); (2) a mapped record with ref_id
 * -1 is dropped (the reference writes a REGION_*_0_0 file for it); (3) the reads of a region come
 * in record order, where the reference has the order of `sort`'s last-resort comparison of whole
 * lines (strand, name, sequence, qualities, bytewise under the C locale, different under others);
 * crispresso_amd/regions.py restores that order on the host on request.
 *
 * min_reads: a region with at least min_reads records in the whole call has its reads emitted;
 * any other region is still reported by nwr_fetch_regions, with an empty range in
 * region_offsets (min_reads <= 0 emits all).  The only flag is NWR_EQX_AS_MATCH.  At most 2^30
 * records in a call and NWR_MAX_REGIONS regions *emitted* (any number reported), and the chunk
 * limits of nwr_extract, else NW_E_UNSUPPORTED; a full table (which the sizing rules out) is
 * NW_E_STATE.  CRISPR_NWR_HASH_BITS=k, read at nwr_create, keeps the low k bits of the key's hash,
 * so that tests reach long probe chains and distinct keys under one hash on small inputs.  The
 * result is served by nwr_fetch and nwr_release as above, and is a function of the input alone. */
int nwr_discover(nwr_ctx* c, const nwr_bam* bam, int32_t flags, int64_t min_reads, nwr_result* res);

/* After nwr_discover (NW_E_STATE after nwr_extract): regions [n_regions] the keys in result order,
 * n_records [n_regions] the records of each in the whole call, emitted or not; stats: n_aligned
 * (records with flag & 0x904 == 0, the reference's get_n_aligned_bam), the kept records, the
 * emitted regions, 0 (reserved).  Any pointer may be NULL. */
int nwr_fetch_regions(const nwr_result* res, nwr_region* regions, int64_t* n_records, int64_t stats[4]);

/* The packed batch of a result made with NWR_PACKED (NW_E_STATE on any other): lens uint16
 * [n_hits], region_exc int64 [n_regions + 1] (region g's exceptions are the slots region_exc[g] ..
 * region_exc[g + 1] of the list), their number, the packer's device time.  Any pointer may be
 * NULL. */
int nwr_packed_info(const nwr_result* res, uint16_t* lens, int64_t* region_exc, int64_t* n_exc, float* kernel_ms);

/* Copies the batch to the host (for tests): the (n_bytes + 3) / 4 bytes of the stream to packed
 * (cap bytes; *needed gets the size, NW_E_CAPACITY and nothing copied when cap is short), the
 * exception list to exc_pos / exc_byte (n_exc each).  Any pointer may be NULL. */
int nwr_fetch_packed(const nwr_result* res, uint8_t* packed, int64_t cap, int64_t* exc_pos, uint8_t* exc_byte, int64_t* needed);

/* Makes region g's reads the resident batch of the aligner context ctx, as nw_batch_upload_packed
 * of the same reads would: a device-to-device adoption of the region's slice on ctx's stream,
 * behind the packer's event; only the group-base offsets cross PCIe.  ctx needs a reference and
 * NW_OUT_OPS, else NW_E_STATE, as on a result made without NWR_PACKED; NW_E_INVALID for a context
 * on another device, g out of range or a region without hits.  A refusal changes nothing;
 * regions are adoptable in any order, any number of times.  A region whose hits are all empty
 * reads is adoptable: its records come out NW_FLAG_EMPTY.  The aligner's own errors are read with
 * nw_last_error(ctx). */
struct nw_ctx;
int nwr_adopt_region(const nwr_result* res, struct nw_ctx* ctx, int64_t g);

#ifdef __cplusplus
}
#endif
#endif
