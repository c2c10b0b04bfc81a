/* crispr_ingest.h -- C ABI of the MI355X FASTQ ingest with qualities: the text of a FASTQ(.gz)
 * file to dense bases, qualities and names in HBM, where the front end (crispr_front.h,
 * nwp_prepare_records) reads them.
 *
 * CRISPResso hands its raw files to Trimmomatic (CRISPResso/CRISPRessoCORE.py:1585-1640) and
 * FLASH (CORE:1655-1677); this package's front end read them with flash.read_fastq, an
 * interpreter pass.  The records here are exactly what that reader returns, plus per-record
 * flags it never computes:
 *
 *   file     gzip if its first two bytes are 1f 8b, else the bytes are the text.
 *   lines    the pieces between '\n' bytes; an empty final piece is not a line.  With T bytes of
 *            text, L = count('\n') + (0 if T == 0 or the last byte is '\n' else 1).
 *   records  n = L / 4; record r is lines 4r .. 4r+3; the L % 4 lines after the last whole
 *            record are ignored and reported (trailing_lines).
 *   '\r'     header, sequence and quality line each lose all their trailing '\r' bytes
 *            (rstrip(b"\r")); a '\r' elsewhere stays.
 *   fields   name: the stripped header without its first byte (empty for an empty header);
 *            seq, qual: the stripped lines.
 *   flags    one byte a record: NWI_BAD_HEADER the header is empty or does not start with '@';
 *            NWI_BAD_PLUS line 2 is empty or does not start with '+'; NWI_LEN_MISMATCH
 *            len(seq) != len(qual); NWI_BAD_QUAL a byte of qual lies outside 33..126.
 *
 * The binding is crispresso_amd/ingest.py (ctypes); the kernels are crispresso_amd/csrc/fastq_parse.hip.
 */
#ifndef CRISPR_INGEST_H
#define CRISPR_INGEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { NWI_BAD_HEADER = 1, NWI_BAD_PLUS = 2, NWI_LEN_MISMATCH = 4, NWI_BAD_QUAL = 8 };

/* One parsed text: its streams and offsets stay in HBM until nwi_release. */
typedef struct nwi_records nwi_records;

typedef struct nwi_summary {
    int64_t n;               /* records */
    int64_t lines;           /* L */
    int64_t trailing_lines;  /* L % 4 */
    int64_t lmax;            /* the longest seq */
    int64_t flagged[4];      /* records with NWI_BAD_HEADER, NWI_BAD_PLUS, NWI_LEN_MISMATCH, NWI_BAD_QUAL */
    int64_t first_bad;       /* the smallest flagged record index, or -1 */
    int64_t seq_bytes, qual_bytes, name_bytes;   /* the three streams' sizes */
    int64_t text_bytes;      /* T */
    float upload_ms;         /* the text's copy to the device, by events */
    float kernel_ms;         /* the kernels, by events */
    float inflate_ms;        /* nwi_parse_file on a gzip file: the inflate (host clock); else 0 */
} nwi_summary;

/* Parses `bytes` bytes of FASTQ text in host memory on `device`.  Returns 0, -1 invalid arguments,
 * -3 unsupported (2^32 - 16 bytes of text or more, or more than 2^31 lines, in one call: such
 * files are out of scope and are refused, never truncated), -4 HIP error; nwi_last_error()
 * describes it. */
int nwi_parse_text(int device, const uint8_t* text, int64_t bytes, nwi_records** out);

/* Maps the file.  A gzip file is inflated (every member, concatenated; bytes after the last member
 * that do not start a member are ignored, as gzread does; a damaged or truncated member is an
 * error (-1), never partial data), then parsed as nwi_parse_text.  -1 also when the file cannot
 * be read. */
int nwi_parse_file(int device, const char* path, nwi_records** out);

/* The per-call results. */
int nwi_info(const nwi_records* r, nwi_summary* out);

/* Copies into caller-owned host arrays; any pointer may be NULL.  flags [n]; seq [seq_bytes],
 * seq_off [n + 1] from 0; qual, qual_off and names, name_off likewise.  With no flag set,
 * seq_off and qual_off are equal. */
int nwi_fetch(const nwi_records* r, uint8_t* flags, uint8_t* seq, int64_t* seq_off, uint8_t* qual, int64_t* qual_off,
              uint8_t* names, int64_t* name_off);

/* Frees the records' device arrays (NULL: nothing). */
void nwi_release(nwi_records* r);

/* Message of the last failed nwi_* call in this thread. */
const char* nwi_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
