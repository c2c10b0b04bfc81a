/* crispr_trim.h -- C ABI of the MI355X adapter trimming (Trimmomatic 0.33 ILLUMINACLIP + MINLEN).
 *
 * CRISPResso trims paired-end reads with the external Trimmomatic program before the
 * merge when --trim_sequences is given (CRISPResso/CRISPRessoCORE.py:1620-1640):
 *
 *     java -jar trimmomatic-0.33.jar PE -phred33 R1 R2 fp fu rp ru ILLUMINACLIP:<fa>:0:90:10:0:true MINLEN:40
 *
 * This library call clips a batch of read pairs on the GPU with the algorithm the
 * test-infrastructure restatement oracle/trimmomatic_oracle.py states (IlluminaClip.process,
 * ClipSeq.compare / quality, maximum_range, PrefixPair.compare / quality, _cut and the
 * MINLEN step of run_pe), float32 sums included.  Clipping only ever truncates a read at
 * its 3' end, so the result is one length per read; no bases are copied.  The binding
 * is crispresso_amd/trim.py (ctypes), whose run_trimmomatic_pe() writes Trimmomatic's
 * four output files.
 *
 * Only Trimmomatic's "long" clipping class is implemented: a simple-mode adapter of
 * fewer than 24 bases is refused (-3).  The restatement states that class alone (the
 * short and medium classes seed differently and are pinned by nothing here).
 */
#ifndef CRISPR_TRIM_H
#define CRISPR_TRIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ILLUMINACLIP:<fasta>:<2>:<3>:<4>[:<5>[:<6>]] and MINLEN:<n>. */
typedef struct nwt_params {
    int32_t seed_mismatches;      /* ILLUMINACLIP field 2 */
    int32_t palindrome_threshold; /* field 3 */
    int32_t simple_threshold;     /* field 4 */
    int32_t min_prefix;           /* field 5, Trimmomatic's default 8 */
    int32_t keep_both;            /* field 6 */
    int32_t minlen;               /* MINLEN:n, 0 = none */
} nwt_params;

enum { NWT_MAX_READ = 4096, NWT_MAX_ADAPTER = 128, NWT_MAX_ADAPTERS = 16, NWT_MAX_PREFIX_PAIRS = 4,
       NWT_MIN_SIMPLE_ADAPTER = 24 };

/* Clip n read pairs.  Pair i: read 1 = seq1/qual1[off1[i] .. off1[i+1]), read 2 =
 * seq2/qual2[off2[i] .. off2[i+1]) (as in the FASTQ files; qualities are ASCII, phred 33).
 *
 * Simple-mode adapters: adapter a = adapters[adapter_off[a] .. adapter_off[a+1])
 * (adapter_off has n_adapters + 1 entries from 0), adapter_role[a] 0 = both reads,
 * 1 = read 1 only, 2 = read 2 only.  Palindrome prefix pairs: prefix k of pair p =
 * prefixes[prefix_off[2p+k] .. prefix_off[2p+k+1]) (2 * n_prefix_pairs + 1 offsets; p1, p2,
 * p1, p2, ...); the longer of a pair is cut to the other's length from its 3' end.
 * Bases are compared as given (the adapter FASTA reader upper-cases).
 *
 * seq2 == NULL: single-end (simple mode on read 1 only; qual2, off2 and keep2 are unused).
 *
 * Output (caller-owned host buffers): keep1[i], keep2[i] = the bases of each read that
 * survive ILLUMINACLIP and MINLEN, 0 = the read is dropped.  kernel_ms (may be NULL)
 * receives the device time.  Returns 0, or a negative code (nwt_last_error() describes it):
 * -1 invalid arguments (a quality byte outside 33..126 included), -3 unsupported (a read
 * longer than 4096, an adapter or prefix longer than 128, more than 16 adapters, more
 * than 4 prefix pairs, a simple-mode adapter shorter than 24 bases), -4 HIP error. */
int nwt_trim_batch(int device, const nwt_params* params, const uint8_t* adapters, const int32_t* adapter_off,
                   const int32_t* adapter_role, int32_t n_adapters, const uint8_t* prefixes,
                   const int32_t* prefix_off, int32_t n_prefix_pairs, const uint8_t* seq1, const uint8_t* qual1,
                   const int64_t* off1, const uint8_t* seq2, const uint8_t* qual2, const int64_t* off2, int64_t n,
                   int32_t* keep1, int32_t* keep2, float* kernel_ms);

/* Message of the last failed nwt_trim_batch call in this thread. */
const char* nwt_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
