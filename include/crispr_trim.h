/* crispr_trim.h -- C ABI of the MI355X read trimming (Trimmomatic 0.33: ILLUMINACLIP, MINLEN,
 * and through nwt_trim_program the quality and crop steps).
 *
 * CRISPResso trims paired-end reads with the external Trimmomatic program before the
 * merge when --trim_sequences is given (CRISPResso/CRISPRessoCORE.py:1620-1640):
 *
 *     java -jar trimmomatic-0.33.jar PE -phred33 R1 R2 fp fu rp ru ILLUMINACLIP:<fa>:0:90:10:0:true MINLEN:40
 *
 * nwt_trim_batch clips a batch of read pairs on the GPU with the algorithm the
 * test-infrastructure restatement oracle/trimmomatic_oracle.py states (IlluminaClip.process,
 * ClipSeq.compare / quality, maximum_range, PrefixPair.compare / quality, _cut and the
 * MINLEN step of run_pe), float32 sums included.  Clipping only ever truncates a read at
 * its 3' end, so the result is one length per read; no bases are copied.  The binding
 * is crispresso_amd/trim.py (ctypes), whose run_trimmomatic_pe() writes Trimmomatic's
 * four output files.  nwt_trim_program runs the same clip and then the other steps of a
 * --trimmomatic_options_string (nwt_step below) on the same device buffers; its result is
 * one window (start, length) per read.
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

/* One step of a Trimmomatic program after the optional ILLUMINACLIP (tests/trim_steps_model.py
 * restates them).  A record is a window (start, len) of its read, or
 * dropped; q[i] is the phred-33 quality of base i of the window, 0 where the base is 'N'
 * (zeroN: LEADING, TRAILING, SLIDINGWINDOW, AVGQUAL).
 *   LEADING:t        first i with q[i] >= t -> (start + i, len - i); none: dropped
 *   TRAILING:t       last i >= 1 with q[i] >= t -> (start, i + 1); none: dropped (index 0 is never tested)
 *   SLIDINGWINDOW:w:r  len < w: dropped; the first window of w bases whose total is below
 *                    R = float32(r) * float32(w): the first one drops the read, window j >= 1 cuts it to
 *                    j + w - 1; then bases with (float)q < r are walked back from the end, down to one base
 *   CROP:n           len >= n -> (start, n)
 *   HEADCROP:n       len <= n: dropped, else (start + n, len - n)
 *   AVGQUAL:t        sum(q) < t * len: dropped
 *   MINLEN:n         len < n: dropped */
enum { NWT_OP_LEADING = 1, NWT_OP_TRAILING = 2, NWT_OP_SLIDINGWINDOW = 3, NWT_OP_CROP = 4, NWT_OP_HEADCROP = 5,
       NWT_OP_AVGQUAL = 6, NWT_OP_MINLEN = 7 };
enum { NWT_MAX_STEPS = 16, NWT_MAX_STEP_ARG = 1 << 20, NWT_MAX_STEP_QUAL = 1000 };

typedef struct nwt_step {
    int32_t op;  /* NWT_OP_* */
    int32_t arg; /* t, n, or SLIDINGWINDOW's w (>= 1) */
    float r;     /* SLIDINGWINDOW's required quality, 0 otherwise */
    float R;     /* r * w as a float32 product */
} nwt_step;

/* ILLUMINACLIP (optional) followed by up to NWT_MAX_STEPS steps, on n reads or read pairs.
 * clip == NULL: no ILLUMINACLIP (the adapter and prefix arguments are unused); otherwise as
 * nwt_trim_batch, and clip->minlen must be 0 (MINLEN is a step here).  Reads, adapters and
 * prefixes as nwt_trim_batch; seq2 == NULL: single-end (start2 / keep2 unused).
 *
 * One upload; the clip kernel (when clip is given), then the steps kernel on the same device
 * buffers.  Output: read i survives as seq[start[i] .. start[i] + keep[i]); keep[i] = -1 (and
 * start[i] = 0): dropped.  A read ILLUMINACLIP clips to nothing is dropped; an empty read enters
 * the steps as the live (0, 0).  kernel_ms (may be NULL) receives two device times: the clip
 * kernel's (0 without clip) and the steps kernel's.  Error codes as nwt_trim_batch; more than
 * NWT_MAX_STEPS steps, an unknown op, an argument above NWT_MAX_STEP_ARG, a quality threshold
 * above NWT_MAX_STEP_QUAL and SLIDINGWINDOW with w = 0 or a negative or non-finite r are -1. */
int nwt_trim_program(int device, const nwt_params* clip, const uint8_t* adapters, const int32_t* adapter_off,
                     const int32_t* adapter_role, int32_t n_adapters, const uint8_t* prefixes,
                     const int32_t* prefix_off, int32_t n_prefix_pairs, const nwt_step* steps, int32_t n_steps,
                     const uint8_t* seq1, const uint8_t* qual1, const int64_t* off1, const uint8_t* seq2,
                     const uint8_t* qual2, const int64_t* off2, int64_t n, int32_t* start1, int32_t* keep1,
                     int32_t* start2, int32_t* keep2, float* kernel_ms);

/* Message of the last failed nwt_trim_batch / nwt_trim_program call in this thread. */
const char* nwt_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
