// nw_summary.hip -- the end of the pooled amplicon mode on a resident group (gfx950): the
// identity filter and the UNMODIFIED flag from the aligner's records (for a row with an
// Expected_HDR amplicon: from the records of both passes, with the HDR and MIXED flags), and the
// 16 counters of SAMPLES_QUANTIFICATION_SUMMARY.txt from the quantifier's per-read results, behind
// the C ABI of include/crispr_summary.h.  Nothing per read crosses PCIe.
//
// The kernels run on the context's stream:
//   flags    one lane per nw_stat record (two 16-byte loads).  keep and pre are two compares of
//            n_ident with the threshold tables at aln_len; the tables are the host's (the printed
//            "%.1f" identity is never redone here).  An aln_len outside the tables is counted:
//            ballot and popcount, one 64-bit add per wavefront that saw one.
//   summary  a block of 256 lanes walks the records in steps of the grid; a lane loads its
//            nwq_read as one 16-byte word.  Each of the 15 predicates is a ballot and a popcount,
//            summed over the walk in the wavefront's own (uniform) registers; the four
//            wavefronts' sums meet in LDS and lanes 0..14 add the block's non-zero sums to the
//            counters, one 64-bit integer atomic per counter per block.  Integer sums: the result
//            does not depend on the order of arrival.
//   printed  one lane per nw_stat record: the PRINTED identity float("%.1f" % (100 n_ident /
//            aln_len)) in tenths, as a uint16.  t, r = divmod(1000 n_ident, aln_len) in 32-bit
//            integers; t + 1 when 2 r > aln_len; on a rounding midpoint (2 r == aln_len, rare)
//            one bit of the host's 1000-bit table, 128 bytes in HBM, read only then.
//   dual     one lane per read of a row with an Expected_HDR amplicon: the ref record's tenths by
//            the same function, the HDR pass's stored tenths, then CORE:1849-1856, 536-548 and
//            2014 as integer compares.
//   mask     one lane per read: pre of a dropped read becomes NWQ_PRE_UNMODIFIED, so that the
//            quantifier, which skips such a read before any total, counts kept reads only.
//   hist     the summary's walk; the sizes n_inserted, n_deleted, n_mutated and n_inserted -
//            n_deleted of a kept read go to the block's low bins in LDS (integer LDS atomics),
//            the rare larger ones straight to the 64-bit counters; at the end the block adds its
//            non-zero low bins to the counters, one 64-bit integer atomic each.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/crispr_nw.h"
#include "../../include/crispr_quant.h"
#include "../../include/crispr_summary.h"
#include "host_dev.h"

namespace nws {

constexpr int kBlk = 256;
constexpr int kWaves = kBlk / 64;
constexpr int64_t kMaxBlocks = 2048;      // of the summary's walk: 8 blocks a compute unit

struct FlagArgs {
    const int4* stats;          // [2 n]: nw_stat as two 16-byte words
    int64_t n;
    const int32_t* keep_min;    // [max_cols + 1]
    const int32_t* unmod_min;
    int32_t max_cols;
    uint8_t* pre;
    uint8_t* keep;
    unsigned long long* bad;    // [1]
};

__global__ __launch_bounds__(kBlk) void nws_flags_kernel(const FlagArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    bool outside = false;
    if (r < a.n) {
        const int4 lo = a.stats[2 * r], hi = a.stats[2 * r + 1];
        const int32_t aln_len = lo.x, n_ident = lo.y, flags = hi.w;
        outside = aln_len < 0 || aln_len > a.max_cols;
        uint8_t keep = 0, pre = 0;
        if (!outside) {
            keep = !(flags & NW_FLAG_EMPTY) && n_ident >= a.keep_min[aln_len];
            pre = n_ident >= a.unmod_min[aln_len] ? NWQ_PRE_UNMODIFIED : 0;
        }
        a.keep[r] = keep;
        a.pre[r] = pre;
    }
    const unsigned long long ob = __ballot(outside);
    if (lane == 0 && ob) atomicAdd(a.bad, (unsigned long long)__popcll(ob));
}

// The printed identity of n_ident / aln_len in tenths (0 .. 1000): what "%.1f" prints of the
// double 100.0 * n_ident / aln_len.  0 < aln_len <= NWS_MAX_COLS and 0 <= n_ident <= aln_len, so
// 1000 n_ident < 2^30.  Away from a midpoint the rational lies at least 1 / (20 aln_len) from it
// and the double's error (about 1e-14) cannot move it across; on a midpoint the double is the
// correctly rounded (2 t + 1) / 20, whose printing depends on t alone: tie_up's bit t.
__device__ __forceinline__ uint32_t printed_tenths(uint32_t n_ident, uint32_t aln_len, const uint32_t* tie_up) {
    const uint32_t x = 1000u * n_ident;
    uint32_t t = x / aln_len;
    const uint32_t r2 = 2u * (x - t * aln_len);
    if (r2 > aln_len) {
        ++t;
    } else if (r2 == aln_len) {         // (t <= 999 here: r > 0)
        t += (tie_up[t >> 5] >> (t & 31)) & 1u;
    }
    return t;
}

// One record's tenths: kNoTenths for an EMPTY record, `outside` set (and kNoTenths) for one whose
// aln_len or n_ident is out of range, 0 for aln_len == 0 (as aligner.printed_percent).
constexpr uint32_t kNoTenths = 0xFFFFu;

__device__ __forceinline__ uint32_t record_tenths(const int4* stats, int64_t r, const uint32_t* tie_up, bool& empty,
                                                  bool& outside) {
    const int4 lo = stats[2 * r], hi = stats[2 * r + 1];
    const int32_t aln_len = lo.x, n_ident = lo.y;
    empty = (hi.w & NW_FLAG_EMPTY) != 0;
    outside = aln_len < 0 || aln_len > NWS_MAX_COLS || n_ident < 0 || n_ident > aln_len;
    if (outside) return kNoTenths;
    return aln_len == 0 ? 0u : printed_tenths((uint32_t)n_ident, (uint32_t)aln_len, tie_up);
}

struct PrintedArgs {
    const int4* stats;          // [2 n]
    int64_t n;
    const uint32_t* tie_up;     // [32]: 1000 bits
    uint16_t* tenths;           // [n]
    unsigned long long* bad;    // [1]
};

__global__ __launch_bounds__(kBlk) void nws_printed_kernel(const PrintedArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    bool outside = false;
    if (r < a.n) {
        bool empty;
        const uint32_t t = record_tenths(a.stats, r, a.tie_up, empty, outside);
        a.tenths[r] = (uint16_t)(empty ? kNoTenths : t);
    }
    const unsigned long long ob = __ballot(outside);
    if (lane == 0 && ob) atomicAdd(a.bad, (unsigned long long)__popcll(ob));
}

struct DualArgs {
    const int4* stats;          // [2 n]: the records of the pass against the amplicon
    const uint16_t* rep;        // [n]: nws_printed of the pass against the Expected_HDR amplicon
    int64_t n;
    const uint32_t* tie_up;
    uint32_t keep_tenths, hdr_tenths;
    uint8_t* pre;
    uint8_t* keep;
    unsigned long long* bad;
};

__global__ __launch_bounds__(kBlk) void nws_flags_dual_kernel(const DualArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    bool outside = false;
    if (r < a.n) {
        bool empty;
        const uint32_t ref = record_tenths(a.stats, r, a.tie_up, empty, outside);
        const uint32_t rep = a.rep[r];
        const bool has_rep = rep <= 1000u;          // kNoTenths: no repaired score, every test on it is false
        outside = outside || (!has_rep && rep != kNoTenths);
        uint8_t keep = 0, pre = 0;
        if (!outside) {
            keep = !empty && (ref >= a.keep_tenths || (has_rep && rep >= a.keep_tenths));
            if (ref == 1000u) pre = NWQ_PRE_UNMODIFIED;
            if (has_rep && ref < rep) pre |= rep >= a.hdr_tenths ? NWQ_PRE_HDR : NWQ_PRE_MIXED;
        }
        a.keep[r] = keep;
        a.pre[r] = pre;
    }
    const unsigned long long ob = __ballot(outside);
    if (lane == 0 && ob) atomicAdd(a.bad, (unsigned long long)__popcll(ob));
}

struct SumArgs {
    const int4* reads;          // [n] nwq_read: cls, n_mutated, n_inserted, n_deleted
    const uint8_t* pre;
    const uint8_t* keep;
    int64_t n;
    unsigned long long* counters;   // [NWS_SLOTS], zeroed
};

__global__ __launch_bounds__(kBlk) void nws_summary_kernel(const SumArgs a) {
    __shared__ uint32_t part[kWaves][NWS_SLOTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t sum[NWS_SLOTS] = {};       // uniform in the wavefront; slot 0 is the host's
    const int64_t step = (int64_t)gridDim.x * kBlk;
    // (the same trip count in every lane of the block: at most n / step + 1 < 2^32 / 64 rounds)
    for (int64_t base = (int64_t)blockIdx.x * kBlk; base < a.n; base += step) {
        const int64_t r = base + threadIdx.x;
        bool kept = false, unmod = false;
        int4 q = make_int4(0, 0, 0, 0);
        if (r < a.n) {
            kept = a.keep[r] != 0;
            unmod = (a.pre[r] & NWQ_PRE_UNMODIFIED) != 0;
            q = a.reads[r];
        }
        const int cls = q.x;
        const bool mut = q.y > 0, ins = q.z > 0, del = q.w > 0;
        auto count = [&](int slot, bool p) { sum[slot] += (uint32_t)__popcll(__ballot(kept && p)); };
        count(NWS_TOTAL, true);
        count(NWS_UNMODIFIED, unmod || cls == 0);
        count(NWS_MODIFIED, cls == 1);
        count(NWS_REPAIRED, cls == 2);
        count(NWS_MIXED, cls == 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) {       // NHEJ, HDR, MIXED
            count(NWS_NHEJ_INSERTED + 3 * k, cls == k + 1 && ins);
            count(NWS_NHEJ_DELETED + 3 * k, cls == k + 1 && del);
            count(NWS_NHEJ_MUTATED + 3 * k, cls == k + 1 && mut);
        }
        count(NWS_NOT_ALIGNED, cls < 0);
    }
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NWS_SLOTS; ++s) part[wave][s] = sum[s];
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x < NWS_SLOTS) {
        unsigned long long t = 0;
        for (int w = 0; w < kWaves; ++w) t += part[w][threadIdx.x];
        if (t) atomicAdd(&a.counters[threadIdx.x], t);
    }
}

struct MaskArgs {
    const uint8_t* pre;
    const uint8_t* keep;
    int64_t n;
    uint8_t* pre_q;             // may be pre itself: a lane reads and writes its own byte only
};

__global__ __launch_bounds__(kBlk) void nws_mask_pre_kernel(const MaskArgs a) {
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r < a.n) {
        const uint8_t pre = a.pre[r];
        a.pre_q[r] = a.keep[r] ? pre : (uint8_t)NWQ_PRE_UNMODIFIED;
    }
}

// The low bins of the four histograms a block keeps in LDS: sizes 0 .. kLow - 1 of n_inserted,
// n_deleted and n_mutated, and n_inserted - n_deleted in (-kLow, kLow).
constexpr int kLow = 128;
constexpr int kLowIndel = 2 * kLow - 1;
constexpr int kLowBins = 3 * kLow + kLowIndel;

struct HistArgs {
    const int4* reads;          // [n] nwq_read: cls, n_mutated, n_inserted, n_deleted
    const uint8_t* keep;
    int64_t n;
    int32_t bins;
    unsigned long long* hist;   // [5 bins - 1]: ins, del, mut [bins] each, indel [2 bins - 1]; then bad [1].  Zeroed.
};

__global__ __launch_bounds__(kBlk) void nws_histograms_kernel(const HistArgs a) {
    __shared__ uint32_t low[kLowBins];  // a block counts at most n / gridDim.x + kBlk < 2^32 reads
    for (int i = threadIdx.x; i < kLowBins; i += kBlk) low[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int bins = a.bins;
    unsigned long long* const g_indel = a.hist + 3 * (int64_t)bins;
    uint32_t nbad = 0;                  // uniform in the wavefront
    const int64_t step = (int64_t)gridDim.x * kBlk;
    for (int64_t base = (int64_t)blockIdx.x * kBlk; base < a.n; base += step) {
        const int64_t r = base + threadIdx.x;
        bool counted = false;
        int4 q = make_int4(0, 0, 0, 0);
        if (r < a.n) {
            q = a.reads[r];
            counted = a.keep[r] != 0 && q.x >= 0;
        }
        const unsigned ub = (unsigned)bins;     // (a negative value is a large unsigned one)
        const bool outside = counted && ((unsigned)q.y >= ub || (unsigned)q.z >= ub || (unsigned)q.w >= ub);
        if (counted && !outside) {
            // 0 <= v < bins: the LDS bin when v < kLow, else the global counter which * bins + v
            auto bump = [&](int which, int v) {
                if (v < kLow) atomicAdd(&low[which * kLow + v], 1u);
                else atomicAdd(&a.hist[which * (int64_t)bins + v], 1ull);
            };
            bump(0, q.z);
            bump(1, q.w);
            bump(2, q.y);
            const int d = q.z - q.w;            // -bins < d < bins
            if (d > -kLow && d < kLow) atomicAdd(&low[3 * kLow + d + kLow - 1], 1u);
            else atomicAdd(&g_indel[d + bins - 1], 1ull);
        }
        nbad += (uint32_t)__popcll(__ballot(outside));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kLowBins; i += kBlk) {
        const uint32_t v = low[i];
        if (!v) continue;
        if (i < 3 * kLow) {
            const int which = i / kLow, bin = i % kLow;
            if (bin < bins) atomicAdd(&a.hist[which * (int64_t)bins + bin], (unsigned long long)v);
        } else {
            const int d = i - 3 * kLow - (kLow - 1);
            if (d > -bins && d < bins) atomicAdd(&g_indel[d + bins - 1], (unsigned long long)v);
        }
    }
    if (lane == 0 && nbad) atomicAdd(a.hist + 5 * (int64_t)bins - 1, (unsigned long long)nbad);
}

}  // namespace nws

struct nws_ctx : hd::DevContext {
    hd::DevBuf<unsigned long long> d_hist;     // nws_histograms: [5 bins - 1] and the bad count
    int32_t max_cols = -1;         // -1: no tables yet
    hd::DevBuf<int32_t> d_keep_min, d_unmod_min;
    hd::DevBuf<unsigned long long> d_counters;
    bool printed = false;          // nws_set_printed succeeded
    hd::DevBuf<uint32_t> d_tie_up; // [32]
    int32_t keep_tenths = 0, hdr_tenths = 0;
};

// The shared tail of the one-lane-per-record calls: the bad-record count back, the kernel's time.
static int finish_counted(nws_ctx* c, int64_t* n_bad, float* kernel_ms, unsigned long long* bad) {
    hipStream_t st = c->stream;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipMemcpyAsync(bad, c->d_counters.p, sizeof *bad, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    if (kernel_ms) *kernel_ms = ms;
    if (n_bad) *n_bad = (int64_t)*bad;
    return NW_OK;
}

using hd::fail;

extern "C" {

int nws_create(int device, nws_ctx** out) { return hd::create_context(device, 2, out); }

void nws_destroy(nws_ctx* c) { hd::destroy_context(c); }

const char* nws_last_error(const nws_ctx* c) { return c ? c->err.c_str() : "null context"; }

int nws_set_identity(nws_ctx* c, const int32_t* keep_min, const int32_t* unmod_min, int32_t max_cols) {
    if (!c) return NW_E_INVALID;
    if (!keep_min || !unmod_min) return fail(c, NW_E_INVALID, "null table");
    if (max_cols < 0 || max_cols > NWS_MAX_COLS)
        return fail(c, NW_E_UNSUPPORTED, "max_cols %d: 0 to %d are supported", (int)max_cols, NWS_MAX_COLS);
    c->max_cols = -1;               // no tables until this call succeeds
    const size_t len = (size_t)max_cols + 1;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_keep_min.reserve(len));
    HIP_TRY(c, c->d_unmod_min.reserve(len));
    HIP_TRY(c, hipMemcpyAsync(c->d_keep_min.p, keep_min, sizeof(int32_t) * len, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_unmod_min.p, unmod_min, sizeof(int32_t) * len, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->max_cols = max_cols;
    return NW_OK;
}

int nws_flags(nws_ctx* c, const void* d_stats, int64_t n, uint8_t* d_pre, uint8_t* d_keep, int64_t* n_out_of_range,
              float* kernel_ms) {
    if (!c) return NW_E_INVALID;
    if (n_out_of_range) *n_out_of_range = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (c->max_cols < 0) return fail(c, NW_E_STATE, "nws_flags before nws_set_identity");
    if (n < 0 || n > 0x7FFFFFFFll) return fail(c, NW_E_INVALID, "record count %lld out of range", (long long)n);
    if (n == 0) return NW_OK;
    if (!d_stats || !d_pre || !d_keep) return fail(c, NW_E_INVALID, "null device array");
    if ((uintptr_t)d_stats % 16) return fail(c, NW_E_INVALID, "the records are not 16-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(c, c->d_counters.reserve(NWS_SLOTS));
    HIP_TRY(c, hipMemsetAsync(c->d_counters.p, 0, sizeof(unsigned long long), st));
    nws::FlagArgs a{};
    a.stats = (const int4*)d_stats;
    a.n = n;
    a.keep_min = c->d_keep_min.p;
    a.unmod_min = c->d_unmod_min.p;
    a.max_cols = c->max_cols;
    a.pre = d_pre;
    a.keep = d_keep;
    a.bad = c->d_counters.p;
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(nws::nws_flags_kernel, dim3((unsigned)((n + nws::kBlk - 1) / nws::kBlk)), dim3(nws::kBlk), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    unsigned long long bad = 0;
    HIP_TRY(c, hipMemcpyAsync(&bad, c->d_counters.p, sizeof bad, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    if (kernel_ms) *kernel_ms = ms;
    if (n_out_of_range) *n_out_of_range = (int64_t)bad;
    if (bad)
        return fail(c, NW_E_INVALID, "%llu records with an alignment length outside [0, %d]", bad, (int)c->max_cols);
    return NW_OK;
}

int nws_set_printed(nws_ctx* c, const uint8_t* tie_up, int32_t keep_tenths, int32_t hdr_tenths) {
    if (!c) return NW_E_INVALID;
    if (!tie_up) return fail(c, NW_E_INVALID, "null table");
    if (keep_tenths < 0 || keep_tenths > 1001 || hdr_tenths < 0 || hdr_tenths > 1001)
        return fail(c, NW_E_INVALID, "thresholds %d and %d: tenths from 0 to 1001", (int)keep_tenths, (int)hdr_tenths);
    uint32_t bits[32] = {};
    for (int t = 0; t < 1000; ++t) {
        if (tie_up[t] > 1) return fail(c, NW_E_INVALID, "tie_up[%d] = %d: 0 or 1", t, (int)tie_up[t]);
        bits[t >> 5] |= (uint32_t)tie_up[t] << (t & 31);
    }
    c->printed = false;             // no tables until this call succeeds
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_tie_up.reserve(32));
    HIP_TRY(c, hipMemcpyAsync(c->d_tie_up.p, bits, sizeof bits, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->keep_tenths = keep_tenths;
    c->hdr_tenths = hdr_tenths;
    c->printed = true;
    return NW_OK;
}

int nws_printed(nws_ctx* c, const void* d_stats, int64_t n, uint16_t* d_tenths, int64_t* n_out_of_range,
                float* kernel_ms) {
    if (!c) return NW_E_INVALID;
    if (n_out_of_range) *n_out_of_range = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (!c->printed) return fail(c, NW_E_STATE, "nws_printed before nws_set_printed");
    if (n < 0 || n > 0x7FFFFFFFll) return fail(c, NW_E_INVALID, "record count %lld out of range", (long long)n);
    if (n == 0) return NW_OK;
    if (!d_stats || !d_tenths) return fail(c, NW_E_INVALID, "null device array");
    if ((uintptr_t)d_stats % 16) return fail(c, NW_E_INVALID, "the records are not 16-byte aligned");
    if ((uintptr_t)d_tenths % 2) return fail(c, NW_E_INVALID, "the tenths are not 2-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(c, c->d_counters.reserve(NWS_SLOTS));
    HIP_TRY(c, hipMemsetAsync(c->d_counters.p, 0, sizeof(unsigned long long), st));
    nws::PrintedArgs a{};
    a.stats = (const int4*)d_stats;
    a.n = n;
    a.tie_up = c->d_tie_up.p;
    a.tenths = d_tenths;
    a.bad = c->d_counters.p;
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(nws::nws_printed_kernel, dim3((unsigned)((n + nws::kBlk - 1) / nws::kBlk)), dim3(nws::kBlk), 0, st, a);
    unsigned long long bad = 0;
    if (int rc = finish_counted(c, n_out_of_range, kernel_ms, &bad)) return rc;
    if (bad)
        return fail(c, NW_E_INVALID, "%llu records with an alignment length outside [0, %d] or identities outside it",
                    bad, NWS_MAX_COLS);
    return NW_OK;
}

int nws_flags_dual(nws_ctx* c, const void* d_stats_ref, const uint16_t* d_tenths_rep, int64_t n, uint8_t* d_pre,
                   uint8_t* d_keep, int64_t* n_out_of_range, float* kernel_ms) {
    if (!c) return NW_E_INVALID;
    if (n_out_of_range) *n_out_of_range = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (!c->printed) return fail(c, NW_E_STATE, "nws_flags_dual before nws_set_printed");
    if (n < 0 || n > 0x7FFFFFFFll) return fail(c, NW_E_INVALID, "record count %lld out of range", (long long)n);
    if (n == 0) return NW_OK;
    if (!d_stats_ref || !d_tenths_rep || !d_pre || !d_keep) return fail(c, NW_E_INVALID, "null device array");
    if ((uintptr_t)d_stats_ref % 16) return fail(c, NW_E_INVALID, "the records are not 16-byte aligned");
    if ((uintptr_t)d_tenths_rep % 2) return fail(c, NW_E_INVALID, "the tenths are not 2-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(c, c->d_counters.reserve(NWS_SLOTS));
    HIP_TRY(c, hipMemsetAsync(c->d_counters.p, 0, sizeof(unsigned long long), st));
    nws::DualArgs a{};
    a.stats = (const int4*)d_stats_ref;
    a.rep = d_tenths_rep;
    a.n = n;
    a.tie_up = c->d_tie_up.p;
    a.keep_tenths = (uint32_t)c->keep_tenths;
    a.hdr_tenths = (uint32_t)c->hdr_tenths;
    a.pre = d_pre;
    a.keep = d_keep;
    a.bad = c->d_counters.p;
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(nws::nws_flags_dual_kernel, dim3((unsigned)((n + nws::kBlk - 1) / nws::kBlk)), dim3(nws::kBlk), 0, st,
                       a);
    unsigned long long bad = 0;
    if (int rc = finish_counted(c, n_out_of_range, kernel_ms, &bad)) return rc;
    if (bad)
        return fail(c, NW_E_INVALID, "%llu reads with a record or stored tenths out of range", bad);
    return NW_OK;
}

int nws_summary(nws_ctx* c, const void* d_reads, const uint8_t* d_pre, const uint8_t* d_keep, int64_t n, int64_t* out,
                float* kernel_ms) {
    if (!c) return NW_E_INVALID;
    if (!out) return fail(c, NW_E_INVALID, "null output");
    std::memset(out, 0, sizeof(int64_t) * NWS_SLOTS);
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n < 0 || n > 0x7FFFFFFFll) return fail(c, NW_E_INVALID, "read count %lld out of range", (long long)n);
    if (n == 0) return NW_OK;
    if (!d_reads || !d_pre || !d_keep) return fail(c, NW_E_INVALID, "null device array");
    if ((uintptr_t)d_reads % 16) return fail(c, NW_E_INVALID, "the reads' results are not 16-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(c, c->d_counters.reserve(NWS_SLOTS));
    HIP_TRY(c, hipMemsetAsync(c->d_counters.p, 0, sizeof(unsigned long long) * NWS_SLOTS, st));
    nws::SumArgs a{};
    a.reads = (const int4*)d_reads;
    a.pre = d_pre;
    a.keep = d_keep;
    a.n = n;
    a.counters = c->d_counters.p;
    const int64_t blocks = std::min<int64_t>((n + nws::kBlk - 1) / nws::kBlk, nws::kMaxBlocks);
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(nws::nws_summary_kernel, dim3((unsigned)blocks), dim3(nws::kBlk), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    unsigned long long ctr[NWS_SLOTS] = {};
    HIP_TRY(c, hipMemcpyAsync(ctr, c->d_counters.p, sizeof ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    if (kernel_ms) *kernel_ms = ms;
    for (int s = 1; s < NWS_SLOTS; ++s) out[s] = (int64_t)ctr[s];
    out[NWS_N] = n;
    return NW_OK;
}

int nws_mask_pre(nws_ctx* c, const uint8_t* d_pre, const uint8_t* d_keep, int64_t n, uint8_t* d_pre_q,
                 float* kernel_ms) {
    if (!c) return NW_E_INVALID;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n < 0 || n > 0x7FFFFFFFll) return fail(c, NW_E_INVALID, "read count %lld out of range", (long long)n);
    if (n == 0) return NW_OK;
    if (!d_pre || !d_keep || !d_pre_q) return fail(c, NW_E_INVALID, "null device array");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    nws::MaskArgs a{};
    a.pre = d_pre;
    a.keep = d_keep;
    a.n = n;
    a.pre_q = d_pre_q;
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(nws::nws_mask_pre_kernel, dim3((unsigned)((n + nws::kBlk - 1) / nws::kBlk)), dim3(nws::kBlk), 0, st,
                       a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    if (kernel_ms) *kernel_ms = ms;
    return NW_OK;
}

int nws_histograms(nws_ctx* c, const void* d_reads, const uint8_t* d_keep, int64_t n, int32_t bins, int64_t* out,
                   int64_t* n_out_of_range, float* kernel_ms) {
    if (!c) return NW_E_INVALID;
    if (n_out_of_range) *n_out_of_range = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (bins < 1 || bins > NWS_MAX_BINS)
        return fail(c, NW_E_UNSUPPORTED, "%d bins: 1 to %d are supported", (int)bins, NWS_MAX_BINS);
    if (!out) return fail(c, NW_E_INVALID, "null output");
    const size_t words = 5 * (size_t)bins - 1;
    std::memset(out, 0, sizeof(int64_t) * words);
    if (n < 0 || n > 0x7FFFFFFFll) return fail(c, NW_E_INVALID, "read count %lld out of range", (long long)n);
    if (n == 0) return NW_OK;
    if (!d_reads || !d_keep) return fail(c, NW_E_INVALID, "null device array");
    if ((uintptr_t)d_reads % 16) return fail(c, NW_E_INVALID, "the reads' results are not 16-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(c, c->d_hist.reserve(words + 1));
    HIP_TRY(c, hipMemsetAsync(c->d_hist.p, 0, sizeof(unsigned long long) * (words + 1), st));
    nws::HistArgs a{};
    a.reads = (const int4*)d_reads;
    a.keep = d_keep;
    a.n = n;
    a.bins = bins;
    a.hist = c->d_hist.p;
    const int64_t blocks = std::min<int64_t>((n + nws::kBlk - 1) / nws::kBlk, nws::kMaxBlocks);
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(nws::nws_histograms_kernel, dim3((unsigned)blocks), dim3(nws::kBlk), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    unsigned long long bad = 0;
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counters are copied as they are");
    HIP_TRY(c, hipMemcpyAsync(out, c->d_hist.p, sizeof(int64_t) * words, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&bad, c->d_hist.p + words, sizeof bad, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    if (kernel_ms) *kernel_ms = ms;
    if (n_out_of_range) *n_out_of_range = (int64_t)bad;
    if (bad)
        return fail(c, NW_E_INVALID, "%llu counted reads with a size outside [0, %d)", bad, (int)bins);
    return NW_OK;
}

}  // extern "C"
