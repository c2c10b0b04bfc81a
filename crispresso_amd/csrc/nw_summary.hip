// nw_summary.hip -- the end of the pooled amplicon mode on a resident group (gfx950): the
// identity filter and the UNMODIFIED flag from the aligner's records, and the 16 counters of
// SAMPLES_QUANTIFICATION_SUMMARY.txt from the quantifier's per-read results, behind the C ABI of
// include/crispr_summary.h.  Nothing per read crosses PCIe.
//
// Both kernels run on the context's stream:
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

}  // namespace nws

struct nws_ctx : hd::DevContext {
    int32_t max_cols = -1;         // -1: no tables yet
    hd::DevBuf<int32_t> d_keep_min, d_unmod_min;
    hd::DevBuf<unsigned long long> d_counters;
};

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

}  // extern "C"
