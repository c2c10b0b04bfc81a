// The read front end on gfx950 (include/crispr_front.h): raw reads to a resident aligner batch.
//
// nwp_prepare uploads the reads once and runs, on the null stream, the quality filter (here),
// the clip and steps kernels (trim_clip.hip, trim_steps.hip), the merge kernel on the trimmed
// windows (flash_merge.hip) and the packer (here), which is nw_pack_reads (nw_pack.cpp) on the
// device: the surviving reads' text made dense, their offsets / lengths / group offsets, the
// 2-bit stream and the exception list.  The context then takes the batch with device-to-device
// copies on its own stream behind an event (nw_front::set_packed_batch, nw_host.cpp).
// nwp_prepare_records is the same call on records the FASTQ ingest (fastq_parse.hip) left in HBM:
// nothing is uploaded, the kernels read the ingest's streams and offsets where they lie, and the
// ingest's flags and longest read stand in for the host's checks of the reads.
//
// The packer is block sums / one scan block / scatter, three launches with nothing handed between
// blocks inside a launch (no wait anywhere):
//   * nwp_count_kernel, 256 reads a block: a thread decides its read's status, length and source
//     position; each wave then walks its 64 reads 64 bytes at a time and counts the bytes that are
//     not A C G T a c g t (a ballot and a popcount a step).  The block's (reads, bytes, exceptions)
//     go to sums[]; the status counts to a few device counters (integer atomics: the order of the
//     additions does not matter).
//   * nwp_scan_kernel, one block: the exclusive scan of the block sums and the totals.
//   * nwp_scatter_kernel, 256 reads a block: the scan of the block's reads on top of the block's
//     base gives each surviving read its batch index, offset and first exception slot; the thread
//     writes offsets / lens / src (and every 1024th offset); the waves copy the text (and the
//     qualities) into the dense buffers and write the exceptions in order: the slot of an
//     exception is its read's base + the exceptions before it in the read (ballot prefix).
//   * nwp_words_kernel, a thread a dword of the 2-bit stream: 16 dense bytes (one aligned 16-B
//     load) to 32 bits; an exception or a position past the batch's end gives 0 bits.  Every
//     dword is written once, whole, from the reads that cover it: no zeroed buffer, no partial
//     stores.  It reads 16 B for the 4 B it writes.
// Sums are 32-bit: a call with 2^32 or more bytes of reads is refused.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/crispr_front.h"
#include "flash_device.h"
#include "front_device.h"
#include "ingest_device.h"
#include "nw_device.h"
#include "trim_device.h"

namespace nwp {

constexpr int kBlk = 256;        // reads per block of the count and scatter kernels
constexpr int kScanBlk = 1024;   // threads of the scan block
constexpr int kWpb = 4;

// the counters the count kernel adds to
enum { kCntStatus = 0, kCntTrim = 5, kCounters = 9 };

__device__ __forceinline__ bool is_acgt(uint8_t b) {   // nw_pack.cpp's
    const uint8_t u = b & 0xDF;
    return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}

// ---- the quality filter ---------------------------------------------------------------------

struct FilterArgs {
    const uint8_t* qual[2];
    const int64_t* off[2];
    int64_t n;
    int32_t paired, min_avg, min_single;
    uint8_t* live;
};

// One wavefront per read (pair): sum and minimum of q - 33 over each mate.
__global__ __launch_bounds__(64 * kWpb) void nwp_filter_kernel(const FilterArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t p = (int64_t)blockIdx.x * kWpb + wave; p < a.n; p += (int64_t)gridDim.x * kWpb) {
        bool keep = true;
        for (int mate = 0; mate < (a.paired ? 2 : 1); ++mate) {
            const int64_t o = a.off[mate][p];
            const int len = (int)(a.off[mate][p + 1] - o);
            int sum = 0, mn = INT_MAX;
            for (int k = lane; k < len; k += 64) {
                const int q = (int)a.qual[mate][o + k] - 33;
                sum += q;
                mn = min(mn, q);
            }
            for (int s = 32; s > 0; s >>= 1) {
                sum += __shfl_xor(sum, s);
                mn = min(mn, __shfl_xor(mn, s));
            }
            keep = keep && (int64_t)sum >= (int64_t)a.min_avg * len && mn >= a.min_single;
        }
        if (lane == 0) a.live[p] = keep ? 1 : 0;
    }
}

// ---- the packer -----------------------------------------------------------------------------

// Where the batch's reads are before the packer: the merge kernel's sparse slots (paired), or the
// uploaded reads' windows (single-end).
struct PackSrc {
    const int64_t* off1;
    const int64_t* off2;      // null: single-end
    const uint8_t* text;      // paired: the merged bases; single-end: the uploaded reads
    const uint8_t* qual;
    const int32_t* mlen;      // paired: the merge's lengths and flags
    const int32_t* mflags;
    const int32_t* start1;    // the trim's windows, or null (all four)
    const int32_t* keep1;
    const int32_t* keep2;
    const uint8_t* live;      // the filter's verdicts, or null
    int64_t n;
};

struct ReadAt {
    int status, len;
    int64_t pos;   // of its first byte in src.text
    bool alive;
};

__device__ __forceinline__ ReadAt read_at(const PackSrc& s, int64_t i) {
    ReadAt r{NWP_FILTERED, 0, 0, false};
    const bool paired = s.off2 != nullptr;
    if (s.live && !s.live[i]) return r;
    if (s.keep1 && (s.keep1[i] < 0 || (paired && s.keep2[i] < 0))) {
        r.status = NWP_TRIMMED;
        return r;
    }
    if (paired) {
        const int f = s.mflags[i];
        if (!(f & NWF_COMBINED)) {
            r.status = NWP_NOT_COMBINED;
            return r;
        }
        r.status = (f & NWF_OUTIE) ? NWP_COMBINED_OUTIE : NWP_COMBINED;
        r.len = s.mlen[i];
        r.pos = s.off1[i] + s.off2[i];
    } else {
        r.status = NWP_COMBINED;
        r.len = s.keep1 ? s.keep1[i] : (int)(s.off1[i + 1] - s.off1[i]);
        r.pos = s.off1[i] + (s.keep1 ? s.start1[i] : 0);
    }
    r.alive = true;
    return r;
}

struct PackArgs {
    PackSrc s;
    uint8_t* status;           // [n]
    int32_t* nexc;             // [n] exceptions of each read
    uint32_t* sums;            // [3 * blocks]: reads, bytes, exceptions of each block, then their bases
    unsigned long long* counters;   // [kCounters]
    int64_t* totals;           // [3]: m, bytes, exceptions
    int64_t blocks;
    // the batch
    int64_t* offsets;          // [m + 1]
    uint16_t* lens;            // [m]
    int64_t* src;              // [m]
    int64_t* gbase;            // [m / kLenGroup + 1]
    uint8_t* text;             // dense
    uint8_t* quals;            // dense, or null
    int64_t* exc_pos;
    uint8_t* exc_byte;
    uint32_t* words;           // the 2-bit stream
};

__device__ __forceinline__ void count_to(unsigned long long* c, bool pred, int lane) {
    const uint64_t b = __ballot(pred);
    if (b && lane == 0) atomicAdd(c, (unsigned long long)__builtin_popcountll(b));
}

__global__ __launch_bounds__(kBlk) void nwp_count_kernel(const PackArgs a) {
    __shared__ uint32_t part[kBlk / 64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    const bool in = i < a.s.n;
    ReadAt r{NWP_FILTERED, 0, 0, false};
    if (in) {
        r = read_at(a.s, i);
        a.status[i] = (uint8_t)r.status;
    }
    for (int st = 0; st < 5; ++st) count_to(a.counters + kCntStatus + st, in && r.status == st, lane);
    if (a.s.keep1) {   // Trimmomatic's summary, over the reads the filter kept
        const bool seen = in && r.status != NWP_FILTERED;
        const bool k1 = seen && a.s.keep1[i] >= 0, k2 = seen && a.s.off2 && a.s.keep2[i] >= 0;
        const bool pe = a.s.off2 != nullptr;
        count_to(a.counters + kCntTrim + 0, seen && k1 && (k2 || !pe), lane);
        count_to(a.counters + kCntTrim + 1, seen && pe && k1 && !k2, lane);
        count_to(a.counters + kCntTrim + 2, seen && pe && !k1 && k2, lane);
        count_to(a.counters + kCntTrim + 3, seen && !k1 && !k2, lane);
    }
    // the wave's 64 reads, one after the other: bytes that are exceptions
    int mine = 0;
    for (int t = 0; t < 64; ++t) {
        const int len = __shfl(r.alive ? r.len : 0, t);
        if (len == 0) continue;   // uniform
        const int64_t pos = ((int64_t)__shfl((int)(r.pos >> 32), t) << 32) | (uint32_t)__shfl((int)r.pos, t);
        int cnt = 0;
        for (int k0 = 0; k0 < len; k0 += 64) {
            const int k = k0 + lane;
            const bool exc = k < len && !is_acgt(a.s.text[pos + k]);
            cnt += __builtin_popcountll(__ballot(exc));
        }
        if (lane == t) mine = cnt;
    }
    if (in) a.nexc[i] = mine;
    uint32_t v0 = r.alive ? 1u : 0u, v1 = r.alive ? (uint32_t)r.len : 0u, v2 = (uint32_t)mine;
    for (int s = 32; s > 0; s >>= 1) {
        v0 += __shfl_xor(v0, s);
        v1 += __shfl_xor(v1, s);
        v2 += __shfl_xor(v2, s);
    }
    if (lane == 0) part[wave][0] = v0, part[wave][1] = v1, part[wave][2] = v2;
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t s = 0;
        for (int w = 0; w < kBlk / 64; ++w) s += part[w][threadIdx.x];
        a.sums[3 * (int64_t)blockIdx.x + threadIdx.x] = s;
    }
}

// One block: sums[3 b + q] becomes the exclusive prefix over the blocks before b; the totals.
__global__ __launch_bounds__(kScanBlk) void nwp_scan_kernel(const PackArgs a) {
    __shared__ uint32_t sh[2][kScanBlk];
    const int t = threadIdx.x;
    const int64_t per = (a.blocks + kScanBlk - 1) / kScanBlk;
    const int64_t lo = std::min<int64_t>(a.blocks, t * per), hi = std::min<int64_t>(a.blocks, lo + per);
    for (int q = 0; q < 3; ++q) {
        uint32_t mine = 0;
        for (int64_t b = lo; b < hi; ++b) mine += a.sums[3 * b + q];
        int cur = 0;
        sh[0][t] = mine;
        __syncthreads();
        for (int d = 1; d < kScanBlk; d <<= 1) {   // inclusive scan of the threads' sums
            sh[cur ^ 1][t] = sh[cur][t] + (t >= d ? sh[cur][t - d] : 0u);
            cur ^= 1;
            __syncthreads();
        }
        uint32_t run = sh[cur][t] - mine;
        if (t == kScanBlk - 1) a.totals[q] = (int64_t)sh[cur][t];
        for (int64_t b = lo; b < hi; ++b) {
            const uint32_t v = a.sums[3 * b + q];
            a.sums[3 * b + q] = run;
            run += v;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlk) void nwp_scatter_kernel(const PackArgs a) {
    __shared__ uint32_t part[kBlk / 64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    const bool in = i < a.s.n;
    ReadAt r{NWP_FILTERED, 0, 0, false};
    int ne = 0;
    if (in) {
        r = read_at(a.s, i);
        ne = a.nexc[i];
    }
    const uint32_t v[3] = {r.alive ? 1u : 0u, r.alive ? (uint32_t)r.len : 0u, (uint32_t)ne};
    uint32_t x[3] = {v[0], v[1], v[2]};
    for (int s = 1; s < 64; s <<= 1)
        for (int q = 0; q < 3; ++q) {
            const uint32_t y = __shfl_up(x[q], s);
            if (lane >= s) x[q] += y;
        }
    if (lane == 63) part[wave][0] = x[0], part[wave][1] = x[1], part[wave][2] = x[2];
    __syncthreads();
    int64_t base[3];
    for (int q = 0; q < 3; ++q) {
        uint32_t b = a.sums[3 * (int64_t)blockIdx.x + q];
        for (int w = 0; w < wave; ++w) b += part[w][q];
        base[q] = (int64_t)(b + x[q] - v[q]);
    }
    const int64_t j = base[0], o = base[1];
    if (r.alive) {
        a.offsets[j] = o;
        a.lens[j] = (uint16_t)r.len;
        a.src[j] = i;
        if (j % nw::kLenGroup == 0) a.gbase[j / nw::kLenGroup] = o;
    }
    if (i == 0) {
        const int64_t m = a.totals[0], total = a.totals[1];
        a.offsets[m] = total;
        if (m % nw::kLenGroup == 0) a.gbase[m / nw::kLenGroup] = total;
    }
    // the wave's 64 reads, one after the other: dense text and qualities, the exceptions in order
    for (int t = 0; t < 64; ++t) {
        const int len = __shfl(r.alive ? r.len : 0, t);
        if (len == 0) continue;   // uniform
        const int64_t pos = ((int64_t)__shfl((int)(r.pos >> 32), t) << 32) | (uint32_t)__shfl((int)r.pos, t);
        const int64_t to = ((int64_t)__shfl((int)(o >> 32), t) << 32) | (uint32_t)__shfl((int)o, t);
        int64_t e = ((int64_t)__shfl((int)(base[2] >> 32), t) << 32) | (uint32_t)__shfl((int)base[2], t);
        for (int k0 = 0; k0 < len; k0 += 64) {
            const int k = k0 + lane;
            uint8_t c = 'A';
            if (k < len) {
                c = a.s.text[pos + k];
                a.text[to + k] = c;
                if (a.quals) a.quals[to + k] = a.s.qual[pos + k];
            }
            const bool exc = !is_acgt(c);
            const uint64_t bal = __ballot(exc);
            if (exc) {
                const int64_t slot = e + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
                a.exc_pos[slot] = to + k;
                a.exc_byte[slot] = c;
            }
            e += __builtin_popcountll(bal);
        }
    }
}

// words[w] from dense bytes 16 w .. 16 w + 15 (the dense buffer is 16-B aligned and padded to a
// multiple of 16 bytes; bytes at or past `total` are not part of the batch).
__global__ __launch_bounds__(256) void nwp_words_kernel(const uint8_t* text, int64_t total, uint32_t* words,
                                                        int64_t nwords) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    const uint4 d = *reinterpret_cast<const uint4*>(text + 16 * w);
    const uint32_t in[4] = {d.x, d.y, d.z, d.w};
    const int64_t left = total - 16 * w;   // >= 1
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint8_t c = (uint8_t)(in[k >> 2] >> (8 * (k & 3)));
        if (k < left && is_acgt(c)) out |= (uint32_t)((c >> 1) & 3) << (2 * k);
    }
    words[w] = out;
}

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int fail_trim(int code) {   // a refusal of the trim path's shared checks: its message
    g_err = nwt_last_error();
    return code;
}

// A result's device arrays (nwp_result::handle) and the host copies the adoption needed.
struct Handle {
    nwt::Batch b;
    int device = 0;
    uint8_t* status = nullptr;
    int64_t* src = nullptr;
    uint8_t *text = nullptr, *quals = nullptr, *exc_byte = nullptr;
    uint32_t* words = nullptr;
    int64_t* exc_pos = nullptr;
    std::vector<int64_t> offsets;
    std::vector<uint16_t> lens;
};

}  // namespace nwp

extern "C" const char* nwp_last_error(void) { return nwp::g_err.c_str(); }

extern "C" void nwp_release(nwp_result* res) {
    if (!res || !res->handle) return;
    nwp::Handle* h = (nwp::Handle*)res->handle;
    (void)hipSetDevice(h->device);
    delete h;
    res->handle = nullptr;
}

extern "C" int nwp_fetch(const nwp_result* res, uint8_t* status, int64_t* offsets, uint16_t* lens, int64_t* src,
                         uint8_t* text, uint8_t* quals, uint8_t* packed, int64_t* exc_pos, uint8_t* exc_byte) {
    using namespace nwp;
    if (!res || !res->handle) return fail(-1, "nwp_fetch: no result");
    Handle* h = (Handle*)res->handle;
    if (quals && !h->quals && res->total > 0) return fail(-1, "nwp_fetch: the call did not keep the qualities (want_quals)");
    if (hipSetDevice(h->device) != hipSuccess) return fail(-4, "nwp_fetch: hipSetDevice failed");
    const size_t n = (size_t)res->n, m = (size_t)res->m, total = (size_t)res->total, ne = (size_t)res->n_exc;
    bool ok = true;
    auto get = [&](void* dst, const void* d, size_t bytes) {
        if (dst && bytes && ok) ok = hipMemcpy(dst, d, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    };
    get(status, h->status, n);
    if (offsets) memcpy(offsets, h->offsets.data(), 8 * (m + 1));
    if (lens && m) memcpy(lens, h->lens.data(), 2 * m);
    get(src, h->src, 8 * m);
    get(text, h->text, total);
    get(quals, h->quals, total);
    get(packed, h->words, (total + 3) / 4);
    get(exc_pos, h->exc_pos, 8 * ne);
    get(exc_byte, h->exc_byte, ne);
    if (!ok) return fail(-4, std::string("nwp_fetch: HIP error: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

int nw_front::view_prepared(const nwp_result* res, PreparedView* out) {
    if (!res || !res->handle || !out) return NW_E_INVALID;
    const nwp::Handle* h = (const nwp::Handle*)res->handle;
    const bool any = res->m > 0;
    *out = PreparedView{any ? h->text : nullptr, any ? h->quals : nullptr, h->offsets.data(), res->m, res->total,
                        h->device, any ? h->b.e1 : nullptr};
    return NW_OK;
}

namespace nwp {

// What both entries check before they look at the reads: the arguments, the context's state, the
// trim program.  reads_ok: the entry's own reads are all there.  On 0, *out holds an empty handle
// (all a call with n == 0 returns).
int begin_call(const char* who, nw_ctx* ctx, const nwp_params* params, bool paired, bool reads_ok, int64_t n,
               nwp_result* out, nwt::Program& P) {
    const std::string me = std::string(who) + ": ";
    if (!ctx || !params || !out || n < 0 || params->n_steps < 0 || (params->n_steps > 0 && !params->steps))
        return fail(-1, me + "null argument or negative count");
    memset(out, 0, sizeof(*out));
    int rc = nw_front::check_state(ctx);
    if (rc != NW_OK) return fail(rc, me + nw_last_error(ctx));
    if (params->clip) {
        rc = nwt::check_counts(who, params->adapters, params->adapter_off, params->adapter_role, params->n_adapters,
                               params->prefixes, params->prefix_off, params->n_prefix_pairs);
        if (rc != 0) return fail_trim(rc);
    }
    if (!reads_ok) return fail(-1, me + "null argument");
    if (paired && (params->flash.min_overlap < 1 || params->flash.max_overlap < 1))
        return fail(-1, me + "min_overlap and max_overlap must be >= 1");
    rc = nwt::program_check(who, params->clip, params->adapters, params->adapter_off, params->adapter_role,
                            params->n_adapters, params->prefixes, params->prefix_off, params->n_prefix_pairs,
                            params->steps, params->n_steps, P);
    if (rc != 0) return fail_trim(rc);
    out->n = n;
    Handle* h = new Handle;
    h->device = nw_front::device_of(ctx);
    h->offsets.assign(1, 0);
    out->handle = h;
    return 0;
}

// Everything after the reads are on the device: the batch of out's handle has s1 .. o2 (its own
// upload, or the ingest's arrays) and its events (Batch::begin); n > 0, t1 and t2 are the mates'
// bytes, lmax the longest read.  Filter, trim, merge, pack, and the context's adoption.
int run_call(const char* who, nw_ctx* ctx, const nwp_params* params, nwt::Program& P, bool paired, int64_t n, int lmax,
             int64_t t1, int64_t t2, nwp_result* out) {
    const std::string me = std::string(who) + ": ";
    Handle* h = (Handle*)out->handle;
    nwt::Batch& b = h->b;
    const bool trim = P.clip || P.sa.n_steps > 0;
    const bool filter = params->min_avg_quality > 0 || params->min_single_quality > 0;
    auto bail = [&](int code) {
        nwp_release(out);
        return code;
    };
    const int64_t blocks = (n + kBlk - 1) / kBlk;
    bool have = true;
    int32_t* d_win[4] = {nullptr, nullptr, nullptr, nullptr};   // start1, keep1, start2, keep2
    if (trim) have = nwt::program_alloc(b, P, n, d_win) && have;
    uint8_t* d_live = filter ? (uint8_t*)b.dev((size_t)n) : nullptr;
    uint8_t *d_ms = nullptr, *d_mq = nullptr;
    int32_t *d_mlen = nullptr, *d_mflg = nullptr;
    if (paired) {
        d_ms = (uint8_t*)b.dev((size_t)(t1 + t2) + 8);
        d_mq = (uint8_t*)b.dev((size_t)(t1 + t2) + 8);
        d_mlen = (int32_t*)b.dev(sizeof(int32_t) * n);
        d_mflg = (int32_t*)b.dev(sizeof(int32_t) * n);
        have = have && d_ms && d_mq && d_mlen && d_mflg;
    }
    PackArgs pa{};
    pa.status = h->status = (uint8_t*)b.dev((size_t)n);
    pa.nexc = (int32_t*)b.dev(sizeof(int32_t) * n);
    pa.sums = (uint32_t*)b.dev(sizeof(uint32_t) * 3 * blocks);
    pa.counters = (unsigned long long*)b.dev(sizeof(unsigned long long) * kCounters);
    pa.totals = (int64_t*)b.dev(sizeof(int64_t) * 3);
    pa.blocks = blocks;
    if (!have || (filter && !d_live) || !pa.status || !pa.nexc || !pa.sums || !pa.counters || !pa.totals)
        return bail(fail(-4, me + "hipMalloc failed"));

    auto hip_fail = [&]() {
        return bail(fail(-4, me + "HIP error: " + hipGetErrorString(hipGetLastError())));
    };
    float* ms = out->kernel_ms;
    if (filter) {
        FilterArgs fa{};
        fa.qual[0] = b.q1, fa.off[0] = b.o1, fa.qual[1] = b.q2, fa.off[1] = b.o2;
        fa.n = n, fa.paired = paired;
        fa.min_avg = params->min_avg_quality, fa.min_single = params->min_single_quality;
        fa.live = d_live;
        if (!b.begin()) return hip_fail();
        hipLaunchKernelGGL(nwp_filter_kernel, dim3(b.grid(n, kWpb)), dim3(64 * kWpb), 0, nullptr, fa);
        if (!b.elapsed(ms + NWP_MS_FILTER)) return hip_fail();
    }
    if (trim && !nwt::program_run(b, P, lmax, n, paired, d_win, ms + NWP_MS_CLIP)) return hip_fail();
    if (paired) {
        nwf::Args ma{};
        ma.seq1 = b.s1, ma.qual1 = b.q1, ma.off1 = b.o1;
        ma.seq2 = b.s2, ma.qual2 = b.q2, ma.off2 = b.o2;
        ma.n = n;
        ma.out_seq = d_ms, ma.out_qual = d_mq, ma.out_len = d_mlen, ma.out_flags = d_mflg;
        nwf::set_params(ma, &params->flash, lmax);
        ma.start1 = d_win[0], ma.keep1 = d_win[1], ma.start2 = d_win[2], ma.keep2 = d_win[3];
        ma.live = d_live;
        if (!b.begin()) return hip_fail();
        nwf::launch_merge(ma, b.grid(n, nwf::kWpb), nwf::merge_lds(ma), trim || filter);
        if (!b.elapsed(ms + NWP_MS_MERGE)) return hip_fail();
    }
    // the packer: count, scan, (sizes to the host), scatter, words
    pa.s.off1 = b.o1, pa.s.off2 = paired ? b.o2 : nullptr;
    pa.s.text = paired ? d_ms : b.s1, pa.s.qual = paired ? d_mq : b.q1;
    pa.s.mlen = d_mlen, pa.s.mflags = d_mflg;
    pa.s.start1 = d_win[0], pa.s.keep1 = d_win[1], pa.s.keep2 = d_win[3];
    pa.s.live = d_live;
    pa.s.n = n;
    float ms_a = 0.0f, ms_b = 0.0f;
    if (hipMemsetAsync(pa.counters, 0, sizeof(unsigned long long) * kCounters, nullptr) != hipSuccess || !b.begin())
        return hip_fail();
    hipLaunchKernelGGL(nwp_count_kernel, dim3((unsigned)blocks), dim3(kBlk), 0, nullptr, pa);
    hipLaunchKernelGGL(nwp_scan_kernel, dim3(1), dim3(kScanBlk), 0, nullptr, pa);
    if (!b.elapsed(&ms_a)) return hip_fail();
    int64_t tot[3];
    unsigned long long cnt[kCounters];
    if (hipMemcpy(tot, pa.totals, sizeof(tot), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(cnt, pa.counters, sizeof(cnt), hipMemcpyDeviceToHost) != hipSuccess)
        return hip_fail();
    const int64_t m = tot[0], total = tot[1], n_exc = tot[2];
    out->m = m, out->total = total, out->n_exc = n_exc;
    for (int k = 0; k < 5; ++k) out->counts[k] = (int64_t)cnt[kCntStatus + k];
    for (int k = 0; k < 4; ++k) out->trim[k] = (int64_t)cnt[kCntTrim + k];
    if (!trim) out->trim[0] = n - out->counts[NWP_FILTERED];
    h->offsets.assign((size_t)m + 1, 0);
    h->lens.assign((size_t)m, 0);
    if (m == 0) return 0;

    const int64_t nwords = (total + 15) / 16, ngroups = m / nw::kLenGroup + 1;
    pa.offsets = (int64_t*)b.dev(sizeof(int64_t) * (m + 1));
    pa.lens = (uint16_t*)b.dev(sizeof(uint16_t) * m);
    pa.src = h->src = (int64_t*)b.dev(sizeof(int64_t) * m);
    pa.gbase = (int64_t*)b.dev(sizeof(int64_t) * ngroups);
    pa.text = h->text = (uint8_t*)b.dev((size_t)(16 * nwords) + 16);
    pa.quals = h->quals = params->want_quals ? (uint8_t*)b.dev((size_t)total + 16) : nullptr;
    pa.exc_pos = h->exc_pos = (int64_t*)b.dev(sizeof(int64_t) * std::max<int64_t>(n_exc, 1));
    pa.exc_byte = h->exc_byte = (uint8_t*)b.dev((size_t)std::max<int64_t>(n_exc, 1));
    pa.words = h->words = (uint32_t*)b.dev(sizeof(uint32_t) * std::max<int64_t>(nwords, 1) + 64);
    if (!pa.offsets || !pa.lens || !pa.src || !pa.gbase || !pa.text || (params->want_quals && !pa.quals) ||
        !pa.exc_pos || !pa.exc_byte || !pa.words)
        return bail(fail(-4, me + "hipMalloc failed"));
    if (!b.begin()) return hip_fail();
    hipLaunchKernelGGL(nwp_scatter_kernel, dim3((unsigned)blocks), dim3(kBlk), 0, nullptr, pa);
    if (nwords > 0)
        hipLaunchKernelGGL(nwp_words_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, nullptr, pa.text,
                           total, pa.words, nwords);
    // b.e1 is recorded behind the packer on the null stream: the context's stream waits for it
    if (!b.elapsed(&ms_b)) return hip_fail();
    ms[NWP_MS_PACK] = ms_a + ms_b;
    if (hipMemcpy(h->offsets.data(), pa.offsets, sizeof(int64_t) * (m + 1), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(h->lens.data(), pa.lens, sizeof(uint16_t) * m, hipMemcpyDeviceToHost) != hipSuccess)
        return hip_fail();
    const nw_front::PackedSrc src{(const uint8_t*)pa.words, pa.lens, pa.gbase, pa.exc_pos, pa.exc_byte, true, b.e1};
    const int rc = nw_front::set_packed_batch(ctx, src, h->offsets.data(), h->lens.data(), m, n_exc);
    if (rc != NW_OK) return bail(fail(rc, me + nw_last_error(ctx)));
    return 0;
}

}  // namespace nwp

extern "C" int nwp_prepare(nw_ctx* ctx, const nwp_params* params, const uint8_t* seq1, const uint8_t* qual1,
                           const int64_t* off1, const uint8_t* seq2, const uint8_t* qual2, const int64_t* off2,
                           int64_t n, nwp_result* out) {
    using namespace nwp;
    const char* who = "nwp_prepare";
    const bool paired = seq2 != nullptr;
    nwt::Program P;
    const bool reads_ok = !(n > 0 && (!seq1 || !qual1 || !off1 || (paired && (!qual2 || !off2))));
    int rc = begin_call(who, ctx, params, paired, reads_ok, n, out, P);
    if (rc != 0 || n == 0) return rc;
    auto bail = [&](int code) {
        nwp_release(out);
        return code;
    };
    int lmax = 0;
    rc = nwt::check_reads(who, qual1, off1, qual2, off2, n, paired, &lmax);
    if (rc != 0) return bail(fail_trim(rc));
    const int64_t t1 = off1[n], t2 = paired ? off2[n] : 0;
    if ((uint64_t)t1 + (uint64_t)t2 >= (1ull << 32))
        return bail(fail(-3, "nwp_prepare: 2^32 or more bytes of reads in one call are not supported"));
    Handle* h = (Handle*)out->handle;
    if (hipSetDevice(h->device) != hipSuccess) return bail(fail(-4, "nwp_prepare: hipSetDevice failed"));
    if (!h->b.alloc_reads(t1, t2, n)) return bail(fail(-4, "nwp_prepare: hipMalloc failed"));
    if (!h->b.upload(h->device, seq1, qual1, off1, seq2, qual2, off2, n, paired))
        return bail(fail(-4, std::string("nwp_prepare: HIP error: ") + hipGetErrorString(hipGetLastError())));
    return run_call(who, ctx, params, P, paired, n, lmax, t1, t2, out);
}

extern "C" int nwp_prepare_records(nw_ctx* ctx, const nwp_params* params, const nwi_records* r1, const nwi_records* r2,
                                   nwp_result* out) {
    using namespace nwp;
    const char* who = "nwp_prepare_records";
    const bool paired = r2 != nullptr;
    const int64_t n = !r1 ? 0 : paired ? std::min(r1->info.n, r2->info.n) : r1->info.n;
    nwt::Program P;
    int rc = begin_call(who, ctx, params, paired, r1 != nullptr, n, out, P);
    if (rc != 0 || n == 0) return rc;
    auto bail = [&](int code) {
        nwp_release(out);
        return code;
    };
    Handle* h = (Handle*)out->handle;
    const nwi_records* mates[2] = {r1, r2};
    for (int k = 0; k < (paired ? 2 : 1); ++k)
        if (mates[k]->device != h->device)
            return bail(fail(-1, "nwp_prepare_records: the records lie on another device than the context"));
    if (hipSetDevice(h->device) != hipSuccess) return bail(fail(-4, "nwp_prepare_records: hipSetDevice failed"));
    auto hip_fail = [&]() {
        return bail(fail(-4, std::string("nwp_prepare_records: HIP error: ") + hipGetErrorString(hipGetLastError())));
    };
    // the two refusals nwt::check_reads makes on host arrays, from the ingest's own results
    int64_t t[2] = {0, 0};
    int64_t lmax = 0;
    for (int k = 0; k < (paired ? 2 : 1); ++k) {
        const nwi_records* r = mates[k];
        const int64_t bad = r->info.first_bad;
        if (bad >= 0 && bad < n) {   // first_bad is the smallest flagged index: none below it
            uint8_t f = 0;
            if (hipMemcpy(&f, r->flags + bad, 1, hipMemcpyDeviceToHost) != hipSuccess) return hip_fail();
            return bail(fail(-1, std::string("nwp_prepare_records: record ") + std::to_string(bad) + " of R" +
                                     std::to_string(k + 1) + ": " + nwi::flag_reason(f)));
        }
        lmax = std::max(lmax, r->info.lmax);
        // no flag among the first n: their base and quality offsets are equal
        if (hipMemcpy(&t[k], r->off[0] + n, sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) return hip_fail();
    }
    if (lmax > 4096)
        return bail(fail(-3, "nwp_prepare_records: a read longer than 4096 bases (" + std::to_string(lmax) +
                                 ") is not supported"));
    if ((uint64_t)t[0] + (uint64_t)t[1] >= (1ull << 32))
        return bail(fail(-3, "nwp_prepare_records: 2^32 or more bytes of reads in one call are not supported"));
    // the batch reads the records where the ingest left them (nothing copied; the kernels only read)
    nwt::Batch& b = h->b;
    b.s1 = r1->stream[0], b.q1 = r1->stream[1], b.o1 = r1->off[0];
    if (paired) {
        b.s2 = r2->stream[0], b.q2 = r2->stream[1], b.o2 = r2->off[0];
    } else {   // as alloc_reads leaves them
        b.s2 = (uint8_t*)b.dev(8), b.q2 = (uint8_t*)b.dev(8), b.o2 = (int64_t*)b.dev(sizeof(int64_t));
        if (!b.s2 || !b.q2 || !b.o2) return bail(fail(-4, "nwp_prepare_records: hipMalloc failed"));
    }
    b.set_launch_cap(h->device);
    return run_call(who, ctx, params, P, paired, n, (int)lmax, t[0], t[1], out);
}
