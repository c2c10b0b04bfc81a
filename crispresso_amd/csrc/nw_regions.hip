// nw_regions.hip -- BAM records to per-region reads (gfx950): the CIGAR walk and the slice of
// CRISPRessoWGS's write_trimmed_fastq (CRISPRessoWGSCORE.py:166-221) and the by-reference
// demultiplex of CRISPRessoPooled's amplicon mode (CRISPRessoPooledCORE.py:870-878), behind the
// C ABI of include/crispr_regions.h.  The records come validated from nw_bam.cpp: every field a
// kernel reads lies inside its record, so the kernels carry no per-byte bounds logic.
//
// A call runs its records in chunks of whole records; per chunk, on the context's stream:
//   count   a lane per record: the core fields bytewise (records are not aligned), one CIGAR walk
//           for the mapped span [first, end), a binary search of the region table (sorted by
//           reference and bpstart) for the regions with first <= bpstart < end, and a walk per
//           candidate for the query indices of bpstart and bpend.  The record's hits are counted,
//           the block's sum goes to sums[block].
//   scan    one block: the exclusive scan of the block sums.
//   write   the same walk again; every hit (region, record, st, en) lands at its scanned index,
//           so the list is in record order whatever order the blocks ran in.
//   order   the host brings the 16-byte hits into region-major order with a stable counting sort
//           (the keys (region, record) are unique) and scans en - st into output offsets.  The
//           list is 16 bytes a hit beside the ~300 bytes a hit of bases and qualities, and the
//           host needs it for the names anyway; no base passes through the host here.
//   emit    a lane per four output bytes: the hit of the first byte by binary search on the
//           output offsets, nibbles through the 16-letter table (the parity of st + k picks the
//           half), qualities + 33, one aligned dword store to text and one to quals.
// No atomic arrival order reaches the result: the only atomics are sums of counters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/crispr_nw.h"
#include "../../include/crispr_regions.h"
#include "nw_bam.h"

namespace nwr {

constexpr int kBlk = 256, kScanBlk = 1024;
constexpr int64_t kChunkBytes = (int64_t)256 << 20;   // records per chunk by default
constexpr int64_t kChunkRecords = (int64_t)4 << 20;
constexpr int64_t kMaxHits = (int64_t)1 << 30;        // of a chunk
enum { kHits = 0, kNoSeq = 1 };

struct Args {
    const uint8_t* data;       // the chunk's records
    const int64_t* off;        // [cn + 1] the records' starts within data
    int32_t cn;
    int32_t nreg;              // the region table, sorted by (ref, start)
    const int32_t* rref;
    const int64_t* rstart;
    const int64_t* rend;
    int32_t flags;
    uint32_t* counts;          // [cn] hits of every record
    uint32_t* sums;            // [blocks] hits of every block, then their exclusive scan
    int64_t blocks;
    unsigned long long* totals;
    uint4* hits;               // (region in table order, record of the chunk, st, en)
};

struct EmitHit {
    int64_t seq;               // where the record's sequence bytes start within the chunk
    int32_t l_seq;
    int32_t st;
};

__device__ inline uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ inline uint32_t ld32(const uint8_t* p) { return ld16(p) | (ld16(p + 2) << 16); }

// What an op advances: 1 = query and reference (M), 2 = query (I, S), 3 = reference (D, N),
// 0 = neither (H, P, =, X and the codes BAM does not define; = and X as M with eqx).
__device__ inline int op_class(uint32_t op, bool eqx) {
    if (op == 0 || (eqx && (op == 7 || op == 8))) return 1;
    if (op == 1 || op == 4) return 2;
    if (op == 2 || op == 3) return 3;
    return 0;
}

// the first region not before (ref, x)
__device__ inline int lower_bound(const Args& a, int32_t ref, int64_t x) {
    int lo = 0, hi = a.nreg;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int32_t r = a.rref[mid];
        if (r < ref || (r == ref && a.rstart[mid] < x)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Calls hit(region, st, en) for every hit of record i in table order; returns the hits dropped
// because the record has no sequence or no qualities.
template <class F>
__device__ inline uint32_t for_each_hit(const Args& a, int64_t i, F&& hit) {
    const uint8_t* r = a.data + a.off[i];
    const int32_t ref = (int32_t)ld32(r + nw_bam::kRefId);
    const uint32_t flag = ld16(r + nw_bam::kFlag);
    if ((flag & 4u) || ref < 0) return 0;
    const int32_t n_op = (int32_t)ld16(r + nw_bam::kNCigar), l_seq = (int32_t)ld32(r + nw_bam::kLSeq);
    const uint8_t* cig = r + nw_bam::kName + r[nw_bam::kLReadName];
    const bool has_seq = l_seq > 0 && cig[4 * (int64_t)n_op + (l_seq + 1) / 2] != 0xFF;
    if (a.flags & NWR_BY_REFERENCE) {
        if (!has_seq) return 1;
        hit((uint32_t)ref, 0, l_seq);
        return 0;
    }
    const bool eqx = (a.flags & NWR_EQX_AS_MATCH) != 0;
    const int64_t pos1 = (int64_t)(int32_t)ld32(r + nw_bam::kPos) + 1;
    int64_t pos = pos1, first = -1;
    for (int k = 0; k < n_op; ++k) {
        const uint32_t v = ld32(cig + 4 * k);
        const int64_t len = v >> 4;
        const int c = op_class(v & 15u, eqx);
        if (c == 1 && len > 0 && first < 0) first = pos;
        if (c == 1 || c == 3) pos += len;
    }
    if (first < 0) return 0;
    const int lo = lower_bound(a, ref, first), hi = lower_bound(a, ref, pos);
    uint32_t dropped = 0;
    for (int g = lo; g < hi; ++g) {
        const int64_t bs = a.rstart[g], be = a.rend[g];
        int64_t p = pos1, q = 0, st = -1, en = -1;
        for (int k = 0; k < n_op; ++k) {
            const uint32_t v = ld32(cig + 4 * k);
            const int64_t len = v >> 4;
            const int c = op_class(v & 15u, eqx);
            if (c == 1) {
                if (bs >= p && bs < p + len) st = q + (bs - p);
                if (be >= p && be < p + len) en = q + (be - p);
                p += len;
                q += len;
            } else if (c == 2) {
                q += len;
            } else if (c == 3) {
                p += len;
            }
        }
        if (st < 0 || en < 0) continue;
        if (!has_seq) {
            ++dropped;
            continue;
        }
        hit((uint32_t)g, (int32_t)(st < 0x7FFFFFFF ? st : 0x7FFFFFFF), (int32_t)(en < 0x7FFFFFFF ? en : 0x7FFFFFFF));
    }
    return dropped;
}

__global__ __launch_bounds__(kBlk) void nwr_count_kernel(const Args a) {
    __shared__ uint32_t part[kBlk / 64][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    uint32_t cnt = 0, dropped = 0;
    if (i < a.cn) {
        dropped = for_each_hit(a, i, [&](uint32_t, int32_t, int32_t) { ++cnt; });
        a.counts[i] = cnt;
    }
    uint32_t v0 = cnt, v1 = dropped;
    for (int s = 32; s > 0; s >>= 1) {
        v0 += __shfl_xor(v0, s);
        v1 += __shfl_xor(v1, s);
    }
    if (lane == 0) part[wave][0] = v0, part[wave][1] = v1;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s0 = 0, s1 = 0;
        for (int w = 0; w < kBlk / 64; ++w) s0 += part[w][0], s1 += part[w][1];
        a.sums[blockIdx.x] = s0;
        if (s0) atomicAdd(&a.totals[kHits], (unsigned long long)s0);      // (sums: no order shows)
        if (s1) atomicAdd(&a.totals[kNoSeq], (unsigned long long)s1);
    }
}

// One block: sums[b] becomes the exclusive prefix over the blocks before b (the total is under
// 2^30, checked by the host before this launch).
__global__ __launch_bounds__(kScanBlk) void nwr_scan_kernel(const Args a) {
    __shared__ uint32_t sh[2][kScanBlk];
    const int t = threadIdx.x;
    const int64_t per = (a.blocks + kScanBlk - 1) / kScanBlk;
    const int64_t lo = std::min<int64_t>(a.blocks, t * per), hi = std::min<int64_t>(a.blocks, lo + per);
    uint32_t mine = 0;
    for (int64_t b = lo; b < hi; ++b) mine += a.sums[b];
    int cur = 0;
    sh[0][t] = mine;
    __syncthreads();
    for (int d = 1; d < kScanBlk; d <<= 1) {
        sh[cur ^ 1][t] = sh[cur][t] + (t >= d ? sh[cur][t - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    uint32_t run = sh[cur][t] - mine;
    for (int64_t b = lo; b < hi; ++b) {
        const uint32_t v = a.sums[b];
        a.sums[b] = run;
        run += v;
    }
}

__global__ __launch_bounds__(kBlk) void nwr_write_kernel(const Args a) {
    __shared__ uint32_t part[kBlk / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    const uint32_t cnt = i < a.cn ? a.counts[i] : 0u;
    uint32_t x = cnt;
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t y = __shfl_up(x, s);
        if (lane >= s) x += y;
    }
    if (lane == 63) part[wave] = x;
    __syncthreads();
    uint32_t at = a.sums[blockIdx.x] + x - cnt;
    for (int w = 0; w < wave; ++w) at += part[w];
    if (cnt == 0) return;
    const uint32_t end = at + cnt;      // (the walk is the count kernel's: it cannot pass its own count)
    for_each_hit(a, i, [&](uint32_t g, int32_t st, int32_t en) {
        if (at < end) a.hits[at++] = make_uint4(g, (uint32_t)i, (uint32_t)st, (uint32_t)en);
    });
}

// "=ACMGRSVTWYHKDBN" as two little-endian words
constexpr uint64_t kNibLo = 0x565352474D43413Dull, kNibHi = 0x4E42444B48595754ull;

__global__ __launch_bounds__(256) void nwr_emit_kernel(const uint8_t* data, const EmitHit* eh, const uint32_t* ooff,
                                                       int64_t n_hits, int64_t total, uint32_t* text, uint32_t* quals) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t b0 = 4 * t;
    if (b0 >= total) return;
    // the hit of byte b0: the last h with ooff[h] <= b0 (so ooff[h + 1] > b0; empty hits fall out)
    int64_t lo = 0, hi = n_hits;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)ooff[mid] <= b0) lo = mid;
        else hi = mid;
    }
    int64_t h = lo;
    EmitHit e = eh[h];
    int64_t h0 = ooff[h], h1 = ooff[h + 1];
    uint32_t tw = 0, qw = 0;
    for (int k = 0; k < 4; ++k) {
        const int64_t b = b0 + k;
        if (b >= total) break;
        if (b >= h1) {
            do {
                ++h;
                h1 = ooff[h + 1];
            } while (b >= h1);      // (b < total = ooff[n_hits]: ends inside the list)
            h0 = ooff[h];
            e = eh[h];
        }
        const int64_t q = (int64_t)e.st + (b - h0);
        const uint32_t two = data[e.seq + (q >> 1)];
        const uint32_t code = (q & 1) ? (two & 15u) : (two >> 4);
        const uint32_t letter = (uint32_t)(((code & 8u) ? kNibHi : kNibLo) >> (8 * (code & 7u))) & 0xFFu;
        const uint32_t qual = ((uint32_t)data[e.seq + (e.l_seq + 1) / 2 + q] + 33u) & 0xFFu;
        tw |= letter << (8 * k);
        qw |= qual << (8 * k);
    }
    text[t] = tw;
    quals[t] = qw;
}

template <class T>
struct Buf {
    T* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t n) {
        if (n <= cap && p) return hipSuccess;
        release();
        hipError_t e = hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// The hits of one chunk (or of the whole call) in region-major order.
struct Hits {
    std::vector<int32_t> reg, st, en;
    std::vector<int64_t> src, toff{0};
    std::vector<uint8_t> text, quals;
};

struct Result {
    std::vector<int64_t> region_off;
    Hits h;
};

}  // namespace nwr

struct nwr_ctx {
    int device = 0;
    int64_t chunk_records = 0;      // 0: by bytes
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {};
    std::string err;
    nwr::Buf<uint8_t> d_data;
    nwr::Buf<int64_t> d_off, d_rstart, d_rend;
    nwr::Buf<int32_t> d_rref;
    nwr::Buf<uint32_t> d_counts, d_sums, d_ooff, d_text, d_quals;
    nwr::Buf<unsigned long long> d_totals;
    nwr::Buf<uint4> d_hits;
    nwr::Buf<nwr::EmitHit> d_eh;
};

namespace {

int rfail(nwr_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define RHIP(c, expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return rfail((c), e_ == hipErrorOutOfMemory ? NW_E_NOMEM : NW_E_HIP, "%s: %s", #expr, \
                         hipGetErrorString(e_));                                                  \
    } while (0)

inline uint32_t h16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t h32(const uint8_t* p) { return h16(p) | (h16(p + 2) << 16); }

// One chunk: records [r0, r1) of bam; its hits in region-major order (the caller's regions).
int run_chunk(nwr_ctx* c, const nwr_bam* bam, int64_t r0, int64_t r1, nwr::Args a, const std::vector<int32_t>& perm,
              int64_t n_regions, std::vector<int64_t>* cursor, nwr::Hits* out, int64_t* n_no_seq, float* kernel_ms,
              float* upload_ms) {
    hipStream_t st = c->stream;
    const int64_t cn = r1 - r0, base = bam->off[(size_t)r0], nbytes = bam->off[(size_t)r1] - base;
    const int64_t blocks = (cn + nwr::kBlk - 1) / nwr::kBlk;
    std::vector<int64_t> off((size_t)cn + 1);
    for (int64_t i = 0; i <= cn; ++i) off[(size_t)i] = bam->off[(size_t)(r0 + i)] - base;
    RHIP(c, c->d_data.reserve((size_t)nbytes));
    RHIP(c, c->d_off.reserve((size_t)cn + 1));
    RHIP(c, c->d_counts.reserve((size_t)cn));
    RHIP(c, c->d_sums.reserve((size_t)blocks));
    const auto t0 = std::chrono::steady_clock::now();
    RHIP(c, hipMemcpyAsync(c->d_data.p, bam->data.data() + base, (size_t)nbytes, hipMemcpyHostToDevice, st));
    RHIP(c, hipMemcpyAsync(c->d_off.p, off.data(), sizeof(int64_t) * (size_t)(cn + 1), hipMemcpyHostToDevice, st));
    RHIP(c, hipMemsetAsync(c->d_totals.p, 0, 2 * sizeof(unsigned long long), st));
    RHIP(c, hipStreamSynchronize(st));
    *upload_ms += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    a.data = c->d_data.p;
    a.off = c->d_off.p;
    a.cn = (int32_t)cn;
    a.counts = c->d_counts.p;
    a.sums = c->d_sums.p;
    a.blocks = blocks;
    a.totals = c->d_totals.p;
    RHIP(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(nwr::nwr_count_kernel, dim3((unsigned)blocks), dim3(nwr::kBlk), 0, st, a);
    RHIP(c, hipGetLastError());
    RHIP(c, hipEventRecord(c->ev[1], st));
    unsigned long long totals[2] = {0, 0};
    RHIP(c, hipMemcpyAsync(totals, a.totals, sizeof totals, hipMemcpyDeviceToHost, st));
    RHIP(c, hipStreamSynchronize(st));
    float ms = 0.0f;
    RHIP(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    *kernel_ms += ms;
    *n_no_seq += (int64_t)totals[nwr::kNoSeq];
    const int64_t nh = (int64_t)totals[nwr::kHits];
    if (nh > nwr::kMaxHits)
        return rfail(c, NW_E_UNSUPPORTED, "%lld hits in the chunk of records %lld to %lld: at most 2^30 (use a smaller CRISPR_NWR_CHUNK)",
                     (long long)nh, (long long)r0, (long long)r1);
    if (nh == 0) return NW_OK;

    RHIP(c, c->d_hits.reserve((size_t)nh));
    a.hits = c->d_hits.p;
    RHIP(c, hipEventRecord(c->ev[2], st));
    hipLaunchKernelGGL(nwr::nwr_scan_kernel, dim3(1), dim3(nwr::kScanBlk), 0, st, a);
    RHIP(c, hipGetLastError());
    hipLaunchKernelGGL(nwr::nwr_write_kernel, dim3((unsigned)blocks), dim3(nwr::kBlk), 0, st, a);
    RHIP(c, hipGetLastError());
    RHIP(c, hipEventRecord(c->ev[3], st));
    std::vector<uint4> hits((size_t)nh);
    RHIP(c, hipMemcpyAsync(hits.data(), a.hits, sizeof(uint4) * (size_t)nh, hipMemcpyDeviceToHost, st));
    RHIP(c, hipStreamSynchronize(st));
    RHIP(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
    *kernel_ms += ms;

    // region-major, record order within a region: a stable counting sort on the caller's region
    const bool by_ref = (a.flags & NWR_BY_REFERENCE) != 0;
    std::vector<int64_t>& cur = *cursor;
    std::fill(cur.begin(), cur.end(), 0);
    for (const uint4& h : hits) {
        if ((int64_t)h.x >= (by_ref ? n_regions : (int64_t)perm.size()) || (int64_t)h.y >= cn)
            return rfail(c, NW_E_STATE, "inconsistent hit");
        ++cur[(size_t)(by_ref ? (int32_t)h.x : perm[h.x]) + 1];
    }
    for (int64_t g = 0; g < n_regions; ++g) cur[(size_t)g + 1] += cur[(size_t)g];
    out->reg.resize((size_t)nh);
    out->src.resize((size_t)nh);
    out->st.resize((size_t)nh);
    out->en.resize((size_t)nh);
    std::vector<nwr::EmitHit> eh((size_t)nh);
    std::vector<int32_t> len((size_t)nh);
    for (const uint4& h : hits) {
        const int32_t g = by_ref ? (int32_t)h.x : perm[h.x];
        const size_t k = (size_t)cur[(size_t)g]++;
        const uint8_t* r = bam->data.data() + bam->off[(size_t)(r0 + h.y)];
        const int64_t l_seq = (int32_t)h32(r + nw_bam::kLSeq);
        const int64_t s = std::min<int64_t>((int32_t)h.z, l_seq), e = std::min<int64_t>((int32_t)h.w, l_seq);
        out->reg[k] = g;
        out->src[k] = r0 + h.y;
        out->st[k] = (int32_t)h.z;
        out->en[k] = (int32_t)h.w;
        len[k] = (int32_t)std::max<int64_t>(0, e - s);
        eh[k].seq = off[h.y] + nw_bam::kName + r[nw_bam::kLReadName] + 4 * (int64_t)h16(r + nw_bam::kNCigar);
        eh[k].l_seq = (int32_t)l_seq;
        eh[k].st = (int32_t)s;
    }
    out->toff.resize((size_t)nh + 1);
    out->toff[0] = 0;
    for (int64_t k = 0; k < nh; ++k) out->toff[(size_t)k + 1] = out->toff[(size_t)k] + len[(size_t)k];
    const int64_t total = out->toff[(size_t)nh];
    if (total >= ((int64_t)1 << 32))
        return rfail(c, NW_E_UNSUPPORTED, "%lld output bytes in the chunk of records %lld to %lld: under 2^32 (use a smaller CRISPR_NWR_CHUNK)",
                     (long long)total, (long long)r0, (long long)r1);
    if (total == 0) return NW_OK;
    std::vector<uint32_t> ooff((size_t)nh + 1);
    for (int64_t k = 0; k <= nh; ++k) ooff[(size_t)k] = (uint32_t)out->toff[(size_t)k];
    const int64_t words = (total + 3) / 4;
    RHIP(c, c->d_eh.reserve((size_t)nh));
    RHIP(c, c->d_ooff.reserve((size_t)nh + 1));
    RHIP(c, c->d_text.reserve((size_t)words));
    RHIP(c, c->d_quals.reserve((size_t)words));
    RHIP(c, hipMemcpyAsync(c->d_eh.p, eh.data(), sizeof(nwr::EmitHit) * (size_t)nh, hipMemcpyHostToDevice, st));
    RHIP(c, hipMemcpyAsync(c->d_ooff.p, ooff.data(), sizeof(uint32_t) * (size_t)(nh + 1), hipMemcpyHostToDevice, st));
    RHIP(c, hipEventRecord(c->ev[4], st));
    hipLaunchKernelGGL(nwr::nwr_emit_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, c->d_data.p, c->d_eh.p,
                       c->d_ooff.p, nh, total, c->d_text.p, c->d_quals.p);
    RHIP(c, hipGetLastError());
    RHIP(c, hipEventRecord(c->ev[5], st));
    out->text.resize((size_t)words * 4);
    out->quals.resize((size_t)words * 4);
    RHIP(c, hipMemcpyAsync(out->text.data(), c->d_text.p, (size_t)words * 4, hipMemcpyDeviceToHost, st));
    RHIP(c, hipMemcpyAsync(out->quals.data(), c->d_quals.p, (size_t)words * 4, hipMemcpyDeviceToHost, st));
    RHIP(c, hipStreamSynchronize(st));
    RHIP(c, hipEventElapsedTime(&ms, c->ev[4], c->ev[5]));
    *kernel_ms += ms;
    out->text.resize((size_t)total);
    out->quals.resize((size_t)total);
    return NW_OK;
}

// The chunks' hits (each region-major) as one region-major list, the chunks in order in a region.
void merge_chunks(std::vector<nwr::Hits>& chunks, int64_t n_regions, nwr::Result* res) {
    std::vector<int64_t>& ro = res->region_off;
    ro.assign((size_t)n_regions + 1, 0);
    for (const nwr::Hits& h : chunks)
        for (int32_t g : h.reg) ++ro[(size_t)g + 1];
    for (int64_t g = 0; g < n_regions; ++g) ro[(size_t)g + 1] += ro[(size_t)g];
    if (chunks.size() == 1) {
        res->h = std::move(chunks[0]);
        return;
    }
    const size_t nh = (size_t)ro[(size_t)n_regions];
    nwr::Hits& o = res->h;
    o.reg.resize(nh);
    o.src.resize(nh);
    o.st.resize(nh);
    o.en.resize(nh);
    o.toff.assign(nh + 1, 0);
    std::vector<int64_t> cur(ro.begin(), ro.end() - 1);
    // pass 1: every hit's slot and length; pass 2: the bytes, a run of one region at a time
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            for (size_t k = 0; k < nh; ++k) o.toff[k + 1] += o.toff[k];
            o.text.resize((size_t)o.toff[nh]);
            o.quals.resize((size_t)o.toff[nh]);
            std::copy(ro.begin(), ro.end() - 1, cur.begin());
        }
        for (const nwr::Hits& h : chunks) {
            const size_t n = h.reg.size();
            for (size_t x = 0; x < n;) {
                size_t y = x + 1;
                while (y < n && h.reg[y] == h.reg[x]) ++y;
                const size_t k = (size_t)cur[(size_t)h.reg[x]];
                cur[(size_t)h.reg[x]] += (int64_t)(y - x);
                if (pass == 0) {
                    for (size_t j = 0; j < y - x; ++j) {
                        o.reg[k + j] = h.reg[x + j];
                        o.src[k + j] = h.src[x + j];
                        o.st[k + j] = h.st[x + j];
                        o.en[k + j] = h.en[x + j];
                        o.toff[k + j + 1] = h.toff[x + j + 1] - h.toff[x + j];
                    }
                } else if (h.toff[y] > h.toff[x]) {
                    std::memcpy(o.text.data() + o.toff[k], h.text.data() + h.toff[x], (size_t)(h.toff[y] - h.toff[x]));
                    std::memcpy(o.quals.data() + o.toff[k], h.quals.data() + h.toff[x], (size_t)(h.toff[y] - h.toff[x]));
                }
                x = y;
            }
        }
    }
}

}  // namespace

extern "C" {

int nwr_create(int device, nwr_ctx** out) {
    if (!out) return NW_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return NW_E_HIP;
    nwr_ctx* c = new nwr_ctx();
    c->device = device;
    bool ok = hipSetDevice(device) == hipSuccess &&
              hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i < 6; ++i) ok = hipEventCreate(&c->ev[i]) == hipSuccess;
    if (!ok) {
        nwr_destroy(c);
        return NW_E_HIP;
    }
    if (const char* e = std::getenv("CRISPR_NWR_CHUNK"))
        c->chunk_records = std::max<int64_t>(0, std::min<int64_t>(std::atoll(e), nwr::kChunkRecords));
    *out = c;
    return NW_OK;
}

void nwr_destroy(nwr_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    c->d_data.release();
    c->d_off.release();
    c->d_rstart.release();
    c->d_rend.release();
    c->d_rref.release();
    c->d_counts.release();
    c->d_sums.release();
    c->d_ooff.release();
    c->d_text.release();
    c->d_quals.release();
    c->d_totals.release();
    c->d_hits.release();
    c->d_eh.release();
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* nwr_last_error(const nwr_ctx* c) { return c ? c->err.c_str() : "null context"; }

int nwr_extract(nwr_ctx* c, const nwr_bam* bam, const nwr_region* regions, int64_t n_regions, int32_t flags,
                nwr_result* res) {
    if (!c) return NW_E_INVALID;
    if (!bam || !res) return rfail(c, NW_E_INVALID, "null argument");
    std::memset(res, 0, sizeof *res);
    if (flags & ~(NWR_BY_REFERENCE | NWR_EQX_AS_MATCH)) return rfail(c, NW_E_INVALID, "unknown flags %d", (int)flags);
    const bool by_ref = (flags & NWR_BY_REFERENCE) != 0;
    if (by_ref) n_regions = (int64_t)bam->ref_len.size();
    if (n_regions < 0 || (!by_ref && n_regions > 0 && !regions)) return rfail(c, NW_E_INVALID, "null regions");
    if (n_regions > NWR_MAX_REGIONS)
        return rfail(c, NW_E_UNSUPPORTED, "%lld regions: at most %d are supported", (long long)n_regions, NWR_MAX_REGIONS);
    const int64_t n = (int64_t)bam->off.size() - 1;
    nwr::Result* R = new nwr::Result();
    R->region_off.assign((size_t)n_regions + 1, 0);
    res->n_regions = n_regions;
    res->handle = R;
    if (n <= 0 || n_regions == 0) return NW_OK;

    auto bail = [&](int rc) {
        delete R;
        res->handle = nullptr;
        return rc;
    };
    nwr::Args a{};
    a.flags = flags;
    std::vector<int32_t> perm;
    if (hipSetDevice(c->device) != hipSuccess) return bail(rfail(c, NW_E_HIP, "hipSetDevice failed"));
    int rc = [&]() -> int {
        RHIP(c, c->d_totals.reserve(2));
        if (by_ref) return NW_OK;
        // the table in (ref, bpstart) order, equal keys in the caller's order; perm leads back
        perm.resize((size_t)n_regions);
        std::iota(perm.begin(), perm.end(), 0);
        std::stable_sort(perm.begin(), perm.end(), [&](int32_t x, int32_t y) {
            if (regions[x].ref_id != regions[y].ref_id) return regions[x].ref_id < regions[y].ref_id;
            return regions[x].bpstart < regions[y].bpstart;
        });
        std::vector<int32_t> rref((size_t)n_regions);
        std::vector<int64_t> rstart((size_t)n_regions), rend((size_t)n_regions);
        for (int64_t g = 0; g < n_regions; ++g) {
            const nwr_region& r = regions[perm[(size_t)g]];
            rref[(size_t)g] = r.ref_id;
            rstart[(size_t)g] = r.bpstart;
            rend[(size_t)g] = r.bpend;
        }
        RHIP(c, c->d_rref.reserve((size_t)n_regions));
        RHIP(c, c->d_rstart.reserve((size_t)n_regions));
        RHIP(c, c->d_rend.reserve((size_t)n_regions));
        RHIP(c, hipMemcpy(c->d_rref.p, rref.data(), sizeof(int32_t) * (size_t)n_regions, hipMemcpyHostToDevice));
        RHIP(c, hipMemcpy(c->d_rstart.p, rstart.data(), sizeof(int64_t) * (size_t)n_regions, hipMemcpyHostToDevice));
        RHIP(c, hipMemcpy(c->d_rend.p, rend.data(), sizeof(int64_t) * (size_t)n_regions, hipMemcpyHostToDevice));
        a.nreg = (int32_t)n_regions;
        a.rref = c->d_rref.p;
        a.rstart = c->d_rstart.p;
        a.rend = c->d_rend.p;
        return NW_OK;
    }();
    if (rc != NW_OK) return bail(rc);

    std::vector<nwr::Hits> chunks;
    std::vector<int64_t> cursor((size_t)n_regions + 1);
    for (int64_t r0 = 0; r0 < n;) {
        int64_t r1;
        if (c->chunk_records > 0) {
            r1 = std::min(n, r0 + c->chunk_records);
        } else {
            r1 = std::min(n, r0 + nwr::kChunkRecords);
            const int64_t* o = bam->off.data();
            const int64_t* e = std::upper_bound(o + r0 + 1, o + r1 + 1, o[r0] + nwr::kChunkBytes);
            r1 = std::max<int64_t>(r0 + 1, (e - o) - 1);      // (one record at least, whatever its size)
        }
        nwr::Hits h;
        rc = run_chunk(c, bam, r0, r1, a, perm, n_regions, &cursor, &h, &res->n_no_seq, &res->kernel_ms, &res->upload_ms);
        if (rc != NW_OK) return bail(rc);
        if (!h.reg.empty()) chunks.push_back(std::move(h));
        r0 = r1;
    }
    merge_chunks(chunks, n_regions, R);
    res->n_hits = (int64_t)R->h.reg.size();
    res->n_bytes = R->h.toff.back();
    return NW_OK;
}

int nwr_fetch(const nwr_result* res, int64_t* region_offsets, int64_t* src, int32_t* st, int32_t* en,
              int64_t* text_offsets, uint8_t* text, uint8_t* quals) {
    if (!res || !res->handle) return NW_E_INVALID;
    const nwr::Result* R = (const nwr::Result*)res->handle;
    const nwr::Hits& h = R->h;
    const size_t nh = h.reg.size(), nb = (size_t)h.toff.back();
    if (region_offsets) std::memcpy(region_offsets, R->region_off.data(), sizeof(int64_t) * R->region_off.size());
    if (src && nh) std::memcpy(src, h.src.data(), sizeof(int64_t) * nh);
    if (st && nh) std::memcpy(st, h.st.data(), sizeof(int32_t) * nh);
    if (en && nh) std::memcpy(en, h.en.data(), sizeof(int32_t) * nh);
    if (text_offsets) std::memcpy(text_offsets, h.toff.data(), sizeof(int64_t) * (nh + 1));
    if (text && nb) std::memcpy(text, h.text.data(), nb);
    if (quals && nb) std::memcpy(quals, h.quals.data(), nb);
    return NW_OK;
}

void nwr_release(nwr_result* res) {
    if (!res) return;
    delete (nwr::Result*)res->handle;
    res->handle = nullptr;
}

}  // extern "C"
