// fastq_parse.hip -- the FASTQ ingest with qualities on gfx950 (include/crispr_ingest.h): the
// inflated text of a FASTQ file, uploaded once, to dense bases / qualities / names with int64
// offsets and a flag byte a record, all resident in HBM for the front end (front_pack.hip,
// nwp_prepare_records).  The records are flash.read_fastq's (crispresso_amd/flash.py): the
// semantics are restated in the header and in tests/ingest_model.py.
//
// The text lies on the device padded with zero bytes to a multiple of 16 (and 16 more, so an
// aligned dword pair around any text byte is readable).  Per call, on the null stream:
//   count    a lane per 16 bytes (one dwordx4 load): its '\n' bytes; the block's sum (256 lanes,
//            4 KiB of text) goes to sums[block].
//   scan     one block: the exclusive scan of the block sums and the total.
//   lines    the same sweep again: every newline's position (uint32) lands at its rank, the
//            block's base plus the newlines before it in the block, so the index is in text
//            order whatever order the blocks ran in.
//   records  a lane per record: its five line bounds from the index, the trailing '\r's of the
//            header, sequence and quality line stripped, the first byte of lines 0 and 2; the
//            three starts and lengths and flag bits 0-2 are stored, the block's three length
//            sums and its longest sequence go to sums / bmax.
//   scan     the three sums' exclusive scans, the totals and the longest sequence.
//   offsets  a lane per record: the scan of the block's lengths on top of the block's base is
//            the record's offset in each of the three streams.
//   gather   (bases, qualities, names) a lane per four output bytes: the record of the first
//            byte by binary search on the stream's offsets (empty fields fall out of the search),
//            the source bytes from the unaligned text (two aligned dwords and a shift when all
//            four lie in one record, else byte by byte, stepping into the next record), one
//            aligned dword store.  The quality gather tests 33..126 on the bytes it holds and
//            sets flag bit 3: every writer of a record's flag byte writes the same value.
//   tally    the flag bytes to per-block (count of each bit, smallest flagged index), then one
//            block sums those.
// No atomic anywhere: every order comes from a scan, every reduction from block partials.
// Positions are 32-bit: a text of 2^32 - 16 bytes or more, or with more than 2^31 lines, is
// refused (never truncated).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <zlib.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/crispr_ingest.h"
#include "gz_inflate.h"
#include "host_dev.h"
#include "host_pool.h"
#include "ingest_device.h"

namespace nwi {

constexpr int kBlk = 256, kScanBlk = 1024;
constexpr int kTallyBlocks = 1024;                       // at most (one scan block sums them)
constexpr uint64_t kMaxText = (1ull << 32) - 16;         // bytes of text a call takes: fewer than this
constexpr int64_t kMaxLines = (int64_t)1 << 31;
enum { kTotSeq = 0, kTotQual = 1, kTotName = 2, kTotLmax = 3, kTotals = 4 };

// 0x80 in every byte of w that is '\n'
__device__ __forceinline__ uint32_t nl_mask(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// the block's sum of v (every thread calls it; part has a slot a wave); valid in thread 0
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* part) {
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    __syncthreads();   // part may still be read from the call before
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t s = 0;
    if (threadIdx.x == 0)
        for (unsigned w = 0; w < blockDim.x / 64; ++w) s += part[w];
    return s;
}

// v's exclusive prefix over the block's threads (every thread calls it)
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t y = __shfl_up(x, s);
        if (lane >= s) x += y;
    }
    __syncthreads();
    if (lane == 63) part[wave] = x;
    __syncthreads();
    uint32_t before = x - v;
    for (int w = 0; w < wave; ++w) before += part[w];
    return before;
}

// ---- the line index -------------------------------------------------------------------------

__global__ __launch_bounds__(kBlk) void nwi_count_kernel(const uint4* text, int64_t chunks, uint32_t* sums) {
    __shared__ uint32_t part[kBlk / 64];
    const int64_t c = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    uint32_t cnt = 0;
    if (c < chunks) {
        const uint4 d = text[c];
        cnt = __popc(nl_mask(d.x)) + __popc(nl_mask(d.y)) + __popc(nl_mask(d.z)) + __popc(nl_mask(d.w));
    }
    const uint32_t s = block_sum(cnt, part);
    if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

// One block: sums[nq b + q] becomes the exclusive prefix over the blocks before b, totals[q] the
// sum; with bmax, totals[nq] is the largest bmax[b].
__global__ __launch_bounds__(kScanBlk) void nwi_scan_kernel(uint32_t* sums, int64_t blocks, int nq, const uint32_t* bmax,
                                                            int64_t* totals) {
    __shared__ uint32_t sh[2][kScanBlk];
    const int t = threadIdx.x;
    const int64_t per = (blocks + kScanBlk - 1) / kScanBlk;
    const int64_t lo = std::min<int64_t>(blocks, t * per), hi = std::min<int64_t>(blocks, lo + per);
    for (int q = 0; q < nq; ++q) {
        uint32_t mine = 0;
        for (int64_t b = lo; b < hi; ++b) mine += sums[nq * b + q];
        int cur = 0;
        sh[0][t] = mine;
        __syncthreads();
        for (int d = 1; d < kScanBlk; d <<= 1) {   // inclusive scan of the threads' sums
            sh[cur ^ 1][t] = sh[cur][t] + (t >= d ? sh[cur][t - d] : 0u);
            cur ^= 1;
            __syncthreads();
        }
        uint32_t run = sh[cur][t] - mine;
        if (t == kScanBlk - 1) totals[q] = (int64_t)sh[cur][t];
        for (int64_t b = lo; b < hi; ++b) {
            const uint32_t v = sums[nq * b + q];
            sums[nq * b + q] = run;
            run += v;
        }
        __syncthreads();
    }
    if (bmax) {
        uint32_t mine = 0;
        for (int64_t b = lo; b < hi; ++b) mine = max(mine, bmax[b]);
        sh[0][t] = mine;
        __syncthreads();
        for (int d = kScanBlk / 2; d > 0; d >>= 1) {
            if (t < d) sh[0][t] = max(sh[0][t], sh[0][t + d]);
            __syncthreads();
        }
        if (t == 0) totals[nq] = (int64_t)sh[0][0];
    }
}

__global__ __launch_bounds__(kBlk) void nwi_lines_kernel(const uint4* text, int64_t chunks, const uint32_t* sums,
                                                         uint32_t* nl, int64_t n_nl) {
    __shared__ uint32_t part[kBlk / 64];
    const int64_t c = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    uint32_t m[4] = {0, 0, 0, 0};
    if (c < chunks) {
        const uint4 d = text[c];
        m[0] = nl_mask(d.x), m[1] = nl_mask(d.y), m[2] = nl_mask(d.z), m[3] = nl_mask(d.w);
    }
    const uint32_t cnt = __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
    int64_t at = (int64_t)sums[blockIdx.x] + block_exclusive(cnt, part);
#pragma unroll
    for (int w = 0; w < 4; ++w)
        for (uint32_t x = m[w]; x; x &= x - 1) {
            const uint32_t k = (uint32_t)__builtin_ctz(x) >> 3;
            if (at < n_nl) nl[at] = (uint32_t)(16 * c) + 4u * w + k;   // (the count kernel's count: always inside)
            ++at;
        }
}

// ---- the records ----------------------------------------------------------------------------

struct RecArgs {
    const uint8_t* text;
    const uint32_t* nl;    // [n_nl] the newlines' positions, ascending
    int64_t n_nl;
    uint32_t T;            // bytes of text
    int64_t n;             // records
    uint32_t* start;       // [3][n]: where seq, qual, name begin in the text
    uint32_t* len;         // [3][n]
    uint8_t* flags;        // [n]
    uint32_t* sums;        // [3 blocks]: the blocks' length sums, then their bases
    uint32_t* bmax;        // [blocks]: the blocks' longest sequence
    int64_t* totals;       // [kTotals]
    int64_t* off[3];       // [n + 1] each
};

__device__ __forceinline__ uint32_t strip_cr(const uint8_t* text, uint32_t s, uint32_t e) {
    while (e > s && text[e - 1] == '\r') --e;
    return e;
}

__global__ __launch_bounds__(kBlk) void nwi_records_kernel(const RecArgs a) {
    __shared__ uint32_t part[kBlk / 64];
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    uint32_t ls = 0, lq = 0, ln = 0;
    if (r < a.n) {
        // lines 4r .. 4r+3: line i is [its predecessor's newline + 1, its own newline), the last
        // line of a text with no final newline ends at T
        const int64_t i = 4 * r;
        const uint32_t s0 = r == 0 ? 0u : a.nl[i - 1] + 1u;
        const uint32_t e0 = a.nl[i], e1 = a.nl[i + 1], e2 = a.nl[i + 2];
        const uint32_t e3 = i + 3 < a.n_nl ? a.nl[i + 3] : a.T;
        const uint32_t s1 = e0 + 1u, s2 = e1 + 1u, s3 = e2 + 1u;
        const uint32_t h = strip_cr(a.text, s0, e0), q1 = strip_cr(a.text, s1, e1), q3 = strip_cr(a.text, s3, e3);
        uint8_t f = 0;
        if (h == s0 || a.text[s0] != '@') f |= NWI_BAD_HEADER;
        if (e2 == s2 || a.text[s2] != '+') f |= NWI_BAD_PLUS;
        ls = q1 - s1, lq = q3 - s3;
        if (ls != lq) f |= NWI_LEN_MISMATCH;
        const uint32_t ns = h > s0 ? s0 + 1u : s0;
        ln = h - ns;
        a.start[r] = s1, a.start[a.n + r] = s3, a.start[2 * a.n + r] = ns;
        a.len[r] = ls, a.len[a.n + r] = lq, a.len[2 * a.n + r] = ln;
        a.flags[r] = f;
    }
    const uint32_t t0 = block_sum(ls, part), t1 = block_sum(lq, part), t2 = block_sum(ln, part);
    uint32_t mx = ls;
    for (int s = 32; s > 0; s >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, s));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        a.sums[3 * (int64_t)blockIdx.x + 0] = t0;
        a.sums[3 * (int64_t)blockIdx.x + 1] = t1;
        a.sums[3 * (int64_t)blockIdx.x + 2] = t2;
        a.bmax[blockIdx.x] = max(max(part[0], part[1]), max(part[2], part[3]));
    }
}

__global__ __launch_bounds__(kBlk) void nwi_offsets_kernel(const RecArgs a) {
    __shared__ uint32_t part[kBlk / 64];
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    for (int q = 0; q < 3; ++q) {
        const uint32_t v = r < a.n ? a.len[q * a.n + r] : 0u;
        const uint32_t before = a.sums[3 * (int64_t)blockIdx.x + q] + block_exclusive(v, part);
        if (r < a.n) a.off[q][r] = (int64_t)before;
        if (r == 0) a.off[q][a.n] = a.totals[q];
    }
}

// ---- the gather -----------------------------------------------------------------------------

// out[t] = bytes 4t .. 4t+3 of the stream whose record r is text[start[r] .. start[r] + off[r+1] - off[r]).
template <bool kQual>
__global__ __launch_bounds__(256) void nwi_gather_kernel(const uint8_t* text, const uint32_t* start, const int64_t* off,
                                                         int64_t n, int64_t total, uint32_t* out, uint8_t* flags) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t b0 = 4 * t;
    if (b0 >= total) return;
    // the record of byte b0: the last r with off[r] <= b0 (so off[r + 1] > b0)
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= b0) lo = mid;
        else hi = mid;
    }
    int64_t r = lo, h0 = off[r], h1 = off[r + 1];
    uint32_t w = 0;
    if (b0 + 3 < h1) {   // all four in record r: two aligned dwords (the text is padded past its end)
        const uint32_t s = start[r] + (uint32_t)(b0 - h0);
        const uint32_t* p = reinterpret_cast<const uint32_t*>(text + (s & ~3u));
        const uint64_t two = ((uint64_t)p[1] << 32) | p[0];
        w = (uint32_t)(two >> (8 * (s & 3u)));
        if (kQual) {
            bool bad = false;
            for (int k = 0; k < 4; ++k) {
                const uint32_t c = (w >> (8 * k)) & 0xFFu;
                bad = bad || c < 33u || c > 126u;
            }
            if (bad) flags[r] = (uint8_t)((flags[r] & 7u) | NWI_BAD_QUAL);
        }
    } else {
        for (int k = 0; k < 4; ++k) {
            const int64_t b = b0 + k;
            if (b >= total) break;
            if (b >= h1) {
                do {
                    ++r;
                    h1 = off[r + 1];
                } while (b >= h1);      // (b < total = off[n]: ends inside the list)
                h0 = off[r];
            }
            const uint32_t c = text[start[r] + (uint32_t)(b - h0)];
            w |= c << (8 * k);
            if (kQual && (c < 33u || c > 126u)) flags[r] = (uint8_t)((flags[r] & 7u) | NWI_BAD_QUAL);
        }
    }
    out[t] = w;
}

// ---- the tally ------------------------------------------------------------------------------

// partial[5 block + k]: the block's records with flag bit k (k < 4), the smallest flagged index
// (0xFFFFFFFF: none).
__global__ __launch_bounds__(kBlk) void nwi_tally_kernel(const uint8_t* flags, int64_t n, uint32_t* partial) {
    __shared__ uint32_t part[kBlk / 64];
    uint32_t c[4] = {0, 0, 0, 0}, first = 0xFFFFFFFFu;
    for (int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlk) {
        const uint32_t f = flags[r];
        for (int k = 0; k < 4; ++k) c[k] += (f >> k) & 1u;
        if (f) first = min(first, (uint32_t)r);
    }
    for (int k = 0; k < 4; ++k) {
        const uint32_t s = block_sum(c[k], part);
        if (threadIdx.x == 0) partial[5 * blockIdx.x + k] = s;
    }
    for (int s = 32; s > 0; s >>= 1) first = min(first, (uint32_t)__shfl_xor(first, s));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = first;
    __syncthreads();
    if (threadIdx.x == 0) partial[5 * blockIdx.x + 4] = min(min(part[0], part[1]), min(part[2], part[3]));
}

// One block: out[k] the sums over the blocks' partials, out[4] the smallest first (or -1).
__global__ __launch_bounds__(kScanBlk) void nwi_tally_sum_kernel(const uint32_t* partial, int blocks, int64_t* out) {
    __shared__ uint32_t part[kScanBlk / 64];
    const int t = threadIdx.x;
    for (int k = 0; k < 4; ++k) {
        const uint32_t s = block_sum(t < blocks ? partial[5 * t + k] : 0u, part);
        if (t == 0) out[k] = (int64_t)s;
    }
    uint32_t first = t < blocks ? partial[5 * t + 4] : 0xFFFFFFFFu;
    for (int s = 32; s > 0; s >>= 1) first = min(first, (uint32_t)__shfl_xor(first, s));
    __syncthreads();
    if ((t & 63) == 0) part[t >> 6] = first;
    __syncthreads();
    if (t == 0) {
        uint32_t f = 0xFFFFFFFFu;
        for (int w = 0; w < kScanBlk / 64; ++w) f = min(f, part[w]);
        out[4] = f == 0xFFFFFFFFu ? -1 : (int64_t)f;
    }
}

// ---- the host side --------------------------------------------------------------------------

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// a call's scratch arrays and events: released when it goes out of scope
struct Scratch : hd::DevBag {
    // adds what ran since begin() to *ms
    bool end(float* ms) {
        float d = 0.0f;
        if (!elapsed(&d)) return false;
        *ms += d;
        return true;
    }
};

void* keep(nwi_records* r, size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr;
    r->bufs.push_back(p);
    return p;
}

int parse(const char* who, int device, const uint8_t* text, int64_t bytes, float inflate_ms, nwi_records** out) {
    const std::string me = std::string(who) + ": ";
    if (!out || bytes < 0 || (bytes > 0 && !text)) return fail(-1, me + "null argument or negative size");
    *out = nullptr;
    if ((uint64_t)bytes >= kMaxText)
        return fail(-3, me + "a text of 2^32 - 16 bytes or more in one call is out of scope (nothing is truncated)");
    if (hipSetDevice(device) != hipSuccess) return fail(-4, me + "hipSetDevice failed");
    nwi_records* R = new nwi_records;
    R->device = device;
    nwi_summary& I = R->info;
    I.first_bad = -1;
    I.text_bytes = bytes;
    I.inflate_ms = inflate_ms;
    auto bail = [&](int code, const std::string& msg) {
        nwi_release(R);
        return fail(code, me + msg);
    };
    auto hip_fail = [&]() { return bail(-4, std::string("HIP error: ") + hipGetErrorString(hipGetLastError())); };
    if (bytes == 0) {
        *out = R;
        return 0;
    }
    Scratch S;
    const uint32_t T = (uint32_t)bytes;
    const int64_t chunks = ((int64_t)bytes + 15) / 16, blocks = (chunks + kBlk - 1) / kBlk;
    uint8_t* d_text = (uint8_t*)S.dev((size_t)(16 * chunks) + 16);
    uint32_t* d_sums = (uint32_t*)S.dev(sizeof(uint32_t) * blocks);
    int64_t* d_tot = (int64_t*)S.dev(sizeof(int64_t) * 8);
    if (!d_text || !d_sums || !d_tot) return bail(-4, "hipMalloc failed");
    if (!S.begin() || hipMemcpy(d_text, text, (size_t)bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemsetAsync(d_text + bytes, 0, (size_t)(16 * chunks + 16 - bytes), nullptr) != hipSuccess ||
        !S.end(&I.upload_ms))
        return hip_fail();

    // the line index
    if (!S.begin()) return hip_fail();
    hipLaunchKernelGGL(nwi_count_kernel, dim3((unsigned)blocks), dim3(kBlk), 0, nullptr, (const uint4*)d_text, chunks,
                       d_sums);
    hipLaunchKernelGGL(nwi_scan_kernel, dim3(1), dim3(kScanBlk), 0, nullptr, d_sums, blocks, 1, (const uint32_t*)nullptr,
                       d_tot);
    if (!S.end(&I.kernel_ms)) return hip_fail();
    int64_t n_nl = 0;
    if (hipMemcpy(&n_nl, d_tot, sizeof(n_nl), hipMemcpyDeviceToHost) != hipSuccess) return hip_fail();
    const int64_t L = n_nl + (text[bytes - 1] == '\n' ? 0 : 1);
    if (L > kMaxLines) return bail(-3, "a text of more than 2^31 lines in one call is out of scope (nothing is truncated)");
    const int64_t n = L / 4;
    I.lines = L, I.n = n, I.trailing_lines = L % 4;
    if (n == 0) {
        *out = R;
        return 0;
    }
    uint32_t* d_nl = (uint32_t*)S.dev(sizeof(uint32_t) * n_nl);
    const int64_t rblocks = (n + kBlk - 1) / kBlk;
    RecArgs ra{};
    ra.text = d_text, ra.nl = d_nl, ra.n_nl = n_nl, ra.T = T, ra.n = n;
    ra.start = (uint32_t*)S.dev(sizeof(uint32_t) * 3 * n);
    ra.len = (uint32_t*)S.dev(sizeof(uint32_t) * 3 * n);
    ra.sums = (uint32_t*)S.dev(sizeof(uint32_t) * 3 * rblocks);
    ra.bmax = (uint32_t*)S.dev(sizeof(uint32_t) * rblocks);
    ra.totals = d_tot;
    ra.flags = R->flags = (uint8_t*)keep(R, (size_t)n);
    for (int q = 0; q < 3; ++q) ra.off[q] = R->off[q] = (int64_t*)keep(R, sizeof(int64_t) * (n + 1));
    const int tblocks = (int)std::min<int64_t>(rblocks, kTallyBlocks);
    uint32_t* d_partial = (uint32_t*)S.dev(sizeof(uint32_t) * 5 * tblocks);
    if (!d_nl || !ra.start || !ra.len || !ra.sums || !ra.bmax || !ra.flags || !ra.off[0] || !ra.off[1] || !ra.off[2] ||
        !d_partial)
        return bail(-4, "hipMalloc failed");
    if (!S.begin()) return hip_fail();
    hipLaunchKernelGGL(nwi_lines_kernel, dim3((unsigned)blocks), dim3(kBlk), 0, nullptr, (const uint4*)d_text, chunks,
                       (const uint32_t*)d_sums, d_nl, n_nl);
    hipLaunchKernelGGL(nwi_records_kernel, dim3((unsigned)rblocks), dim3(kBlk), 0, nullptr, ra);
    hipLaunchKernelGGL(nwi_scan_kernel, dim3(1), dim3(kScanBlk), 0, nullptr, ra.sums, rblocks, 3,
                       (const uint32_t*)ra.bmax, d_tot);
    hipLaunchKernelGGL(nwi_offsets_kernel, dim3((unsigned)rblocks), dim3(kBlk), 0, nullptr, ra);
    if (!S.end(&I.kernel_ms)) return hip_fail();
    int64_t tot[kTotals];
    if (hipMemcpy(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost) != hipSuccess) return hip_fail();
    I.seq_bytes = tot[kTotSeq], I.qual_bytes = tot[kTotQual], I.name_bytes = tot[kTotName], I.lmax = tot[kTotLmax];

    // the streams: whole dwords are stored, and the front end's kernels may read a few bytes past the end
    const int64_t size[3] = {I.seq_bytes, I.qual_bytes, I.name_bytes};
    for (int q = 0; q < 3; ++q) {
        R->stream[q] = (uint8_t*)keep(R, (size_t)((size[q] + 3) / 4 * 4) + 16);
        if (!R->stream[q]) return bail(-4, "hipMalloc failed");
    }
    if (!S.begin()) return hip_fail();
    for (int q = 0; q < 3; ++q) {
        const int64_t words = (size[q] + 3) / 4;
        if (words == 0) continue;
        const dim3 grid((unsigned)((words + 255) / 256));
        if (q == 1)
            hipLaunchKernelGGL(nwi_gather_kernel<true>, grid, dim3(256), 0, nullptr, (const uint8_t*)d_text,
                               (const uint32_t*)(ra.start + q * n), (const int64_t*)ra.off[q], n, size[q],
                               (uint32_t*)R->stream[q], R->flags);
        else
            hipLaunchKernelGGL(nwi_gather_kernel<false>, grid, dim3(256), 0, nullptr, (const uint8_t*)d_text,
                               (const uint32_t*)(ra.start + q * n), (const int64_t*)ra.off[q], n, size[q],
                               (uint32_t*)R->stream[q], (uint8_t*)nullptr);
    }
    hipLaunchKernelGGL(nwi_tally_kernel, dim3((unsigned)tblocks), dim3(kBlk), 0, nullptr, (const uint8_t*)R->flags, n,
                       d_partial);
    hipLaunchKernelGGL(nwi_tally_sum_kernel, dim3(1), dim3(kScanBlk), 0, nullptr, (const uint32_t*)d_partial, tblocks,
                       d_tot);
    if (!S.end(&I.kernel_ms)) return hip_fail();
    int64_t tally[5];
    if (hipMemcpy(tally, d_tot, sizeof(tally), hipMemcpyDeviceToHost) != hipSuccess) return hip_fail();
    for (int k = 0; k < 4; ++k) I.flagged[k] = tally[k];
    I.first_bad = tally[4];
    *out = R;
    return 0;
}

// ---- the file -------------------------------------------------------------------------------

struct FileMap {
    const unsigned char* p = nullptr;
    size_t n = 0;
    ~FileMap() {
        if (p) munmap((void*)p, n);
    }
    // 1 mapped, 0 an empty file, -1 cannot be read
    int open_file(const char* path) {
        const int fd = open(path, O_RDONLY);
        if (fd < 0) return -1;
        struct stat st;
        int rc = -1;
        if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
            if (st.st_size == 0) {
                rc = 0;
            } else {
                void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
                if (m != MAP_FAILED) {
                    (void)madvise(m, (size_t)st.st_size, MADV_SEQUENTIAL);
                    p = (const unsigned char*)m;
                    n = (size_t)st.st_size;
                    rc = 1;
                }
            }
        }
        close(fd);
        return rc;
    }
};

// Every gzip member of [p, p + n) into out, one after the other (zlib); bytes after a member that
// do not start another are ignored.  Empty string: done; else what was wrong.
std::string inflate_members(const unsigned char* p, size_t n, std::vector<unsigned char>& out) {
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, 15 + 16) != Z_OK) return "inflateInit2 failed";
    size_t pos = 0;
    std::string err;
    out.resize(std::max<size_t>(4 * n, 1 << 16));
    size_t used = 0;
    for (int member = 0;; ++member) {
        int rc = Z_OK;
        while (rc != Z_STREAM_END) {
            if (used == out.size()) {
                if (used >= kMaxText) {
                    err = "the inflated text reaches 2^32 - 16 bytes: out of scope (nothing is truncated)";
                    break;
                }
                out.resize(std::min<size_t>(2 * out.size(), (size_t)kMaxText));
            }
            const size_t in_now = std::min<size_t>(n - pos, (size_t)1 << 30);
            const size_t out_now = std::min<size_t>(out.size() - used, (size_t)1 << 30);
            zs.next_in = const_cast<unsigned char*>(p + pos);
            zs.avail_in = (uInt)in_now;
            zs.next_out = out.data() + used;
            zs.avail_out = (uInt)out_now;
            rc = inflate(&zs, Z_NO_FLUSH);
            pos += in_now - zs.avail_in;
            used += out_now - zs.avail_out;
            if (rc == Z_STREAM_END) break;
            if (rc != Z_OK && rc != Z_BUF_ERROR) {
                err = "gzip member " + std::to_string(member) + " is damaged" + (zs.msg ? std::string(": ") + zs.msg : "");
                break;
            }
            if (pos == n && zs.avail_out > 0) {   // the input ended inside the member
                err = "gzip member " + std::to_string(member) + " is truncated";
                break;
            }
        }
        if (!err.empty()) break;
        if (n - pos < 2 || p[pos] != 0x1f || p[pos + 1] != 0x8b) break;   // no further member
        if (inflateReset(&zs) != Z_OK) {
            err = "inflateReset failed";
            break;
        }
    }
    inflateEnd(&zs);
    out.resize(err.empty() ? used : 0);
    return err;
}

}  // namespace nwi

extern "C" const char* nwi_last_error(void) { return nwi::g_err.c_str(); }

extern "C" void nwi_release(nwi_records* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    for (void* p : r->bufs) (void)hipFree(p);
    delete r;
}

extern "C" int nwi_parse_text(int device, const uint8_t* text, int64_t bytes, nwi_records** out) {
    return nwi::parse("nwi_parse_text", device, text, bytes, 0.0f, out);
}

extern "C" int nwi_parse_file(int device, const char* path, nwi_records** out) {
    using namespace nwi;
    const char* who = "nwi_parse_file";
    if (!path || !out) return fail(-1, "nwi_parse_file: null argument");
    *out = nullptr;
    FileMap in;
    const int got = in.open_file(path);
    if (got < 0) return fail(-1, std::string("nwi_parse_file: cannot read ") + path);
    if (got == 0) return parse(who, device, nullptr, 0, 0.0f, out);
    if (!(in.n >= 2 && in.p[0] == 0x1f && in.p[1] == 0x8b)) {
        if ((uint64_t)in.n >= kMaxText)   // before the cast below
            return fail(-3, "nwi_parse_file: a text of 2^32 - 16 bytes or more in one call is out of scope (nothing is truncated)");
        return parse(who, device, in.p, (int64_t)in.n, 0.0f, out);
    }
    const auto t0 = std::chrono::steady_clock::now();
    auto ms_since = [&]() {
        return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    nw_gz::Buffer whole;   // one member, decoded by all the pool's threads (gz_inflate.h)
    if (nw_gz::inflate_parallel(in.p, in.n, nw_host::Pool::get().threads(), nullptr, &whole)) {
        const float ms = ms_since();
        const int rc = (uint64_t)whole.n >= kMaxText
                           ? fail(-3, "nwi_parse_file: the inflated text reaches 2^32 - 16 bytes: out of scope (nothing is truncated)")
                           : parse(who, device, whole.p, (int64_t)whole.n, ms, out);
        whole.release();
        return rc;
    }
    std::vector<unsigned char> text;
    const std::string err = inflate_members(in.p, in.n, text);
    if (!err.empty()) return fail(err.find("out of scope") != std::string::npos ? -3 : -1, "nwi_parse_file: " + err);
    return parse(who, device, text.data(), (int64_t)text.size(), ms_since(), out);
}

extern "C" int nwi_info(const nwi_records* r, nwi_summary* out) {
    if (!r || !out) return nwi::fail(-1, "nwi_info: null argument");
    *out = r->info;
    return 0;
}

extern "C" int nwi_fetch(const nwi_records* r, uint8_t* flags, uint8_t* seq, int64_t* seq_off, uint8_t* qual,
                         int64_t* qual_off, uint8_t* names, int64_t* name_off) {
    using namespace nwi;
    if (!r) return fail(-1, "nwi_fetch: no records");
    const nwi_summary& I = r->info;
    int64_t* const offs[3] = {seq_off, qual_off, name_off};
    uint8_t* const streams[3] = {seq, qual, names};
    const int64_t size[3] = {I.seq_bytes, I.qual_bytes, I.name_bytes};
    if (I.n == 0) {
        for (int q = 0; q < 3; ++q)
            if (offs[q]) offs[q][0] = 0;
        return 0;
    }
    if (hipSetDevice(r->device) != hipSuccess) return fail(-4, "nwi_fetch: hipSetDevice failed");
    bool ok = true;
    auto get = [&](void* dst, const void* d, size_t bytes) {
        if (dst && bytes && ok) ok = hipMemcpy(dst, d, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    };
    get(flags, r->flags, (size_t)I.n);
    for (int q = 0; q < 3; ++q) {
        get(streams[q], r->stream[q], (size_t)size[q]);
        get(offs[q], r->off[q], sizeof(int64_t) * (size_t)(I.n + 1));
    }
    if (!ok) return fail(-4, std::string("nwi_fetch: HIP error: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}
