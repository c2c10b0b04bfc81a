// nw_alleles.hip -- groups of byte-identical reads of a device-resident batch (gfx950), the
// per-read half of CRISPResso's allele table (CRISPRessoCORE.py:2923-2946), behind the C ABI of
// include/crispr_alleles.h; and the same grouping on host text (nwa_group_host).
//
// Device pass (nwa_group_device), every kernel launched once on the context's stream:
//   hash     one wavefront per read: a 64-bit polynomial in the read's dwords (lane l takes
//            dwords l, l + 64, ...: 256 B per step, coalesced; aligned dword loads shifted to the
//            read's start, so no load touches a word without a byte of the batch), summed across
//            the lanes, finished with the length and the tag, forced nonzero (0 = not kept).
//   insert   one lane per read: the lanes of a wavefront that share a hash elect their lowest
//            lane (ballot loop), which claims the hash's slot of an open-addressing table
//            (64-bit CAS, linear probing bounded by the table size) and adds the lanes' count
//            once: atomicMin(first) / atomicAdd(count) make the slot's content independent of
//            the order of arrival.
//   verify   one wavefront per read: a read that is not its slot's first is compared with it
//            (tag, length, bytes); a read that differs (equal hashes, different reads) goes to
//            the collided list, which the host groups exactly.
//   compact  is_first -> exclusive scan (tile sums, one block over the sums, tiles again) -> the
//            groups in order of first appearance, and every read's group.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "group_device.h"
#include "host_pool.h"
#include "nwa_device.h"

namespace nwa {

using grp::fmix64;
using grp::kLenMul;
using grp::kPoly;
using grp::load_dword;
using grp::shfl_xor64;

constexpr uint64_t kTagMul = 0x165667B19E3779F9ull;
constexpr int kTile = 2048;                            // flags per block of the scan (256 threads x 8)

// The hash of a read from the sum of its dword terms: length and tag mixed in, cut to the
// low `bits` bits (CRISPR_NWA_HASH_BITS), never 0.
__host__ __device__ inline uint64_t finish_hash(uint64_t poly, int64_t len, int32_t tag, uint64_t mask) {
    uint64_t h = fmix64(poly ^ ((uint64_t)len * kLenMul) ^ ((uint64_t)(uint32_t)tag * kTagMul + 1));
    h &= mask;
    return h ? h : 1;
}

struct Args {
    const uint8_t* reads;      // read r at reads + off[r] - bias
    const int64_t* off;
    int64_t bias;
    int64_t n;
    const uint8_t* keep;       // device copies (or null)
    const int32_t* tag;
    uint64_t* hash;            // [n] 0 = not kept
    uint32_t* slot;            // [n] the read's table slot
    uint8_t* is_first;         // [n rounded up to kTile]
    unsigned long long* key;   // table: [cap]
    uint32_t* first;
    uint32_t* count;
    uint32_t* gid;             // [cap] the slot's group
    uint64_t cap_mask;
    int shift;                 // 64 - log2(cap)
    uint64_t hash_mask;
    uint32_t* coll;            // [n] collided reads, any order
    uint32_t* counters;        // [0] groups, [1] collided, [2] error word
    uint32_t* tile_sum;        // [tiles]
    uint32_t* tile_off;
    uint32_t* gfirst;          // [groups]
    uint32_t* gcount;
    int32_t* gor;              // [n]
};

__global__ __launch_bounds__(256) void hash_kernel(Args a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    uint64_t p1 = kPoly, p64 = 1;                      // kPoly^(lane + 1), kPoly^64
    for (int i = 0; i < lane; ++i) p1 *= kPoly;
    for (int i = 0; i < 64; ++i) p64 *= kPoly;
    for (int64_t r = wave; r < a.n; r += nwaves) {
        if (a.keep && !a.keep[r]) {
            if (lane == 0) a.hash[r] = 0;
            continue;
        }
        const int64_t o0 = a.off[r], L = a.off[r + 1] - o0;
        const uint8_t* p = a.reads + (o0 - a.bias);
        const int64_t nd = (L + 3) >> 2;
        uint64_t acc = 0, pw = p1;
        for (int64_t k = lane; k < nd; k += 64) {
            acc += (uint64_t)load_dword(p, k, L) * pw;
            pw *= p64;
        }
        for (int o = 32; o > 0; o >>= 1) acc += shfl_xor64(acc, o);
        if (lane == 0) a.hash[r] = finish_hash(acc, L, a.tag ? a.tag[r] : 0, a.hash_mask);
    }
}

__global__ __launch_bounds__(256) void insert_kernel(Args a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t h = r < a.n ? a.hash[r] : 0;
    // the lanes that share a hash elect the lowest of them (the smallest read index)
    int lead;
    const uint32_t cnt = grp::wave_elect(h, h != 0, &lead);
    uint32_t found = 0;
    if (cnt) {
        const uint64_t s = grp::claim_slot(a.key, a.first, a.count, h, (uint32_t)r, cnt, a.shift, a.cap_mask);
        if (s == grp::kNoSlot) a.counters[2] = 1;      // a full table: cannot happen at load <= 1/2; the host reports it
        else found = (uint32_t)s;                      // (slot 0 otherwise)
    }
    found = (uint32_t)__shfl((int)found, lead, 64);
    if (h != 0) a.slot[r] = found;
}

__global__ __launch_bounds__(256) void verify_kernel(Args a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t r = wave; r < a.n; r += nwaves) {
        if (a.hash[r] == 0) continue;                       // is_first stays 0
        const int64_t f = a.first[a.slot[r]];
        if (f == r) {
            if (lane == 0) a.is_first[r] = 1;
            continue;
        }
        if (f > r) {                                        // (only after a failed insert)
            if (lane == 0) a.counters[2] = 1;
            continue;
        }
        const int64_t o0 = a.off[r], L = a.off[r + 1] - o0;
        const int64_t g0 = a.off[f], Lf = a.off[f + 1] - g0;
        bool diff = L != Lf || (a.tag && a.tag[r] != a.tag[f]);
        if (!diff) {
            const uint8_t* p = a.reads + (o0 - a.bias);
            const uint8_t* q = a.reads + (g0 - a.bias);
            const int64_t nd = (L + 3) >> 2;
            for (int64_t k = lane; k < nd; k += 64) diff |= load_dword(p, k, L) != load_dword(q, k, L);
        }
        if (__ballot(diff) && lane == 0) a.coll[atomicAdd(&a.counters[1], 1u)] = (uint32_t)r;
    }
}

// Exclusive scan of one value per thread over a block of NW wavefronts; *total = the block's sum.
template <int NW>
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* total) {
    __shared__ uint32_t wsum[NW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64);
        if (lane >= o) x += y;
    }
    __syncthreads();                                        // (a previous call's wsum is consumed)
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int i = 0; i < NW; ++i) {
        if (i < w) before += wsum[i];
        all += wsum[i];
    }
    *total = all;
    return before + x - v;
}

// the 8 flags of thread t of tile b (is_first is padded to whole tiles and zeroed)
__device__ inline uint64_t tile_flags(const Args& a) {
    return *reinterpret_cast<const uint64_t*>(a.is_first + ((int64_t)blockIdx.x * kTile + threadIdx.x * 8));
}

__global__ __launch_bounds__(256) void tile_sum_kernel(Args a) {
    uint32_t total;
    block_scan<4>((uint32_t)__popcll(tile_flags(a)), &total);
    if (threadIdx.x == 0) a.tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void tile_scan_kernel(Args a, int64_t tiles) {
    uint32_t carry = 0;
    for (int64_t base = 0; base < tiles; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const uint32_t v = i < tiles ? a.tile_sum[i] : 0;
        uint32_t total;
        const uint32_t ex = block_scan<16>(v, &total);
        if (i < tiles) a.tile_off[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) a.counters[0] = carry;
}

__global__ __launch_bounds__(256) void emit_kernel(Args a) {
    const uint64_t fl = tile_flags(a);
    uint32_t total;
    uint32_t g = a.tile_off[blockIdx.x] + block_scan<4>((uint32_t)__popcll(fl), &total);
    const int64_t r0 = (int64_t)blockIdx.x * kTile + threadIdx.x * 8;
    for (int j = 0; j < 8; ++j) {
        if ((fl >> (8 * j)) & 1) {
            const int64_t r = r0 + j;                       // < n: the padding holds no flag
            const uint32_t s = a.slot[r];
            a.gfirst[g] = (uint32_t)r;
            a.gcount[g] = a.count[s];
            a.gid[s] = g;
            ++g;
        }
    }
}

__global__ __launch_bounds__(256) void assign_kernel(Args a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < a.n) a.gor[r] = a.hash[r] ? (int32_t)a.gid[a.slot[r]] : -1;
}

__global__ __launch_bounds__(256) void coll_info_kernel(Args a, const uint32_t* list, int64_t m, CollInfo* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int64_t r = list[i];
    CollInfo c;
    c.start = a.off[r] - a.bias;
    c.len = a.off[r + 1] - a.off[r];
    c.tag = a.tag ? a.tag[r] : 0;
    c.group = (int32_t)a.gid[a.slot[r]];
    out[i] = c;
}

// The non-zero bytes of keep[n]: a sum per block, one atomic per block (an integer sum: the same
// total in any order; n < 2^31).
__global__ __launch_bounds__(256) void count_kept_kernel(const uint8_t* keep, int64_t n, uint32_t* total) {
    uint32_t v = 0;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) v += keep[r] != 0;
    uint32_t sum;
    block_scan<4>(v, &sum);
    if (threadIdx.x == 0 && sum) atomicAdd(total, sum);
}

}  // namespace nwa

namespace {

using hd::fail;

// Groups of the collided reads (sorted by read index) by (tag, bytes), in order of first
// appearance: grp[i] = the group of collided read i, gfirst / gcount per group.
void group_collided(const std::vector<nwa::CollInfo>& info, const std::vector<int64_t>& byte_off,
                    const std::vector<char>& bytes, std::vector<int64_t>* grp, std::vector<int64_t>* gcount) {
    std::map<std::pair<int32_t, std::string>, int64_t> seen;
    grp->resize(info.size());
    gcount->clear();
    for (size_t i = 0; i < info.size(); ++i) {
        std::pair<int32_t, std::string> key(info[i].tag,
                                            std::string(bytes.data() + byte_off[i], (size_t)info[i].len));
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(std::move(key), (int64_t)gcount->size()).first;
            gcount->push_back(0);
        }
        (*grp)[i] = it->second;
        ++(*gcount)[(size_t)it->second];
    }
}

uint64_t host_hash(const unsigned char* p, int64_t n, int32_t tag) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n ^ ((uint64_t)(uint32_t)tag * nwa::kTagMul);
    int64_t k = 0;
    for (; k + 8 <= n; k += 8) {
        uint64_t w;
        std::memcpy(&w, p + k, 8);
        h = (h ^ w) * 0xFF51AFD7ED558CCDull;
        h ^= h >> 32;
    }
    uint64_t w = 0;
    std::memcpy(&w, p + k, (size_t)(n - k));
    h = (h ^ w) * 0xC4CEB9FE1A85EC53ull;
    return h ^ (h >> 29);
}

}  // namespace

namespace nwa {

int count_kept(nwa_ctx* c, const uint8_t* d_keep, int64_t n, int64_t* kept) {
    *kept = n;
    if (!d_keep || n <= 0) return NW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_counters.reserve(4));
    hipStream_t st = c->stream;
    HIP_TRY(c, hipMemsetAsync(c->d_counters.p, 0, sizeof(uint32_t) * 4, st));
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)16 * c->num_cus);
    hipLaunchKernelGGL(count_kept_kernel, dim3(grid), dim3(256), 0, st, d_keep, n, c->d_counters.p + 3);
    HIP_TRY(c, hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, c->d_counters.p + 3, sizeof total, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if ((int64_t)total > n) return fail(c, NW_E_STATE, "inconsistent kept count");
    *kept = total;
    return NW_OK;
}

int group_resident(nwa_ctx* c, const uint8_t* d_reads, const int64_t* d_offsets, int64_t reads_bias, int64_t n,
                   const uint8_t* d_keep, int64_t kept, const int32_t* tag, int64_t* first, int64_t* count,
                   int64_t cap, int32_t* group_of_read, int64_t* n_groups, float* kernel_ms) {
    c->collided = 0;
    std::fill(c->phase_ms, c->phase_ms + 4, 0.0f);
    if (kernel_ms) *kernel_ms = 0.0f;
    *n_groups = 0;
    if (kept == 0) {
        if (group_of_read) std::fill(group_of_read, group_of_read + n, -1);
        return NW_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const grp::TableGeometry tg = grp::table_geometry(kept, c->hash_bits);
    const size_t slots = tg.slots;
    const int64_t tiles = (n + nwa::kTile - 1) / nwa::kTile;
    const size_t padded = (size_t)tiles * nwa::kTile;
    HIP_TRY(c, c->d_hash.reserve((size_t)n));
    HIP_TRY(c, c->d_slot.reserve((size_t)n));
    HIP_TRY(c, c->d_is_first.reserve(padded));
    HIP_TRY(c, c->d_key.reserve(slots));
    HIP_TRY(c, c->d_first.reserve(slots));
    HIP_TRY(c, c->d_count.reserve(slots));
    HIP_TRY(c, c->d_gid.reserve(slots));
    HIP_TRY(c, c->d_coll.reserve((size_t)kept));
    HIP_TRY(c, c->d_counters.reserve(4));
    HIP_TRY(c, c->d_tile_sum.reserve((size_t)tiles));
    HIP_TRY(c, c->d_tile_off.reserve((size_t)tiles));
    HIP_TRY(c, c->d_gfirst.reserve((size_t)kept));
    HIP_TRY(c, c->d_gcount.reserve((size_t)kept));
    HIP_TRY(c, c->d_gor.reserve((size_t)n));
    if (tag) {
        HIP_TRY(c, c->d_tag.reserve((size_t)n));
        HIP_TRY(c, hipMemcpy(c->d_tag.p, tag, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    }
    nwa::Args a;
    a.reads = d_reads;
    a.off = d_offsets;
    a.bias = reads_bias;
    a.n = n;
    a.keep = d_keep;
    a.tag = tag ? c->d_tag.p : nullptr;
    a.hash = c->d_hash.p;
    a.slot = c->d_slot.p;
    a.is_first = c->d_is_first.p;
    a.key = c->d_key.p;
    a.first = c->d_first.p;
    a.count = c->d_count.p;
    a.gid = c->d_gid.p;
    a.cap_mask = tg.cap_mask;
    a.shift = tg.shift;
    a.hash_mask = tg.hash_mask;
    a.coll = c->d_coll.p;
    a.counters = c->d_counters.p;
    a.tile_sum = c->d_tile_sum.p;
    a.tile_off = c->d_tile_off.p;
    a.gfirst = c->d_gfirst.p;
    a.gcount = c->d_gcount.p;
    a.gor = c->d_gor.p;

    hipStream_t st = c->stream;
    HIP_TRY(c, hipMemsetAsync(a.key, 0, sizeof(unsigned long long) * slots, st));
    HIP_TRY(c, hipMemsetAsync(a.first, 0xFF, sizeof(uint32_t) * slots, st));
    HIP_TRY(c, hipMemsetAsync(a.count, 0, sizeof(uint32_t) * slots, st));
    HIP_TRY(c, hipMemsetAsync(a.is_first, 0, padded, st));
    HIP_TRY(c, hipMemsetAsync(a.counters, 0, sizeof(uint32_t) * 4, st));
    const unsigned wave_grid = (unsigned)std::min<int64_t>((n + 3) / 4, (int64_t)16 * c->num_cus);
    const unsigned lane_grid = (unsigned)((n + 255) / 256);
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(nwa::hash_kernel, dim3(wave_grid), dim3(256), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    hipLaunchKernelGGL(nwa::insert_kernel, dim3(lane_grid), dim3(256), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[2], st));
    hipLaunchKernelGGL(nwa::verify_kernel, dim3(wave_grid), dim3(256), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[3], st));
    hipLaunchKernelGGL(nwa::tile_sum_kernel, dim3((unsigned)tiles), dim3(256), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(nwa::tile_scan_kernel, dim3(1), dim3(1024), 0, st, a, tiles);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(nwa::emit_kernel, dim3((unsigned)tiles), dim3(256), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(nwa::assign_kernel, dim3(lane_grid), dim3(256), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[4], st));
    uint32_t ctr[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(ctr, a.counters, sizeof ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    for (int i = 0; i < 4; ++i) HIP_TRY(c, hipEventElapsedTime(&c->phase_ms[i], c->ev[i], c->ev[i + 1]));
    if (kernel_ms) HIP_TRY(c, hipEventElapsedTime(kernel_ms, c->ev[0], c->ev[4]));
    if (ctr[2]) return fail(c, NW_E_STATE, "the hash table's probe bound was reached (%zu slots, %lld reads)", slots,
                            (long long)kept);
    const int64_t ng_dev = ctr[0], nc = ctr[1];
    if (ng_dev > kept || nc > kept) return fail(c, NW_E_STATE, "inconsistent group count");

    // the collided reads (equal hashes, different bytes): grouped exactly here
    std::vector<uint32_t> coll((size_t)nc);
    std::vector<nwa::CollInfo> info((size_t)nc);
    std::vector<int64_t> cgrp, cg_count, cg_first;
    if (nc > 0) {
        HIP_TRY(c, hipMemcpy(coll.data(), a.coll, sizeof(uint32_t) * (size_t)nc, hipMemcpyDeviceToHost));
        std::sort(coll.begin(), coll.end());
        HIP_TRY(c, hipMemcpy(a.coll, coll.data(), sizeof(uint32_t) * (size_t)nc, hipMemcpyHostToDevice));
        HIP_TRY(c, c->d_info.reserve((size_t)nc));
        hipLaunchKernelGGL(nwa::coll_info_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, a, a.coll, nc,
                           c->d_info.p);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(info.data(), c->d_info.p, sizeof(nwa::CollInfo) * (size_t)nc, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        std::vector<int64_t> byte_off((size_t)nc + 1, 0);
        for (int64_t i = 0; i < nc; ++i) {
            if (info[(size_t)i].len < 0 || info[(size_t)i].group < 0 || info[(size_t)i].group >= ng_dev)
                return fail(c, NW_E_STATE, "inconsistent collided read");
            byte_off[(size_t)i + 1] = byte_off[(size_t)i] + info[(size_t)i].len;
        }
        std::vector<char> bytes((size_t)std::max<int64_t>(byte_off[(size_t)nc], 1));
        for (int64_t i = 0; i < nc; ++i)
            if (info[(size_t)i].len > 0)
                HIP_TRY(c, hipMemcpyAsync(bytes.data() + byte_off[(size_t)i], d_reads + info[(size_t)i].start,
                                          (size_t)info[(size_t)i].len, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        group_collided(info, byte_off, bytes, &cgrp, &cg_count);
        cg_first.assign(cg_count.size(), -1);
        for (int64_t i = 0; i < nc; ++i)
            if (cg_first[(size_t)cgrp[(size_t)i]] < 0) cg_first[(size_t)cgrp[(size_t)i]] = coll[(size_t)i];
    }
    c->collided = nc;
    const int64_t ng_new = (int64_t)cg_count.size(), ng = ng_dev + ng_new;
    *n_groups = ng;
    if (ng > cap) return fail(c, NW_E_CAPACITY, "%lld groups, capacity %lld", (long long)ng, (long long)cap);
    std::vector<uint32_t> gf((size_t)ng_dev), gc((size_t)ng_dev);
    HIP_TRY(c, hipMemcpy(gf.data(), a.gfirst, sizeof(uint32_t) * (size_t)ng_dev, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(gc.data(), a.gcount, sizeof(uint32_t) * (size_t)ng_dev, hipMemcpyDeviceToHost));
    if (group_of_read) HIP_TRY(c, hipMemcpy(group_of_read, a.gor, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    if (nc == 0) {
        for (int64_t g = 0; g < ng_dev; ++g) {
            first[g] = gf[(size_t)g];
            count[g] = gc[(size_t)g];
        }
        return NW_OK;
    }
    for (int64_t i = 0; i < nc; ++i) --gc[(size_t)info[(size_t)i].group];
    // merge the two lists (both ascending in first) into the order of first appearance
    std::vector<int64_t> dev_id((size_t)ng_dev), new_id((size_t)ng_new);
    int64_t i = 0, j = 0, g = 0;
    while (i < ng_dev || j < ng_new) {
        if (j >= ng_new || (i < ng_dev && (int64_t)gf[(size_t)i] < cg_first[(size_t)j])) {
            first[g] = gf[(size_t)i];
            count[g] = gc[(size_t)i];
            dev_id[(size_t)i++] = g++;
        } else {
            first[g] = cg_first[(size_t)j];
            count[g] = cg_count[(size_t)j];
            new_id[(size_t)j++] = g++;
        }
    }
    if (group_of_read) {
        for (int64_t r = 0; r < n; ++r)
            if (group_of_read[r] >= 0) group_of_read[r] = (int32_t)dev_id[(size_t)group_of_read[r]];
        for (int64_t k = 0; k < nc; ++k) group_of_read[coll[(size_t)k]] = (int32_t)new_id[(size_t)cgrp[(size_t)k]];
    }
    return NW_OK;
}

}  // namespace nwa

extern "C" {

int nwa_create(int device, nwa_ctx** out) {
    const int rc = hd::create_context(device, nwa::kEvents, out);
    if (rc != NW_OK) return rc;
    nwa_ctx* c = *out;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cus = prop.multiProcessorCount;
    c->hash_bits = grp::env_hash_bits("CRISPR_NWA_HASH_BITS");
    return NW_OK;
}

void nwa_destroy(nwa_ctx* c) { hd::destroy_context(c); }

const char* nwa_last_error(const nwa_ctx* c) { return c ? c->err.c_str() : "null context"; }

int64_t nwa_last_collided(const nwa_ctx* c) { return c ? c->collided : -1; }

int nwa_phase_times(const nwa_ctx* c, float* ms) {
    if (!c || !ms) return NW_E_INVALID;
    std::memcpy(ms, c->phase_ms, sizeof c->phase_ms);
    return NW_OK;
}

int64_t nwa_reads_per_step(const nwa_ctx* c) { return c ? (int64_t)4 * 16 * c->num_cus : -1; }

int nwa_group_device(nwa_ctx* c, const uint8_t* d_reads, const int64_t* d_offsets, int64_t reads_bias, int64_t n,
                     const uint8_t* keep, const int32_t* tag, int64_t* first, int64_t* count, int64_t cap,
                     int32_t* group_of_read, int64_t* n_groups, float* kernel_ms) {
    if (!c) return NW_E_INVALID;
    if (n < 0 || n > 0x7FFFFFFFll) return fail(c, NW_E_INVALID, "read count %lld out of range", (long long)n);
    if (!n_groups || cap < 0 || (cap > 0 && (!first || !count)))
        return fail(c, NW_E_INVALID, "null output array");
    if (n > 0 && (!d_reads || !d_offsets)) return fail(c, NW_E_INVALID, "null device array");
    int64_t kept = n;
    if (keep) {
        kept = 0;
        for (int64_t r = 0; r < n; ++r) kept += keep[r] != 0;
    }
    if (keep && kept > 0) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, c->d_keep.reserve((size_t)n));
        HIP_TRY(c, hipMemcpy(c->d_keep.p, keep, (size_t)n, hipMemcpyHostToDevice));
    }
    return nwa::group_resident(c, d_reads, d_offsets, reads_bias, n, keep ? c->d_keep.p : nullptr, kept, tag, first, count,
                               cap, group_of_read, n_groups, kernel_ms);
}

int nwa_group_host(const char* reads, const int64_t* offsets, int64_t n, const uint8_t* keep, const int32_t* tag,
                   int64_t* first, int64_t* count, int64_t cap, int32_t* group_of_read, int64_t* n_groups,
                   int32_t nthreads) {
    if (n < 0 || n > 0x7FFFFFFFll || !n_groups || cap < 0 || (cap > 0 && (!first || !count)) ||
        (n > 0 && (!reads || !offsets)))
        return NW_E_INVALID;
    *n_groups = 0;
    if (n == 0) return NW_OK;
    nw_host::Pool& pool = nw_host::Pool::get();
    int P = nthreads > 0 ? std::min((int)nthreads, pool.threads()) : pool.threads();
    P = (int)std::max<int64_t>(1, std::min<int64_t>(P, n / 8192 + 1));
    auto kept = [&](int64_t r) { return !keep || keep[r]; };
    std::vector<uint64_t> h((size_t)n);
    pool.run(P, [&](int k) {
        int64_t lo, hi;
        nw_host::Pool::range(n, P, k, &lo, &hi);
        for (int64_t r = lo; r < hi; ++r)
            if (kept(r))
                h[(size_t)r] = host_hash((const unsigned char*)reads + offsets[r], offsets[r + 1] - offsets[r],
                                         tag ? tag[r] : 0);
    });
    // one open-addressing table per hash partition, its reads visited in read order: rep[r] = the
    // first read of r's group, size[] counted at the first (a group lies in one partition)
    std::vector<int64_t> rep((size_t)n, -1), size((size_t)n, 0);
    pool.run(P, [&](int part) {
        int64_t cnt = 0;
        for (int64_t r = 0; r < n; ++r) cnt += kept(r) && (int)(h[(size_t)r] % (uint64_t)P) == part;
        size_t tcap = 16;
        while (tcap < (size_t)(2 * cnt + 16)) tcap <<= 1;
        std::vector<int64_t> slot(tcap, -1);
        for (int64_t r = 0; r < n; ++r) {
            const uint64_t hr = h[(size_t)r];
            if (!kept(r) || (int)(hr % (uint64_t)P) != part) continue;
            const int64_t Lr = offsets[r + 1] - offsets[r];
            for (size_t s = (size_t)(hr >> 24) & (tcap - 1);; s = (s + 1) & (tcap - 1)) {
                const int64_t q = slot[s];
                if (q < 0) {
                    slot[s] = r;
                    rep[(size_t)r] = r;
                    size[(size_t)r] = 1;
                    break;
                }
                if (h[(size_t)q] == hr && offsets[q + 1] - offsets[q] == Lr && (!tag || tag[q] == tag[r]) &&
                    std::memcmp(reads + offsets[q], reads + offsets[r], (size_t)Lr) == 0) {
                    rep[(size_t)r] = q;
                    ++size[(size_t)q];
                    break;
                }
            }
        }
    });
    int64_t ng = 0;
    for (int64_t r = 0; r < n; ++r) ng += rep[(size_t)r] == r;
    *n_groups = ng;
    if (ng > cap) return NW_E_CAPACITY;
    int64_t g = 0;
    for (int64_t r = 0; r < n; ++r) {
        if (rep[(size_t)r] != r) continue;
        first[g] = r;
        count[g] = size[(size_t)r];
        size[(size_t)r] = g++;      // from here on: the group of the first
    }
    if (group_of_read)
        for (int64_t r = 0; r < n; ++r)
            group_of_read[r] = rep[(size_t)r] < 0 ? -1 : (int32_t)size[(size_t)rep[(size_t)r]];
    return NW_OK;
}

int nwa_reads_have_lower(const char* reads, const int64_t* offsets, int64_t n, int32_t nthreads) {
    if (n < 0 || (n > 0 && (!reads || !offsets))) return NW_E_INVALID;
    if (n == 0) return 0;
    const int64_t b0 = offsets[0], nb = offsets[n] - b0;
    if (nb < 0) return NW_E_INVALID;
    nw_host::Pool& pool = nw_host::Pool::get();
    int P = nthreads > 0 ? std::min((int)nthreads, pool.threads()) : pool.threads();
    P = (int)std::max<int64_t>(1, std::min<int64_t>(P, nb / (1 << 20) + 1));
    std::atomic<int> any{0};
    pool.run(P, [&](int k) {
        int64_t lo, hi;
        nw_host::Pool::range(nb, P, k, &lo, &hi);
        const unsigned char* p = (const unsigned char*)reads + b0;
        int hit = 0;
        for (int64_t i = lo; i < hi; ++i) hit |= (unsigned)(p[i] - 'a') < 26u;
        if (hit) any.store(1, std::memory_order_relaxed);
    });
    return any.load();
}

}  // extern "C"
