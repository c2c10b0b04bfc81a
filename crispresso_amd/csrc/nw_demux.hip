// nw_demux.hip -- pooled-amplicon demultiplexing on host reads (gfx950): the bowtie2 step of
// CRISPRessoPooled's ONLY_AMPLICONS mode (CRISPRessoPooledCORE.py:843-878) as the exact window
// vote of include/crispr_demux.h, behind that header's C ABI.
//
// Every kernel is launched on the context's stream:
//   index    one lane per amplicon position: the 2-bit key of the k bases from there (none when
//            the window leaves the amplicon or holds a break), bit 62 set so that it is never 0.
//            The key claims a slot of an open-addressing table (16 bytes a slot: key, value) by
//            a 64-bit CAS, linear probing bounded by the table size, load <= 1/2; the value is
//            set by CAS(EMPTY -> g), and any lane that finds another amplicon there stores
//            AMBIGUOUS: the final table does not depend on the order of arrival.
//   census   the occupied and the ambiguous slots, counted (n_windows, n_ambiguous).
//   assign   one wavefront per read.  A lane takes a contiguous stretch of ceil(windows / 64)
//            window positions: it rolls the forward and the reverse-complement key over the
//            k - 1 bases before its first window, then one base per step, breaks included, and
//            probes both keys.  The candidates (2 g + strand) of a step are tallied in the
//            wavefront's LDS table of `slots` entries: the lanes with one candidate elect their
//            lowest lane (wave_elect), which claims the candidate's entry (LDS CAS, probing
//            bounded by `slots`) and adds the group's size.  best and rival are a wave reduction
//            over that table.  A read with more distinct candidates than entries goes to the
//            fallback list (wave_reserve) and is decided by the same rule on the host.
//   gather   one wavefront per assigned read: its bytes copied, or reversed and complemented,
//            to their place in the grouped text.  The counts' prefix sum and each read's rank in
//            its group (ascending input index) are one pass of the host over `which`.
//   pack     nw_pack_reads (nw_pack.cpp) of the gathered text without that text: a thread a dword
//            of the 2-bit stream.  It finds the read that holds gathered position 16 w by a
//            bounded binary search of dst, takes its 16 bytes from the resident input (one 16-B
//            load when they lie in one read; reversed for a strand-1 read, whose complement is
//            code ^ 2), and writes the dword once, whole: an exception or a position past the end
//            gives 0 bits.  The block's exceptions go to sums[]; one block scans the sums; if
//            there are any, the exceptions kernel walks the same dwords and writes (position,
//            byte) at the block's base + the block scan of the threads' counts: ascending
//            positions, a function of the input alone.  No atomics, no zeroed buffer, nothing
//            handed between blocks inside a launch.  Sums are 32-bit: 2^32 or more gathered
//            bytes are refused.  bounds: a thread a group, the first exception at or after the
//            group's first position (binary search of the exception list).
// The reads are uploaded in chunks into one text buffer that stays resident for the gather, the
// packer and, through nwd_adopt_group, the aligner (nw_front::set_packed_batch on a slice).
// nwd_assign_prepared fills that buffer from the front end's merged text in HBM instead
// (nw_front::view_prepared): the chunks' copies are device to device, nothing else differs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/crispr_demux.h"
#include "../../include/crispr_nw.h"
#include "front_device.h"
#include "group_device.h"
#include "host_dev.h"
#include "nw_device.h"

namespace nwd {

using grp::kPoly;

constexpr int64_t kChunkBytes = (int64_t)64 << 20;     // text per chunk by default
constexpr int64_t kChunkReads = (int64_t)4 << 20;      // and no more reads than this
constexpr uint64_t kKeyBit = 1ull << 62;               // set in every key: a key is never 0
constexpr unsigned long long kEmpty = ~0ull;           // a claimed slot's value before its amplicon
constexpr unsigned long long kAmbiguous = ~0ull - 1;   // the window of two or more amplicons
constexpr int32_t kNone = -1;                          // no candidate / a free tally entry
enum { kError = 0, kFallback = 1, kWindows = 2, kAmbig = 3, kCounters = 4 };

// 0..3 for A C G T in either case, 4 (a break) for every other byte.
__host__ __device__ inline int base_code(uint8_t c) {
    switch (c | 0x20) {
        case 'a': return 0;
        case 'c': return 1;
        case 'g': return 2;
        case 't': return 3;
        default: return 4;
    }
}

__host__ __device__ inline uint8_t complement(uint8_t c) {
    switch (c) {
        case 'A': return 'T';
        case 'C': return 'G';
        case 'G': return 'C';
        case 'T': return 'A';
        case 'a': return 't';
        case 'c': return 'g';
        case 'g': return 'c';
        case 't': return 'a';
        default: return c;
    }
}

// The forward and reverse-complement keys of the last k bases and the number of bases since the
// last break: the window that ends at the pushed base is break-free iff run >= k.
struct Roll {
    uint64_t fwd = 0, rc = 0;
    int run = 0;
    __host__ __device__ inline void push(uint8_t c, int k, uint64_t mask) {
        const int b = base_code(c);
        if (b > 3) {
            run = 0;
            return;
        }
        fwd = ((fwd << 2) | (uint64_t)b) & mask;
        rc = (rc >> 2) | ((uint64_t)(3 - b) << (2 * (k - 1)));
        ++run;
    }
};

struct IndexArgs {
    const uint8_t* refs;        // the amplicons, concatenated
    const int64_t* roff;        // [n_refs + 1], roff[0] == 0
    int32_t n_refs, k;
    int64_t total;
    unsigned long long* tab;    // [2 * slots]: key (0 = empty), value
    uint64_t cap_mask;
    int shift;                  // 64 - log2(slots)
    uint32_t* counters;
};

__global__ __launch_bounds__(256) void nwd_clear_kernel(IndexArgs a) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > a.cap_mask) return;
    a.tab[2 * s] = 0;
    a.tab[2 * s + 1] = kEmpty;
}

__global__ __launch_bounds__(256) void nwd_index_kernel(IndexArgs a) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.total) return;
    int lo = 0, hi = a.n_refs;                   // the last g with roff[g] <= p (empty amplicons skipped)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.roff[mid] <= p) lo = mid; else hi = mid;
    }
    const int g = lo;
    if (p + a.k > a.roff[g + 1]) return;
    const uint64_t mask = (1ull << (2 * a.k)) - 1ull;
    Roll w;
    for (int i = 0; i < a.k; ++i) w.push(a.refs[p + i], a.k, mask);
    if (w.run < a.k) return;
    const unsigned long long key = w.fwd | kKeyBit;
    uint64_t s = (key * kPoly) >> a.shift;
    bool placed = false;
    for (uint64_t probe = 0; probe <= a.cap_mask; ++probe) {      // bounded by the table size
        unsigned long long cur = __hip_atomic_load(&a.tab[2 * s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) cur = atomicCAS(&a.tab[2 * s], 0ull, key);
        if (cur == 0 || cur == key) {
            const unsigned long long old = atomicCAS(&a.tab[2 * s + 1], kEmpty, (unsigned long long)g);
            if (old != kEmpty && old != (unsigned long long)g) atomicExch(&a.tab[2 * s + 1], kAmbiguous);
            placed = true;
            break;
        }
        s = (s + 1) & a.cap_mask;
    }
    if (!placed) a.counters[kError] = 1;          // a full table: cannot happen at load <= 1/2
}

__global__ __launch_bounds__(256) void nwd_census_kernel(IndexArgs a) {
    const int lane = threadIdx.x & 63;
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool used = s <= a.cap_mask && a.tab[2 * s] != 0;
    const bool amb = used && a.tab[2 * s + 1] == kAmbiguous;
    const unsigned long long ub = __ballot(used), ab = __ballot(amb);
    if (lane == 0 && ub) atomicAdd(&a.counters[kWindows], (uint32_t)__popcll(ub));
    if (lane == 0 && ab) atomicAdd(&a.counters[kAmbig], (uint32_t)__popcll(ab));
}

struct AssignArgs {
    const uint8_t* text;        // the resident text: byte 0 is offset `base` of the caller's buffer
    const int64_t* off;         // [n + 1] the caller's offsets
    int64_t base;
    int64_t r0;                 // the chunk's first read
    int32_t cn;                 // reads of the chunk
    int32_t k, min_hits, both, slots;
    const unsigned long long* tab;
    uint64_t cap_mask;
    int shift;
    int32_t* which;             // [n]
    uint8_t* strand;
    int32_t* votes;
    int32_t* rival;
    uint32_t* fb;               // [n] the reads whose tally overflowed, any order
    uint32_t* counters;
};

// The amplicon of a window's key, kNone when the key is absent or AMBIGUOUS.
__device__ inline int32_t lookup(const unsigned long long* tab, uint64_t window, int shift, uint64_t cap_mask) {
    const unsigned long long key = window | kKeyBit;
    uint64_t s = (key * kPoly) >> shift;
    for (uint64_t probe = 0; probe <= cap_mask; ++probe) {        // bounded by the table size
        const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(tab + 2 * s);
        if (e.x == key) return e.y < kAmbiguous ? (int32_t)e.y : kNone;
        if (e.x == 0) return kNone;
        s = (s + 1) & cap_mask;
    }
    return kNone;
}

// The lanes that hold one candidate add their number to its tally entry once; false in a lane
// whose candidate found every entry taken by another.
__device__ inline bool tally(int32_t* tk, int32_t* tc, int slots, int32_t cand) {
    int lead;
    const uint32_t cnt = grp::wave_elect((uint64_t)(uint32_t)cand, cand != kNone, &lead);
    if (!cnt) return true;
    int s = cand % slots;
    for (int probe = 0; probe < slots; ++probe) {
        int32_t cur = __hip_atomic_load(&tk[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == kNone) cur = atomicCAS(&tk[s], kNone, cand);
        if (cur == kNone || cur == cand) {
            atomicAdd(&tc[s], (int32_t)cnt);
            return true;
        }
        s = s + 1 == slots ? 0 : s + 1;
    }
    return false;
}

// The tally is one wavefront's own: its LDS operations complete in order, the fence keeps the
// compiler from moving them across.
__device__ inline void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(256) void nwd_assign_kernel(AssignArgs a) {
    __shared__ int32_t t_key[4][NWD_MAX_TALLY_SLOTS];
    __shared__ int32_t t_cnt[4][NWD_MAX_TALLY_SLOTS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 4 + wv;
    if (i >= a.cn) return;                                    // (the whole wavefront)
    const int64_t r = a.r0 + i;
    const int64_t o0 = a.off[r];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.off[r + 1] - o0));
    const uint8_t* s = a.text + (o0 - a.base);
    int32_t* tk = t_key[wv];
    int32_t* tc = t_cnt[wv];
    for (int j = lane; j < a.slots; j += 64) {
        tk[j] = kNone;
        tc[j] = 0;
    }
    wave_lds_fence();
    const int k = a.k, nwin = n - k + 1;
    bool full = false;
    if (nwin > 0) {
        const uint64_t mask = (1ull << (2 * k)) - 1ull;
        const int per = (nwin + 63) >> 6;                     // windows per lane
        const int p0 = lane * per;
        Roll w;
        for (int j = 0; j < k - 1; ++j)
            if (p0 + j < n) w.push(s[p0 + j], k, mask);
        for (int t = 0; t < per; ++t) {
            const int p = p0 + t;
            const bool have = p < nwin;
            if (have) w.push(s[p + k - 1], k, mask);
            const bool clean = have && w.run >= k;
            int32_t cf = kNone, cr = kNone;
            if (clean) {
                const int32_t g = lookup(a.tab, w.fwd, a.shift, a.cap_mask);
                if (g != kNone) cf = 2 * g;
                if (a.both) {
                    const int32_t h = lookup(a.tab, w.rc, a.shift, a.cap_mask);
                    if (h != kNone) cr = 2 * h + 1;
                }
            }
            if (!tally(tk, tc, a.slots, cf)) full = true;
            if (!tally(tk, tc, a.slots, cr)) full = true;
        }
    }
    wave_lds_fence();
    // best, its candidate and the largest count of any other entry
    int32_t best = 0, cand = kNone, riv = 0;
    for (int j = lane; j < a.slots; j += 64) {
        const int32_t c = tc[j];
        if (c > best) {
            riv = best;
            best = c;
            cand = tk[j];
        } else if (c > riv) {
            riv = c;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const int32_t ob = __shfl_xor(best, o, 64), oc = __shfl_xor(cand, o, 64), orv = __shfl_xor(riv, o, 64);
        const int32_t low = best < ob ? best : ob;
        if (ob > best) cand = oc;          // (equal counts: rival == best, the candidate is not used)
        best = best > ob ? best : ob;
        riv = riv > orv ? riv : orv;
        riv = riv > low ? riv : low;
    }
    const bool over = __ballot(full) != 0;
    const uint32_t at = grp::wave_reserve(over && lane == 0, &a.counters[kFallback]);
    if (lane == 0) {
        if (over) a.fb[at] = (uint32_t)r;
        const bool hit = best >= a.min_hits, sole = best > riv;
        a.which[r] = !hit ? NWD_NO_HIT : (sole ? (cand >> 1) : NWD_TIE);
        a.strand[r] = (uint8_t)(hit && sole ? (cand & 1) : 0);
        a.votes[r] = best;
        a.rival[r] = riv;
    }
}

// src[j] = the input index of gathered read j, bit 63 set for strand 1; dst [na + 1].
__global__ __launch_bounds__(256) void nwd_gather_kernel(const uint8_t* text, const int64_t* off, int64_t base,
                                                         const uint64_t* src, const int64_t* dst, int64_t na,
                                                         uint8_t* out) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= na) return;
    const uint64_t sr = src[j];
    const int64_t r = (int64_t)(sr & ~(1ull << 63));
    const bool rev = (sr >> 63) != 0;
    const int64_t o0 = off[r];
    const int n = (int)(off[r + 1] - o0);
    const uint8_t* s = text + (o0 - base);
    uint8_t* d = out + dst[j];
    for (int p = lane; p < n; p += 64) d[p] = rev ? complement(s[n - 1 - p]) : s[p];
}

// ---- the packer of the grouped reads -----------------------------------------------------------

constexpr int kPackBlk = 256;      // dwords (threads) per block: 4096 gathered positions
constexpr int kScanBlk = 1024;     // threads of the scan block

__device__ __forceinline__ bool is_acgt(uint8_t b) {   // nw_pack.cpp's
    const uint8_t u = b & 0xDF;
    return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}

struct PackArgs {
    const uint8_t* text;        // the resident input (AssignArgs::text)
    const int64_t* off;
    int64_t base;
    const uint64_t* src;        // [na]
    const int64_t* dst;         // [na + 1]
    int64_t na, total, nwords, blocks, n_exc;
    uint32_t* words;            // [nwords]
    uint32_t* sums;             // [blocks] exceptions of each block, then their exclusive prefix
    int64_t* totals;            // [1]
    int64_t* exc_pos;           // [n_exc]
    uint8_t* exc_byte;
};

// Gathered positions 16 w .. 16 w + 15 in the gathered order: byte k of raw is the input byte that
// position 16 w + k shows (not yet complemented), bit k of rev set when its read is strand 1,
// have = the positions before the end of the gathered text (1..16).
struct Piece {
    uint64_t lo, hi;           // bytes 0..7 and 8..15
    uint32_t rev;
    int have;
};

__device__ __forceinline__ Piece piece_at(const PackArgs& a, int64_t w) {
    Piece pc{0, 0, 0, 0};
    const int64_t p0 = 16 * w;
    const int64_t left = a.total - p0;                     // >= 1
    pc.have = left < 16 ? (int)left : 16;
    int64_t lo = 0, hi = a.na;                             // the last j with dst[j] <= p0: its read holds p0
    while (hi - lo > 1) {                                  // (at most 31 steps: na < 2^31)
        const int64_t mid = (lo + hi) >> 1;
        if (a.dst[mid] <= p0) lo = mid; else hi = mid;
    }
    int64_t j = lo;
    uint64_t sr = a.src[j];
    int64_t r = (int64_t)(sr & ~(1ull << 63));
    bool rev = (sr >> 63) != 0;
    int64_t o0 = a.off[r] - a.base, d0 = a.dst[j], e = a.dst[j + 1];
    if (p0 + 16 <= e) {                                    // all 16 in this read: one load
        const int64_t q = p0 - d0, n = e - d0;
        uint32_t in[4];
        __builtin_memcpy(in, a.text + o0 + (rev ? n - q - 16 : q), 16);
        if (rev) {
            pc.lo = ((uint64_t)__builtin_bswap32(in[2]) << 32) | __builtin_bswap32(in[3]);
            pc.hi = ((uint64_t)__builtin_bswap32(in[0]) << 32) | __builtin_bswap32(in[1]);
            pc.rev = 0xFFFFu;
        } else {
            pc.lo = ((uint64_t)in[1] << 32) | in[0];
            pc.hi = ((uint64_t)in[3] << 32) | in[2];
        }
        return pc;
    }
    for (int k = 0; k < pc.have; ++k) {                    // the end of one read and the start of the next
        const int64_t p = p0 + k;
        while (p >= e && j + 1 < a.na) {                   // (empty reads are stepped over)
            ++j;
            sr = a.src[j];
            r = (int64_t)(sr & ~(1ull << 63));
            rev = (sr >> 63) != 0;
            o0 = a.off[r] - a.base;
            d0 = e;
            e = a.dst[j + 1];
        }
        const int64_t q = p - d0;
        const uint8_t c = a.text[o0 + (rev ? (e - d0) - 1 - q : q)];
        if (k < 8) pc.lo |= (uint64_t)c << (8 * k);
        else pc.hi |= (uint64_t)c << (8 * (k - 8));
        pc.rev |= (rev ? 1u : 0u) << k;
    }
    return pc;
}

__device__ __forceinline__ uint8_t piece_byte(const Piece& pc, int k) {
    return (uint8_t)(k < 8 ? pc.lo >> (8 * k) : pc.hi >> (8 * (k - 8)));
}

__global__ __launch_bounds__(kPackBlk) void nwd_pack_words_kernel(const PackArgs a) {
    __shared__ uint32_t part[kPackBlk / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * kPackBlk + threadIdx.x;
    uint32_t ne = 0;
    if (w < a.nwords) {
        const Piece pc = piece_at(a, w);
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint8_t c = piece_byte(pc, k);
            if (k < pc.have) {
                // the complement of a base is its code ^ 2 (A C T G = 0 1 2 3)
                if (is_acgt(c)) out |= ((uint32_t)((c >> 1) & 3) ^ (((pc.rev >> k) & 1u) << 1)) << (2 * k);
                else ++ne;
            }
        }
        a.words[w] = out;
    }
    for (int s = 32; s > 0; s >>= 1) ne += __shfl_xor(ne, s);
    if (lane == 0) part[wave] = ne;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int v = 0; v < kPackBlk / 64; ++v) s += part[v];
        a.sums[blockIdx.x] = s;
    }
}

// One block: sums[b] becomes the exclusive prefix over the blocks before b; totals[0] the sum.
__global__ __launch_bounds__(kScanBlk) void nwd_pack_scan_kernel(const PackArgs a) {
    __shared__ uint32_t sh[2][kScanBlk];
    const int t = threadIdx.x;
    const int64_t per = (a.blocks + kScanBlk - 1) / kScanBlk;
    const int64_t lo = std::min<int64_t>(a.blocks, t * per), hi = std::min<int64_t>(a.blocks, lo + per);
    uint32_t mine = 0;
    for (int64_t b = lo; b < hi; ++b) mine += a.sums[b];
    int cur = 0;
    sh[0][t] = mine;
    __syncthreads();
    for (int d = 1; d < kScanBlk; d <<= 1) {               // inclusive scan of the threads' sums
        sh[cur ^ 1][t] = sh[cur][t] + (t >= d ? sh[cur][t - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    uint32_t run = sh[cur][t] - mine;
    if (t == kScanBlk - 1) a.totals[0] = (int64_t)sh[cur][t];
    for (int64_t b = lo; b < hi; ++b) {
        const uint32_t v = a.sums[b];
        a.sums[b] = run;
        run += v;
    }
}

// The exceptions in ascending position: the slot of a thread's first one is the block's base +
// the exceptions of the block's threads before it.
__global__ __launch_bounds__(kPackBlk) void nwd_pack_exc_kernel(const PackArgs a) {
    __shared__ uint32_t part[kPackBlk / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * kPackBlk + threadIdx.x;
    Piece pc{0, 0, 0, 0};
    uint32_t ne = 0;
    if (w < a.nwords) {
        pc = piece_at(a, w);
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < pc.have && !is_acgt(piece_byte(pc, k))) ++ne;
    }
    uint32_t x = ne;
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t y = __shfl_up(x, s);
        if (lane >= s) x += y;
    }
    if (lane == 63) part[wave] = x;
    __syncthreads();
    int64_t slot = (int64_t)a.sums[blockIdx.x] + (x - ne);
    for (int v = 0; v < wave; ++v) slot += part[v];
    if (ne == 0) return;
    for (int k = 0; k < pc.have; ++k) {
        const uint8_t c = piece_byte(pc, k);
        if (is_acgt(c)) continue;
        if (slot < a.n_exc) {                              // (always: the count kernel's sum)
            a.exc_pos[slot] = 16 * w + k;
            a.exc_byte[slot] = c;                          // (complement leaves every such byte as it is)
        }
        ++slot;
    }
}

// gexc[g] = the exceptions before group g's first position, g in [0, ng]: group g's are the slots
// gexc[g] .. gexc[g + 1].
__global__ __launch_bounds__(256) void nwd_pack_bounds_kernel(const int64_t* exc_pos, int64_t n_exc, const int64_t* dst,
                                                              const int64_t* goff, int64_t ng, int64_t* gexc) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g > ng) return;
    const int64_t pos = dst[goff[g]];
    int64_t lo = 0, hi = n_exc;                            // the first slot with exc_pos >= pos
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (exc_pos[mid] < pos) lo = mid + 1; else hi = mid;
    }
    gexc[g] = lo;
}

}  // namespace nwd

struct nwd_ctx : hd::DevContext {
    int64_t chunk_reads = 0;       // 0: by bytes
    int32_t slots = 64;
    // the index
    int32_t k = 0;
    int64_t n_refs = 0;
    grp::TableGeometry tg{};
    std::vector<uint8_t> refs;     // kept for the exact path
    std::vector<int64_t> roff;
    bool host_index_built = false;
    std::unordered_map<uint64_t, int32_t> host_index;      // window -> g, -1 = AMBIGUOUS
    // the last assign
    int64_t n = 0, base = 0, fallback = 0;
    std::vector<int64_t> off;      // the caller's offsets
    std::vector<int32_t> which;
    std::vector<uint8_t> strand;
    std::vector<int64_t> counts;
    float phase_ms[4] = {0, 0, 0, 0};
    // the groups of the last assign (group_layout): one host pass, shared by the gather and the packer
    bool layout_ok = false;
    std::vector<int64_t> goff, dst;
    std::vector<uint64_t> src;     // input index, bit 63 = strand
    // the last pack: valid until the next nwd_assign / nwd_set_amplicons
    bool packed_ok = false;
    int64_t pk_total = 0, pk_n_exc = 0;
    std::vector<uint16_t> lens16;
    std::vector<int64_t> gexc;
    hd::DevBuf<uint32_t> d_words, d_sums;
    hd::DevBuf<uint16_t> d_lens16;
    hd::DevBuf<int64_t> d_totals, d_exc_pos, d_goff, d_gexc, d_gbase;
    hd::DevBuf<uint8_t> d_exc_byte;
    hd::DevBuf<unsigned long long> d_tab;
    hd::DevBuf<uint8_t> d_refs, d_text, d_strand, d_out;
    hd::DevBuf<int64_t> d_roff, d_off, d_dst;
    hd::DevBuf<int32_t> d_which, d_votes, d_rival;
    hd::DevBuf<uint32_t> d_fb, d_counters;
    hd::DevBuf<uint64_t> d_src;
};

namespace {

using hd::fail;

// The index as the host's exact path reads it: the rule of the header on a hash map.
void build_host_index(nwd_ctx* c) {
    c->host_index.clear();
    const int k = c->k;
    const uint64_t mask = (1ull << (2 * k)) - 1ull;
    for (int64_t g = 0; g < c->n_refs; ++g) {
        nwd::Roll w;
        for (int64_t p = c->roff[(size_t)g]; p < c->roff[(size_t)g + 1]; ++p) {
            w.push(c->refs[(size_t)p], k, mask);
            if (w.run < k) continue;
            auto ins = c->host_index.emplace(w.fwd, (int32_t)g);
            if (!ins.second && ins.first->second != (int32_t)g) ins.first->second = -1;
        }
    }
    c->host_index_built = true;
}

// One read by the rule, on the host (the reads whose device tally overflowed).
void decide_on_host(nwd_ctx* c, const uint8_t* s, int n, int min_hits, bool both, int32_t* which, uint8_t* strand,
                    int32_t* votes, int32_t* rival) {
    const int k = c->k;
    const uint64_t mask = (1ull << (2 * k)) - 1ull;
    std::unordered_map<int32_t, int32_t> tally;
    nwd::Roll w;
    for (int p = 0; p < n; ++p) {
        w.push(s[p], k, mask);
        if (w.run < k) continue;
        auto f = c->host_index.find(w.fwd);
        if (f != c->host_index.end() && f->second >= 0) ++tally[2 * f->second];
        if (!both) continue;
        auto b = c->host_index.find(w.rc);
        if (b != c->host_index.end() && b->second >= 0) ++tally[2 * b->second + 1];
    }
    int32_t best = 0, cand = -1, riv = 0;
    for (const auto& e : tally) {
        if (e.second > best) {
            riv = best;
            best = e.second;
            cand = e.first;
        } else if (e.second > riv) {
            riv = e.second;
        }
    }
    const bool hit = best >= min_hits, sole = best > riv;
    *which = !hit ? NWD_NO_HIT : (sole ? (cand >> 1) : NWD_TIE);
    *strand = (uint8_t)(hit && sole ? (cand & 1) : 0);
    *votes = best;
    *rival = riv;
}

// The groups of the last assign, one pass of the host over `which` (kept until the next assign):
// goff by a prefix sum of the counts, src[j] = the input index of gathered read j (ascending in
// its group) with bit 63 as its strand, dst [na + 1] the gathered offsets.
void group_layout(nwd_ctx* c) {
    if (c->layout_ok) return;
    const int64_t n = c->n, ng = c->n_refs;
    c->goff.assign((size_t)ng + 1, 0);
    if (c->counts.size() == (size_t)ng)
        for (int64_t g = 0; g < ng; ++g) c->goff[(size_t)g + 1] = c->goff[(size_t)g] + c->counts[(size_t)g];
    const int64_t na = c->goff[(size_t)ng];
    std::vector<int64_t> next(c->goff.begin(), c->goff.end() - 1);
    c->dst.assign((size_t)na + 1, 0);
    c->src.resize((size_t)na);
    for (int64_t r = 0; r < n; ++r) {
        const int32_t g = c->which[(size_t)r];
        if (g < 0) continue;
        c->src[(size_t)next[(size_t)g]++] = (uint64_t)r | ((uint64_t)(c->strand[(size_t)r] & 1) << 63);
    }
    for (int64_t j = 0; j < na; ++j) {
        const int64_t r = (int64_t)(c->src[(size_t)j] & ~(1ull << 63));
        c->dst[(size_t)j + 1] = c->dst[(size_t)j] + (c->off[(size_t)r + 1] - c->off[(size_t)r]);
    }
    c->layout_ok = true;
}

}  // namespace

extern "C" {

int nwd_create(int device, nwd_ctx** out) {
    const int rc = hd::create_context(device, 3, out);      // ev[2]: recorded behind the last packer
    if (rc != NW_OK) return rc;
    nwd_ctx* c = *out;
    if (const char* e = std::getenv("CRISPR_NWD_CHUNK"))
        c->chunk_reads = std::max<int64_t>(0, std::min<int64_t>(std::atoll(e), 0x7FFFFFFFll));
    if (const char* e = std::getenv("CRISPR_NWD_TALLY_SLOTS"))
        c->slots = (int32_t)std::max<long long>(1, std::min<long long>(std::atoll(e), NWD_MAX_TALLY_SLOTS));
    return NW_OK;
}

void nwd_destroy(nwd_ctx* c) { hd::destroy_context(c); }

const char* nwd_last_error(const nwd_ctx* c) { return c ? c->err.c_str() : "null context"; }

int64_t nwd_last_fallback(const nwd_ctx* c) { return c ? c->fallback : -1; }

int nwd_phase_times(const nwd_ctx* c, float* ms) {
    if (!c || !ms) return NW_E_INVALID;
    std::memcpy(ms, c->phase_ms, sizeof c->phase_ms);
    return NW_OK;
}

int nwd_set_amplicons(nwd_ctx* c, const uint8_t* refs, const int64_t* ref_offsets, int64_t n_refs, int32_t k,
                      int64_t* n_windows, int64_t* n_ambiguous) {
    if (!c) return NW_E_INVALID;
    if (k < NWD_MIN_K || k > NWD_MAX_K)
        return fail(c, NW_E_UNSUPPORTED, "window length %d: %d to %d are supported", (int)k, NWD_MIN_K, NWD_MAX_K);
    if (n_refs < 1 || n_refs > NWD_MAX_REFS)
        return fail(c, NW_E_UNSUPPORTED, "%lld amplicons: 1 to %d are supported", (long long)n_refs, NWD_MAX_REFS);
    if (!refs || !ref_offsets) return fail(c, NW_E_INVALID, "null input array");
    for (int64_t g = 0; g < n_refs; ++g)
        if (ref_offsets[g + 1] < ref_offsets[g])
            return fail(c, NW_E_INVALID, "offsets do not ascend at amplicon %lld", (long long)g);
    const int64_t total = ref_offsets[n_refs] - ref_offsets[0];
    if (total > NWD_MAX_REF_BASES)
        return fail(c, NW_E_UNSUPPORTED, "%lld amplicon bases: at most %d are supported", (long long)total,
                    NWD_MAX_REF_BASES);
    c->k = 0;                      // no index until this call succeeds
    c->n_refs = 0;
    c->n = 0;
    c->layout_ok = c->packed_ok = false;
    c->which.clear();
    c->strand.clear();
    c->counts.clear();
    c->host_index_built = false;
    c->host_index.clear();
    c->refs.assign(refs + ref_offsets[0], refs + ref_offsets[n_refs]);
    c->roff.resize((size_t)n_refs + 1);
    for (int64_t g = 0; g <= n_refs; ++g) c->roff[(size_t)g] = ref_offsets[g] - ref_offsets[0];
    const grp::TableGeometry tg = grp::table_geometry(total, 64);      // (windows <= bases)
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(c, c->d_tab.reserve(2 * tg.slots));
    HIP_TRY(c, c->d_refs.reserve((size_t)total));
    HIP_TRY(c, c->d_roff.reserve((size_t)n_refs + 1));
    HIP_TRY(c, c->d_counters.reserve(nwd::kCounters));
    HIP_TRY(c, hipMemsetAsync(c->d_counters.p, 0, sizeof(uint32_t) * nwd::kCounters, st));
    if (total > 0)
        HIP_TRY(c, hipMemcpyAsync(c->d_refs.p, c->refs.data(), (size_t)total, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_roff.p, c->roff.data(), sizeof(int64_t) * (size_t)(n_refs + 1), hipMemcpyHostToDevice, st));
    nwd::IndexArgs a{};
    a.refs = c->d_refs.p;
    a.roff = c->d_roff.p;
    a.n_refs = (int32_t)n_refs;
    a.k = k;
    a.total = total;
    a.tab = c->d_tab.p;
    a.cap_mask = tg.cap_mask;
    a.shift = tg.shift;
    a.counters = c->d_counters.p;
    const unsigned slot_grid = (unsigned)((tg.slots + 255) / 256);
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(nwd::nwd_clear_kernel, dim3(slot_grid), dim3(256), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    if (total > 0) {
        hipLaunchKernelGGL(nwd::nwd_index_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
        HIP_TRY(c, hipGetLastError());
    }
    hipLaunchKernelGGL(nwd::nwd_census_kernel, dim3(slot_grid), dim3(256), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    uint32_t ctr[nwd::kCounters] = {};
    HIP_TRY(c, hipMemcpyAsync(ctr, c->d_counters.p, sizeof ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipEventElapsedTime(&c->phase_ms[2], c->ev[0], c->ev[1]));
    if (ctr[nwd::kError])
        return fail(c, NW_E_STATE, "the index table's probe bound was reached (%zu slots, %lld bases)", tg.slots,
                    (long long)total);
    if (n_windows) *n_windows = ctr[nwd::kWindows];
    if (n_ambiguous) *n_ambiguous = ctr[nwd::kAmbig];
    c->tg = tg;
    c->k = k;
    c->n_refs = n_refs;
    return NW_OK;
}

// nwd_assign and nwd_assign_prepared: `reads` is indexed by the caller's offsets and lies in host
// memory, or (on_device) in this context's HBM, complete once `ready` (may be null) has passed.
// The chunks' copies into the text buffer are then device to device, and a fallback read is
// copied down from that buffer.
static int assign_reads(nwd_ctx* c, const uint8_t* reads, bool on_device, hipEvent_t ready, const int64_t* offsets,
                        int64_t n, int32_t min_hits, int32_t both_strands, int32_t* which, uint8_t* strand,
                        int32_t* votes, int32_t* rival, int64_t* counts, int64_t* n_assigned, int64_t* n_tie,
                        int64_t* n_no_hit, float* kernel_ms) {
    if (n < 0 || n > 0x7FFFFFFFll) return fail(c, NW_E_INVALID, "read count %lld out of range", (long long)n);
    if (min_hits < 1) return fail(c, NW_E_UNSUPPORTED, "min_hits %d: at least 1", (int)min_hits);
    if (n > 0 && (!reads || !offsets)) return fail(c, NW_E_INVALID, "null input array");
    for (int64_t r = 0; r < n; ++r) {
        const int64_t len = offsets[r + 1] - offsets[r];
        if (len < 0) return fail(c, NW_E_INVALID, "offsets do not ascend at read %lld", (long long)r);
        if (len > NWD_MAX_READ)
            return fail(c, NW_E_UNSUPPORTED, "read %lld has %lld bases: at most %d are supported", (long long)r,
                        (long long)len, NWD_MAX_READ);
    }
    c->n = 0;
    c->layout_ok = c->packed_ok = false;
    c->fallback = 0;
    c->phase_ms[0] = c->phase_ms[1] = 0.0f;
    c->which.assign((size_t)n, NWD_NO_HIT);
    c->strand.assign((size_t)n, 0);
    c->counts.assign((size_t)c->n_refs, 0);
    c->off.assign(offsets, offsets + (n > 0 ? n + 1 : 0));
    std::vector<int32_t> h_votes((size_t)n, 0), h_rival((size_t)n, 0);
    const bool both = both_strands != 0;

    if (n > 0) {
        HIP_TRY(c, hipSetDevice(c->device));
        hipStream_t st = c->stream;
        // the text keeps the phase of its first byte within a word (lead), as a resident batch would
        const int64_t lead = offsets[0] & 3, base = offsets[0] - lead, nbytes = offsets[n] - offsets[0];
        c->base = base;
        HIP_TRY(c, c->d_text.reserve((size_t)(lead + nbytes + 4)));
        HIP_TRY(c, c->d_off.reserve((size_t)n + 1));
        HIP_TRY(c, c->d_which.reserve((size_t)n));
        HIP_TRY(c, c->d_strand.reserve((size_t)n));
        HIP_TRY(c, c->d_votes.reserve((size_t)n));
        HIP_TRY(c, c->d_rival.reserve((size_t)n));
        HIP_TRY(c, c->d_fb.reserve((size_t)n));
        HIP_TRY(c, c->d_counters.reserve(nwd::kCounters));
        HIP_TRY(c, hipMemsetAsync(c->d_counters.p, 0, sizeof(uint32_t) * nwd::kCounters, st));
        HIP_TRY(c, hipMemcpyAsync(c->d_off.p, offsets, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, st));
        nwd::AssignArgs a{};
        a.text = c->d_text.p;
        a.off = c->d_off.p;
        a.base = base;
        a.k = c->k;
        a.min_hits = min_hits;
        a.both = both ? 1 : 0;
        a.slots = c->slots;
        a.tab = c->d_tab.p;
        a.cap_mask = c->tg.cap_mask;
        a.shift = c->tg.shift;
        a.which = c->d_which.p;
        a.strand = c->d_strand.p;
        a.votes = c->d_votes.p;
        a.rival = c->d_rival.p;
        a.fb = c->d_fb.p;
        a.counters = c->d_counters.p;
        if (on_device && ready) HIP_TRY(c, hipStreamWaitEvent(st, ready, 0));
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        for (int64_t r0 = 0; r0 < n;) {
            int64_t r1;
            if (c->chunk_reads > 0) {
                r1 = std::min(n, r0 + c->chunk_reads);
            } else {
                r1 = std::min(n, r0 + nwd::kChunkReads);
                const int64_t* e = std::upper_bound(offsets + r0 + 1, offsets + r1 + 1, offsets[r0] + nwd::kChunkBytes);
                r1 = std::max<int64_t>(r0 + 1, (e - offsets) - 1);      // (one read at least)
            }
            const int64_t cn = r1 - r0, cbytes = offsets[r1] - offsets[r0];
            const auto t0 = std::chrono::steady_clock::now();
            if (cbytes > 0)
                HIP_TRY(c, hipMemcpyAsync(c->d_text.p + (offsets[r0] - base), reads + offsets[r0], (size_t)cbytes, kind, st));
            HIP_TRY(c, hipStreamSynchronize(st));
            c->phase_ms[1] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            a.r0 = r0;
            a.cn = (int32_t)cn;
            HIP_TRY(c, hipEventRecord(c->ev[0], st));
            hipLaunchKernelGGL(nwd::nwd_assign_kernel, dim3((unsigned)((cn + 3) / 4)), dim3(256), 0, st, a);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(c->ev[1], st));
            HIP_TRY(c, hipStreamSynchronize(st));
            float ms = 0.0f;
            HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
            c->phase_ms[0] += ms;
            r0 = r1;
        }
        uint32_t ctr[nwd::kCounters] = {};
        HIP_TRY(c, hipMemcpyAsync(ctr, c->d_counters.p, sizeof ctr, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(c->which.data(), a.which, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(c->strand.data(), a.strand, (size_t)n, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(h_votes.data(), a.votes, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(h_rival.data(), a.rival, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        const int64_t nfb = ctr[nwd::kFallback];
        if (nfb > n) return fail(c, NW_E_STATE, "inconsistent fallback count");
        if (nfb > 0) {      // more candidates than the tally holds: the same rule, on the host
            std::vector<uint32_t> fb((size_t)nfb);
            HIP_TRY(c, hipMemcpy(fb.data(), a.fb, sizeof(uint32_t) * (size_t)nfb, hipMemcpyDeviceToHost));
            if (!c->host_index_built) build_host_index(c);
            std::vector<uint8_t> one((size_t)NWD_MAX_READ);
            for (uint32_t r : fb) {
                if ((int64_t)r >= n) return fail(c, NW_E_STATE, "inconsistent fallback read");
                const int len = (int)(offsets[r + 1] - offsets[r]);
                const uint8_t* s = reads + offsets[r];
                if (on_device) {      // the read copied down from the text buffer, one at a time
                    if (len > 0)
                        HIP_TRY(c, hipMemcpy(one.data(), c->d_text.p + (offsets[r] - base), (size_t)len, hipMemcpyDeviceToHost));
                    s = one.data();
                }
                decide_on_host(c, s, len, min_hits, both, &c->which[r], &c->strand[r], &h_votes[r], &h_rival[r]);
            }
        }
        c->fallback = nfb;
    }
    int64_t na = 0, nt = 0, nn = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int32_t g = c->which[(size_t)r];
        if (g >= 0) {
            if (g >= c->n_refs) return fail(c, NW_E_STATE, "read %lld assigned to amplicon %d of %lld", (long long)r,
                                            (int)g, (long long)c->n_refs);
            ++c->counts[(size_t)g];
            ++na;
        } else if (g == NWD_TIE) {
            ++nt;
        } else {
            ++nn;
        }
    }
    c->n = n;
    if (n > 0) {
        if (which) std::memcpy(which, c->which.data(), sizeof(int32_t) * (size_t)n);
        if (strand) std::memcpy(strand, c->strand.data(), (size_t)n);
        if (votes) std::memcpy(votes, h_votes.data(), sizeof(int32_t) * (size_t)n);
        if (rival) std::memcpy(rival, h_rival.data(), sizeof(int32_t) * (size_t)n);
    }
    if (counts) std::memcpy(counts, c->counts.data(), sizeof(int64_t) * (size_t)c->n_refs);
    if (n_assigned) *n_assigned = na;
    if (n_tie) *n_tie = nt;
    if (n_no_hit) *n_no_hit = nn;
    if (kernel_ms) *kernel_ms = c->phase_ms[0];
    return NW_OK;
}

int nwd_assign(nwd_ctx* c, const uint8_t* reads, const int64_t* offsets, int64_t n, int32_t min_hits,
               int32_t both_strands, int32_t* which, uint8_t* strand, int32_t* votes, int32_t* rival,
               int64_t* counts, int64_t* n_assigned, int64_t* n_tie, int64_t* n_no_hit, float* kernel_ms) {
    if (!c) return NW_E_INVALID;
    if (c->k == 0) return fail(c, NW_E_STATE, "nwd_assign before nwd_set_amplicons");
    return assign_reads(c, reads, false, nullptr, offsets, n, min_hits, both_strands, which, strand, votes, rival, counts,
                        n_assigned, n_tie, n_no_hit, kernel_ms);
}

int nwd_assign_prepared(nwd_ctx* c, const nwp_result* res, int32_t min_hits, int32_t both_strands, int32_t* which,
                        uint8_t* strand, int32_t* votes, int32_t* rival, int64_t* counts, int64_t* n_assigned,
                        int64_t* n_tie, int64_t* n_no_hit, float* kernel_ms) {
    if (!c) return NW_E_INVALID;
    nw_front::PreparedView v{};
    if (nw_front::view_prepared(res, &v) != NW_OK) return fail(c, NW_E_INVALID, "a null or released nwp_result");
    if (c->k == 0) return fail(c, NW_E_STATE, "nwd_assign_prepared before nwd_set_amplicons");
    if (v.device != c->device)
        return fail(c, NW_E_INVALID, "the prepared reads lie on device %d, the index on device %d", v.device, c->device);
    if (v.m < 0 || v.total < 0 || v.offsets[0] != 0 || v.offsets[v.m] != v.total)
        return fail(c, NW_E_INVALID, "inconsistent nwp_result");
    return assign_reads(c, v.text, true, v.ready, v.offsets, v.m, min_hits, both_strands, which, strand, votes, rival,
                        counts, n_assigned, n_tie, n_no_hit, kernel_ms);
}

int nwd_gather(nwd_ctx* c, int64_t* group_offsets, int64_t* order, uint8_t* text, int64_t* text_offsets,
               int64_t text_cap, int64_t* needed) {
    if (!c) return NW_E_INVALID;
    if (c->k == 0) return fail(c, NW_E_STATE, "nwd_gather before nwd_set_amplicons");
    if (text_cap < 0) return fail(c, NW_E_INVALID, "negative capacity");
    const int64_t ng = c->n_refs;
    c->phase_ms[3] = 0.0f;
    group_layout(c);
    const std::vector<int64_t>&goff = c->goff, &dst = c->dst;
    const std::vector<uint64_t>& src = c->src;
    const int64_t na = goff[(size_t)ng];
    const int64_t nbytes = dst[(size_t)na];
    if (needed) *needed = nbytes;
    if (group_offsets) std::memcpy(group_offsets, goff.data(), sizeof(int64_t) * (size_t)(ng + 1));
    if (order)
        for (int64_t j = 0; j < na; ++j) order[j] = (int64_t)(src[(size_t)j] & ~(1ull << 63));
    if (text_offsets) std::memcpy(text_offsets, dst.data(), sizeof(int64_t) * (size_t)(na + 1));
    if (nbytes > text_cap)
        return fail(c, NW_E_CAPACITY, "%lld gathered bytes, capacity %lld", (long long)nbytes, (long long)text_cap);
    if (nbytes == 0) return NW_OK;
    if (!text) return fail(c, NW_E_INVALID, "null text");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(c, c->d_src.reserve((size_t)na));
    HIP_TRY(c, c->d_dst.reserve((size_t)na + 1));
    HIP_TRY(c, c->d_out.reserve((size_t)nbytes));
    HIP_TRY(c, hipMemcpyAsync(c->d_src.p, src.data(), sizeof(uint64_t) * (size_t)na, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_dst.p, dst.data(), sizeof(int64_t) * (size_t)(na + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(nwd::nwd_gather_kernel, dim3((unsigned)((na + 3) / 4)), dim3(256), 0, st, c->d_text.p, c->d_off.p,
                       c->base, c->d_src.p, c->d_dst.p, na, c->d_out.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipMemcpyAsync(text, c->d_out.p, (size_t)nbytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));      // (src and dst above are read by the copies)
    HIP_TRY(c, hipEventElapsedTime(&c->phase_ms[3], c->ev[0], c->ev[1]));
    return NW_OK;
}

int nwd_pack(nwd_ctx* c, int64_t* group_offsets, int64_t* order, int64_t* text_offsets, uint16_t* lens,
             int64_t* group_exc, int64_t* n_exc, float* kernel_ms) {
    if (!c) return NW_E_INVALID;
    if (c->k == 0) return fail(c, NW_E_STATE, "nwd_pack before nwd_set_amplicons");
    const int64_t ng = c->n_refs;
    c->packed_ok = false;
    group_layout(c);
    const int64_t na = c->goff[(size_t)ng], total = c->dst[(size_t)na];
    if ((uint64_t)total >= (1ull << 32))
        return fail(c, NW_E_UNSUPPORTED, "%lld gathered bytes: 2^32 or more in one call are not supported",
                    (long long)total);
    c->lens16.resize((size_t)na);
    for (int64_t j = 0; j < na; ++j) c->lens16[(size_t)j] = (uint16_t)(c->dst[(size_t)j + 1] - c->dst[(size_t)j]);
    c->gexc.assign((size_t)ng + 1, 0);
    c->pk_total = total;
    c->pk_n_exc = 0;
    float ms_a = 0.0f, ms_b = 0.0f;
    if (total > 0) {
        HIP_TRY(c, hipSetDevice(c->device));
        hipStream_t st = c->stream;
        nwd::PackArgs a{};
        a.na = na;
        a.total = total;
        a.nwords = (total + 15) / 16;
        a.blocks = (a.nwords + nwd::kPackBlk - 1) / nwd::kPackBlk;
        HIP_TRY(c, c->d_src.reserve((size_t)na));
        HIP_TRY(c, c->d_dst.reserve((size_t)na + 1));
        HIP_TRY(c, c->d_lens16.reserve((size_t)na));
        HIP_TRY(c, c->d_goff.reserve((size_t)ng + 1));
        HIP_TRY(c, c->d_gexc.reserve((size_t)ng + 1));
        HIP_TRY(c, c->d_words.reserve((size_t)a.nwords + 16));      // (the adoption's copies stay inside)
        HIP_TRY(c, c->d_sums.reserve((size_t)a.blocks));
        HIP_TRY(c, c->d_totals.reserve(1));
        HIP_TRY(c, hipMemcpyAsync(c->d_src.p, c->src.data(), sizeof(uint64_t) * (size_t)na, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(c->d_dst.p, c->dst.data(), sizeof(int64_t) * (size_t)(na + 1), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(c->d_lens16.p, c->lens16.data(), sizeof(uint16_t) * (size_t)na, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(c->d_goff.p, c->goff.data(), sizeof(int64_t) * (size_t)(ng + 1), hipMemcpyHostToDevice, st));
        a.text = c->d_text.p;
        a.off = c->d_off.p;
        a.base = c->base;
        a.src = c->d_src.p;
        a.dst = c->d_dst.p;
        a.words = c->d_words.p;
        a.sums = c->d_sums.p;
        a.totals = c->d_totals.p;
        HIP_TRY(c, hipEventRecord(c->ev[0], st));
        hipLaunchKernelGGL(nwd::nwd_pack_words_kernel, dim3((unsigned)a.blocks), dim3(nwd::kPackBlk), 0, st, a);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(nwd::nwd_pack_scan_kernel, dim3(1), dim3(nwd::kScanBlk), 0, st, a);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->ev[1], st));
        int64_t ne = 0;
        HIP_TRY(c, hipMemcpyAsync(&ne, a.totals, sizeof ne, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        HIP_TRY(c, hipEventElapsedTime(&ms_a, c->ev[0], c->ev[1]));
        if (ne < 0 || ne > total) return fail(c, NW_E_STATE, "inconsistent exception count");
        if (ne > 0) {      // (none: the exceptions kernel is skipped)
            HIP_TRY(c, c->d_exc_pos.reserve((size_t)ne));
            HIP_TRY(c, c->d_exc_byte.reserve((size_t)ne));
            a.n_exc = ne;
            a.exc_pos = c->d_exc_pos.p;
            a.exc_byte = c->d_exc_byte.p;
            HIP_TRY(c, hipEventRecord(c->ev[0], st));
            hipLaunchKernelGGL(nwd::nwd_pack_exc_kernel, dim3((unsigned)a.blocks), dim3(nwd::kPackBlk), 0, st, a);
            HIP_TRY(c, hipGetLastError());
            hipLaunchKernelGGL(nwd::nwd_pack_bounds_kernel, dim3((unsigned)((ng + 1 + 255) / 256)), dim3(256), 0, st,
                               (const int64_t*)a.exc_pos, ne, a.dst, (const int64_t*)c->d_goff.p, ng, c->d_gexc.p);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(c->ev[1], st));
            HIP_TRY(c, hipMemcpyAsync(c->gexc.data(), c->d_gexc.p, sizeof(int64_t) * (size_t)(ng + 1), hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipEventRecord(c->ev[2], st));
            HIP_TRY(c, hipStreamSynchronize(st));
            HIP_TRY(c, hipEventElapsedTime(&ms_b, c->ev[0], c->ev[1]));
        } else {
            HIP_TRY(c, hipEventRecord(c->ev[2], st));
        }
        c->pk_n_exc = ne;
    }
    if (group_offsets) std::memcpy(group_offsets, c->goff.data(), sizeof(int64_t) * (size_t)(ng + 1));
    if (order)
        for (int64_t j = 0; j < na; ++j) order[j] = (int64_t)(c->src[(size_t)j] & ~(1ull << 63));
    if (text_offsets) std::memcpy(text_offsets, c->dst.data(), sizeof(int64_t) * (size_t)(na + 1));
    if (lens && na > 0) std::memcpy(lens, c->lens16.data(), sizeof(uint16_t) * (size_t)na);
    if (group_exc) std::memcpy(group_exc, c->gexc.data(), sizeof(int64_t) * (size_t)(ng + 1));
    if (n_exc) *n_exc = c->pk_n_exc;
    if (kernel_ms) *kernel_ms = ms_a + ms_b;
    c->packed_ok = true;
    return NW_OK;
}

int nwd_fetch_packed(nwd_ctx* c, uint8_t* packed, int64_t cap, int64_t* exc_pos, uint8_t* exc_byte, int64_t* needed) {
    if (!c) return NW_E_INVALID;
    if (!c->packed_ok) return fail(c, NW_E_STATE, "nwd_fetch_packed before nwd_pack");
    const int64_t nbytes = (c->pk_total + 3) / 4, ne = c->pk_n_exc;
    if (needed) *needed = nbytes;
    if (cap < nbytes)
        return fail(c, NW_E_CAPACITY, "%lld packed bytes, capacity %lld", (long long)nbytes, (long long)cap);
    if (nbytes == 0) return NW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (packed) HIP_TRY(c, hipMemcpyAsync(packed, c->d_words.p, (size_t)nbytes, hipMemcpyDeviceToHost, st));
    if (exc_pos && ne > 0) HIP_TRY(c, hipMemcpyAsync(exc_pos, c->d_exc_pos.p, sizeof(int64_t) * (size_t)ne, hipMemcpyDeviceToHost, st));
    if (exc_byte && ne > 0) HIP_TRY(c, hipMemcpyAsync(exc_byte, c->d_exc_byte.p, (size_t)ne, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return NW_OK;
}

int nwd_adopt_group(nwd_ctx* c, nw_ctx* ctx, int64_t g) {
    if (!c) return NW_E_INVALID;
    if (!ctx) return fail(c, NW_E_INVALID, "null aligner context");
    if (!c->packed_ok) return fail(c, NW_E_STATE, "nwd_adopt_group before nwd_pack");
    if (g < 0 || g >= c->n_refs)
        return fail(c, NW_E_INVALID, "group %lld: there are %lld amplicons", (long long)g, (long long)c->n_refs);
    const int64_t j0 = c->goff[(size_t)g], m = c->goff[(size_t)g + 1] - j0;
    if (m <= 0) return fail(c, NW_E_INVALID, "group %lld holds no read", (long long)g);
    int rc = nw_front::check_state(ctx);
    if (rc != NW_OK) return fail(c, rc, "the aligner context: %s", nw_last_error(ctx));
    if (nw_front::device_of(ctx) != c->device)
        return fail(c, NW_E_INVALID, "the aligner context is on device %d, the reads on device %d",
                    nw_front::device_of(ctx), c->device);
    HIP_TRY(c, hipSetDevice(c->device));
    // every kLenGroup-th offset counted from the group's own first read (a group does not start
    // on a multiple of kLenGroup of the whole call)
    const int64_t ngroups = m / nw::kLenGroup + 1;
    std::vector<int64_t> gb((size_t)ngroups);
    for (int64_t q = 0; q < ngroups; ++q) gb[(size_t)q] = c->dst[(size_t)(j0 + q * nw::kLenGroup)];
    HIP_TRY(c, c->d_gbase.reserve((size_t)ngroups));
    HIP_TRY(c, hipMemcpyAsync(c->d_gbase.p, gb.data(), sizeof(int64_t) * (size_t)ngroups, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int64_t e0 = c->gexc[(size_t)g], ne = c->gexc[(size_t)g + 1] - e0;
    // the whole call's stream and the group's slice of the exceptions, both in gathered
    // coordinates: set_packed_batch copies bytes offsets[0] / 4 .. (offsets[m] + 3) / 4 of it
    const nw_front::PackedSrc src{(const uint8_t*)c->d_words.p,
                                  c->d_lens16.p + j0,
                                  c->d_gbase.p,
                                  ne > 0 ? c->d_exc_pos.p + e0 : nullptr,
                                  ne > 0 ? c->d_exc_byte.p + e0 : nullptr,
                                  true,
                                  c->ev[2]};
    rc = nw_front::set_packed_batch(ctx, src, c->dst.data() + j0, c->lens16.data() + j0, m, ne);
    if (rc != NW_OK) return fail(c, rc, "the aligner context: %s", nw_last_error(ctx));
    return NW_OK;
}

}  // extern "C"
