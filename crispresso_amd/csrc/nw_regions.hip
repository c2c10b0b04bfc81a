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
//
// nwr_discover (CRISPRessoPooled's genome mode, CRISPRessoPooledCORE.py:1045-1082) finds the
// regions first, over the same chunks:
//   span     a lane per record: the clip-extended span (ref, bpstart, bpend) of the header's walk,
//            packed into two 64-bit words, looked up in an open-addressing table in HBM that lives
//            for the call.  The probe starts at the slot of the key's hash; a slot is claimed by
//            a 64-bit atomicCAS on its first word and then on its second, each word is written
//            once and never changes, so a lane decides on what the CAS returned alone: the slot is
//            its key's, or some other key's and it probes on.  No lane waits for another, keys
//            with equal hashes part exactly, the probes are bounded by the table size.  The
//            slot's count goes up by atomicAdd, the record keeps its slot (4 bytes a record).
//   compact  a lane per slot: the used slots (slot, key, count) to a list for the host, which
//            sorts the keys, applies min_reads and sends back region-or-none per listed slot.
//   scatter  that answer to map[slot].
//   mark / scan / write   per chunk as above: a record counts one hit iff map[slot] is a region;
//            the hit (region, record) lands at its scanned index.  order and emit follow as above.
// Which slot a key got depends on arrival order; the slot never leaves this file: the host orders
// by key, and the hit list is in record order.
//
// NWR_PACKED leaves the reads in HBM as the aligner's 2-bit batch (pack_result).  Emit is not run:
// no ASCII base and no quality is made.  The stream is region-major across the chunks, and only
// one chunk's records are on the device at a time, so a region's run from chunk c and its run
// from chunk c + 1 can meet inside a dword, and a chunk's runs are scattered over the stream.
// The shape chosen: all chunks' hit lists are collected and merged on the host first (16 bytes a
// hit, as before), which fixes every hit's final position; then one sweep per chunk (the chunk is
// still resident in a one-chunk call, else uploaded again) over the dwords that hold a base of it:
//   words   a thread per dword of a segment (a maximal run of final hits from this chunk): its
//           segment by binary search of the segments' thread bases, its hit by a bounded binary
//           search of the final offsets.  16 bases in one hit are 8 or 9 consecutive record bytes
//           by the parity of st + k: aligned dword loads (grp::load_dword), the halves of every
//           byte swapped at once, a shift by one code when odd.  Codes 1 2 8 4 are 0 1 2 3.  A
//           dword that the segment fills is stored once, whole; a dword that segments share is
//           OR-ed into the stream, which is zeroed once per call.  Exceptions set their bit in a
//           mask of one bit a base (OR, zeroed once) and are counted into sums[block].
//   scan    one block: the exclusive scan of the block sums; the chunk's count goes to the host.
//   exc     the second walk: (position, letter) into the chunk's own list at the scanned index.
// When the mask is whole: rank sums (the mask's bits per 256 words), scan, place (every listed
// exception to the slot that is the number of mask bits before its position: ascending positions
// whatever chunk a base came from), bounds (the same rank of every region's first position).
// Why this is deterministic: a final position belongs to one hit of one chunk, so every bit of
// the stream and of the mask is written by one thread, and integer OR into zeroed words does not
// depend on order; the places come from the finished mask alone; the chunk lists' indices come
// from scans.  No float, no arrival order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/crispr_nw.h"
#include "../../include/crispr_regions.h"
#include "group_device.h"
#include "front_device.h"
#include "host_dev.h"
#include "nw_bam.h"
#include "nw_device.h"

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
    const uint32_t* slot;      // nwr_discover: [cn] the chunk's records' table slots, kNoSlot = not kept
    const int32_t* map;        // nwr_discover: [cap] the slot's region, -1 = not emitted
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

// ---- nwr_discover ---------------------------------------------------------------------------

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr uint64_t kHashMul = 0x9E3779B97F4A7C15ull;
enum { kKept = 0, kDropped = 1, kAligned = 2, kDistinct = 3, kError = 4, kListed = 5, kCounters = 6 };

// The table: word 0 of a slot is never 0 for a key (bpstart carries a bias), word 1 is stored
// plus one; 0 is "empty" in both.
struct Table {
    unsigned long long* w0;
    unsigned long long* w1;
    uint32_t* count;
    uint64_t cap_mask;
    int shift;                 // 64 - log2(slots)
    uint64_t hash_mask;        // CRISPR_NWR_HASH_BITS
};

struct SpanArgs {
    const uint8_t* data;
    const int64_t* off;
    int32_t cn;
    int32_t flags;
    Table t;
    uint32_t* slot;            // [cn]
    unsigned long long* ctr;   // [kCounters]
};

struct Listed {
    uint64_t w0, w1;
    uint32_t slot, count;
};

// (ref, bpstart, bpend) in 16 bytes, exactly: ref < 2^31, |bpstart| < 2^46 and bpend - bpstart
// < 2^45 (pos < 2^31, at most 65535 ops of under 2^28 each).
constexpr int64_t kStartBias = (int64_t)1 << 47;
__host__ __device__ inline void pack_key(int32_t ref, int64_t bs, int64_t be, uint64_t* w0, uint64_t* w1) {
    *w0 = (uint64_t)(bs + kStartBias) | ((uint64_t)((uint32_t)ref & 0xFFFFu) << 48);
    *w1 = (uint64_t)(be - bs) | ((uint64_t)((uint32_t)ref >> 16) << 48);
}
inline void unpack_key(uint64_t w0, uint64_t w1, nwr_region* r) {
    const uint64_t m48 = ((uint64_t)1 << 48) - 1;
    r->ref_id = (int32_t)((w0 >> 48) | ((w1 >> 48) << 16));
    r->bpstart = (int64_t)(w0 & m48) - kStartBias;
    r->bpend = r->bpstart + (int64_t)(w1 & m48);
    r->reserved = 0;
}

__device__ inline uint64_t key_hash(uint64_t w0, uint64_t w1) {
    uint64_t x = (w0 ^ (w1 * kHashMul)) * 0xD6E8FEB86659FD93ull;
    x ^= x >> 32;
    x *= 0xD6E8FEB86659FD93ull;
    return x ^ (x >> 29);
}

// The span of the header's walk.  Kinds are BAM's op codes: M 0, I 1, D 2, N 3, S 4, H 5, P 6.
__device__ inline void span_step(uint32_t kind, int64_t len, int64_t pos, int64_t* bs, int64_t* be) {
    if (kind == 4) {
        if (*be == pos) *bs -= len;
        else *be += len;
    } else if (kind != 1 && kind != 5) {
        *be += len;
    }
}

__global__ __launch_bounds__(kBlk) void nwr_span_kernel(const SpanArgs a) {
    __shared__ uint32_t part[kBlk / 64][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    uint32_t kept = 0, dropped = 0, aligned = 0, fresh = 0;
    if (i < a.cn) {
        const uint8_t* r = a.data + a.off[i];
        const int32_t ref = (int32_t)ld32(r + nw_bam::kRefId);
        const uint32_t flag = ld16(r + nw_bam::kFlag);
        aligned = (flag & 0x904u) == 0;
        uint32_t found = kNoSlot;
        if (!(flag & 4u) && ref >= 0) {
            const int32_t n_op = (int32_t)ld16(r + nw_bam::kNCigar), l_seq = (int32_t)ld32(r + nw_bam::kLSeq);
            const uint8_t* cig = r + nw_bam::kName + r[nw_bam::kLReadName];
            if (!(l_seq > 0 && cig[4 * (int64_t)n_op + (l_seq + 1) / 2] != 0xFF)) {
                dropped = 1;
            } else {
                const bool eqx = (a.flags & NWR_EQX_AS_MATCH) != 0;
                const int64_t pos = (int64_t)(int32_t)ld32(r + nw_bam::kPos) + 1;
                int64_t bs = pos, be = pos, run = -1;      // run: the length a run of unsplit ops carries
                for (int k = 0; k < n_op; ++k) {
                    const uint32_t v = ld32(cig + 4 * k);
                    uint32_t op = v & 15u;
                    int64_t len = v >> 4;
                    if (op >= 7) {
                        if (eqx) {
                            if (op > 8) continue;
                            op = 0;
                        } else {
                            if (run < 0) run = len;
                            continue;
                        }
                    }
                    if (run >= 0) len = run, run = -1;
                    span_step(op, len, pos, &bs, &be);
                }
                if (run >= 0) span_step(0, run, pos, &bs, &be);
                uint64_t w0, w1;
                pack_key(ref, bs, be, &w0, &w1);
                w1 += 1;
                uint64_t s = ((key_hash(w0, w1) & a.t.hash_mask) * kHashMul) >> a.t.shift;
                for (uint64_t probe = 0; probe <= a.t.cap_mask; ++probe) {      // bounded by the table size
                    unsigned long long x = __hip_atomic_load(&a.t.w0[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (x == 0) {
                        x = atomicCAS(&a.t.w0[s], 0ull, (unsigned long long)w0);
                        if (x == 0) x = w0;
                    }
                    if (x == w0) {
                        unsigned long long y = __hip_atomic_load(&a.t.w1[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (y == 0) {
                            y = atomicCAS(&a.t.w1[s], 0ull, (unsigned long long)w1);
                            if (y == 0) y = w1, fresh = 1;
                        }
                        if (y == w1) {
                            atomicAdd(&a.t.count[s], 1u);
                            found = (uint32_t)s;
                            break;
                        }
                    }
                    s = (s + 1) & a.t.cap_mask;
                }
                if (found == kNoSlot) a.ctr[kError] = 1;      // a full table: cannot happen at load <= 1/2
                else kept = 1;
            }
        }
        a.slot[i] = found;
    }
    uint32_t v0 = kept, v1 = dropped, v2 = aligned, v3 = fresh;
    for (int s = 32; s > 0; s >>= 1) {
        v0 += __shfl_xor(v0, s);
        v1 += __shfl_xor(v1, s);
        v2 += __shfl_xor(v2, s);
        v3 += __shfl_xor(v3, s);
    }
    if (lane == 0) part[wave][0] = v0, part[wave][1] = v1, part[wave][2] = v2, part[wave][3] = v3;
    __syncthreads();
    if (threadIdx.x < 4) {
        uint32_t sum = 0;
        for (int w = 0; w < kBlk / 64; ++w) sum += part[w][threadIdx.x];
        if (sum) atomicAdd(&a.ctr[threadIdx.x], (unsigned long long)sum);      // (sums: no order shows)
    }
}

// The used slots to list[0 .. ctr[kListed]) in any order (the host sorts by key); cap entries
// at most are written.
__global__ __launch_bounds__(kBlk) void nwr_compact_kernel(const Table t, Listed* list, uint64_t cap,
                                                           unsigned long long* ctr) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
    const bool used = s <= t.cap_mask && t.w1[s] != 0;
    const unsigned long long at = grp::wave_reserve(used, &ctr[kListed]);
    if (used && at < cap) list[at] = Listed{t.w0[s], t.w1[s] - 1, (uint32_t)s, t.count[s]};
}

__global__ __launch_bounds__(kBlk) void nwr_scatter_kernel(const uint32_t* slots, const int32_t* reg, int64_t n,
                                                           uint64_t cap_mask, int32_t* map) {
    const int64_t e = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (e < n && slots[e] <= cap_mask) map[slots[e]] = reg[e];
}

__device__ inline uint32_t mark_of(const Args& a, int64_t i) {
    if (i >= a.cn) return 0;
    const uint32_t s = a.slot[i];
    return s != kNoSlot && a.map[s] >= 0;
}

__global__ __launch_bounds__(kBlk) void nwr_mark_kernel(const Args a) {
    __shared__ uint32_t part[kBlk / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    const uint32_t cnt = mark_of(a, i);
    if (i < a.cn) a.counts[i] = cnt;
    uint32_t v0 = cnt;
    for (int s = 32; s > 0; s >>= 1) v0 += __shfl_xor(v0, s);
    if (lane == 0) part[wave] = v0;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s0 = 0;
        for (int w = 0; w < kBlk / 64; ++w) s0 += part[w];
        a.sums[blockIdx.x] = s0;
        if (s0) atomicAdd(&a.totals[kHits], (unsigned long long)s0);
    }
}

// (region, record, 0, 0): the host fills en = l_seq, so this step reads no record byte.
__global__ __launch_bounds__(kBlk) void nwr_mark_write_kernel(const Args a) {
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
    if (cnt) a.hits[at] = make_uint4((uint32_t)a.map[a.slot[i]], (uint32_t)i, 0u, 0u);
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

// ---- NWR_PACKED: the hits as the aligner's 2-bit batch ----------------------------------------

constexpr int kPackBlk = 256;
constexpr int kRankBlk = 256;                  // mask words (32 positions each) per rank sum

// A run of consecutive final hits whose records lie in one chunk: final positions [p_lo, p_hi),
// p_lo < p_hi; its dwords are the threads [t0, t0 + (p_hi + 15) / 16 - p_lo / 16) of the sweep.
struct Seg {
    int64_t h_lo, h_hi, t0;
    uint32_t p_lo, p_hi;
};

struct PackArgs {
    const uint8_t* data;       // the chunk's records
    const EmitHit* eh;         // [n_hits] of the whole call, final order; seq within the hit's own chunk
    const uint32_t* ooff;      // [n_hits + 1] final positions
    const Seg* seg;            // the chunk's segments, ascending
    int32_t nseg;
    int64_t nthreads;          // the segments' dwords
    uint32_t* words;           // the call's stream, zeroed once
    uint32_t* mask;            // bit p % 32 of word p / 32: position p is an exception; zeroed once
    uint32_t* sums;            // [blocks] the sweep's exceptions per block, then their exclusive prefix
    int64_t blocks;
    int64_t* exc_pos;          // the chunk's own list, in sweep order
    uint8_t* exc_byte;
    int64_t n_exc;
};

// The BAM codes of final positions 16 w + k, k in [k0, k1), code k in bits 4 k of nib.
struct Piece {
    uint64_t nib;
    int64_t w;
    int k0, k1;
};

__device__ __forceinline__ Piece piece_at(const PackArgs& a, int64_t t) {
    int lo = 0, hi = a.nseg;                               // the last segment with t0 <= t
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.seg[mid].t0 <= t) lo = mid; else hi = mid;
    }
    const Seg s = a.seg[lo];
    Piece pc;
    pc.w = (int64_t)(s.p_lo >> 4) + (t - s.t0);
    const int64_t p0 = 16 * pc.w;
    const int64_t b0 = p0 > (int64_t)s.p_lo ? p0 : (int64_t)s.p_lo;
    const int64_t b1 = p0 + 16 < (int64_t)s.p_hi ? p0 + 16 : (int64_t)s.p_hi;      // b0 < b1: the dword holds a base of s
    pc.k0 = (int)(b0 - p0);
    pc.k1 = (int)(b1 - p0);
    pc.nib = 0;
    int64_t hl = s.h_lo, hh = s.h_hi;                      // the last hit of the segment with ooff <= b0
    while (hh - hl > 1) {                                  // (at most 31 steps: a chunk has under 2^31 hits)
        const int64_t mid = (hl + hh) >> 1;
        if ((int64_t)a.ooff[mid] <= b0) hl = mid; else hh = mid;
    }
    int64_t h = hl;
    EmitHit e = a.eh[h];
    int64_t h0 = a.ooff[h], h1 = a.ooff[h + 1];
    if (b1 - b0 == 16 && b1 <= h1) {                       // all 16 in this hit: 8 bytes, 9 when q is odd
        const int64_t q = (int64_t)e.st + (b0 - h0);
        const uint8_t* p = a.data + e.seq + (q >> 1);
        const int64_t L = 8 + (q & 1);
        uint64_t v = (uint64_t)grp::load_dword(p, 0, L) | ((uint64_t)grp::load_dword(p, 1, L) << 32);
        v = ((v & 0x0F0F0F0F0F0F0F0Full) << 4) | ((v >> 4) & 0x0F0F0F0F0F0F0F0Full);      // the first base of a byte is its high half
        if (q & 1) v = (v >> 4) | ((uint64_t)(grp::load_dword(p, 2, L) >> 4) << 60);
        pc.nib = v;
        return pc;
    }
    for (int64_t b = b0; b < b1; ++b) {                    // the end of one hit and the start of the next
        if (b >= h1) {
            do {
                ++h;
                h1 = a.ooff[h + 1];
            } while (b >= h1);                             // (b < p_hi = ooff[h_hi]: ends inside the segment)
            h0 = a.ooff[h];
            e = a.eh[h];
        }
        const int64_t q = (int64_t)e.st + (b - h0);
        const uint32_t two = a.data[e.seq + (q >> 1)];
        pc.nib |= (uint64_t)((q & 1) ? (two & 15u) : (two >> 4)) << (4 * (b - p0));
    }
    return pc;
}

// Codes 1, 2, 8, 4 (A, C, T, G) are bases 0, 1, 2, 3; every other code is an exception.
constexpr uint32_t kBaseOf = (1u << 4) | (2u << 16) | (3u << 8), kIsBase = 0x116u;

// One thread per dword of the chunk's segments.  A dword that one segment fills is stored once;
// a dword that segments share (of this chunk or of others) is OR-ed into the zeroed stream.
__global__ __launch_bounds__(kPackBlk) void nwr_pack_words_kernel(const PackArgs a) {
    __shared__ uint32_t part[kPackBlk / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * kPackBlk + threadIdx.x;
    uint32_t ne = 0;
    if (t < a.nthreads) {
        const Piece pc = piece_at(a, t);
        uint32_t out = 0, em = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t n = (uint32_t)(pc.nib >> (4 * k)) & 15u;
            if (k >= pc.k0 && k < pc.k1) {
                if ((kIsBase >> n) & 1u) out |= ((kBaseOf >> (2 * n)) & 3u) << (2 * k);
                else em |= 1u << k;
            }
        }
        if (pc.k1 - pc.k0 == 16) a.words[pc.w] = out;
        else if (out) atomicOr(&a.words[pc.w], out);       // (an OR: no order shows)
        if (em) atomicOr(&a.mask[pc.w >> 1], em << (16 * (int)(pc.w & 1)));
        ne = (uint32_t)__popc(em);
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

// One block: sums[b] becomes the exclusive prefix over the blocks before b; *total the sum.
__global__ __launch_bounds__(kScanBlk) void nwr_pack_scan_kernel(uint32_t* sums, int64_t blocks, int64_t* total) {
    __shared__ uint32_t sh[2][kScanBlk];
    const int t = threadIdx.x;
    const int64_t per = (blocks + kScanBlk - 1) / kScanBlk;
    const int64_t lo = std::min<int64_t>(blocks, t * per), hi = std::min<int64_t>(blocks, lo + per);
    uint32_t mine = 0;
    for (int64_t b = lo; b < hi; ++b) mine += sums[b];
    int cur = 0;
    sh[0][t] = mine;
    __syncthreads();
    for (int d = 1; d < kScanBlk; d <<= 1) {
        sh[cur ^ 1][t] = sh[cur][t] + (t >= d ? sh[cur][t - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    uint32_t run = sh[cur][t] - mine;
    if (t == kScanBlk - 1) *total = (int64_t)sh[cur][t];
    for (int64_t b = lo; b < hi; ++b) {
        const uint32_t v = sums[b];
        sums[b] = run;
        run += v;
    }
}

// The second walk: the chunk's exceptions (position, letter) at the block's base + the
// exceptions of the block's threads before this one.
__global__ __launch_bounds__(kPackBlk) void nwr_pack_exc_kernel(const PackArgs a) {
    __shared__ uint32_t part[kPackBlk / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * kPackBlk + threadIdx.x;
    Piece pc{0, 0, 0, 0};
    uint32_t em = 0;
    if (t < a.nthreads) {
        pc = piece_at(a, t);
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k >= pc.k0 && k < pc.k1 && !((kIsBase >> ((uint32_t)(pc.nib >> (4 * k)) & 15u)) & 1u)) em |= 1u << k;
    }
    const uint32_t ne = (uint32_t)__popc(em);
    uint32_t x = ne;
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t y = __shfl_up(x, s);
        if (lane >= s) x += y;
    }
    if (lane == 63) part[wave] = x;
    __syncthreads();
    int64_t slot = (int64_t)a.sums[blockIdx.x] + (x - ne);
    for (int v = 0; v < wave; ++v) slot += part[v];
    for (; em; em &= em - 1) {
        const int k = __ffs((int)em) - 1;
        const uint32_t code = (uint32_t)(pc.nib >> (4 * k)) & 15u;
        if (slot < a.n_exc) {                              // (always: the words kernel's sum)
            a.exc_pos[slot] = 16 * pc.w + k;
            a.exc_byte[slot] = (uint8_t)(((code & 8u) ? kNibHi : kNibLo) >> (8 * (code & 7u)));
        }
        ++slot;
    }
}

// The exceptions of every kRankBlk mask words, for the scan.
__global__ __launch_bounds__(kRankBlk) void nwr_rank_sums_kernel(const uint32_t* mask, uint32_t* rsums) {
    __shared__ uint32_t part[kRankBlk / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t v = (uint32_t)__popc(mask[(int64_t)blockIdx.x * kRankBlk + threadIdx.x]);      // (the mask is padded to whole blocks)
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    if (lane == 0) part[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kRankBlk / 64; ++w) s += part[w];
        rsums[blockIdx.x] = s;
    }
}

// The exceptions before position p < 32 * (mask words): the place of p's own in the final list.
__device__ inline int64_t rank_of(const uint32_t* mask, const uint32_t* rsums, int64_t p) {
    const int64_t word = p >> 5, first = word & ~(int64_t)(kRankBlk - 1);
    int64_t r = rsums[word / kRankBlk];
    for (int64_t i = first; i < word; ++i) r += __popc(mask[i]);      // (under kRankBlk steps)
    return r + __popc(mask[word] & ((1u << (p & 31)) - 1u));
}

// A chunk's list to its places in the call's: ascending positions whatever chunk a base came from.
__global__ __launch_bounds__(256) void nwr_exc_place_kernel(const int64_t* lpos, const uint8_t* lbyte, int64_t n,
                                                            const uint32_t* mask, const uint32_t* rsums, int64_t n_exc,
                                                            int64_t* exc_pos, uint8_t* exc_byte) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t p = lpos[i], slot = rank_of(mask, rsums, p);
    if (slot < n_exc) {                                    // (always: the mask holds n_exc bits)
        exc_pos[slot] = p;
        exc_byte[slot] = lbyte[i];
    }
}

// gexc[g] = the exceptions before region g's first position rpos[g], g in [0, n_regions].
__global__ __launch_bounds__(256) void nwr_exc_bounds_kernel(const int64_t* rpos, int64_t n, int64_t total,
                                                             const uint32_t* mask, const uint32_t* rsums, int64_t n_exc,
                                                             int64_t* gexc) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const int64_t p = rpos[g];
    gexc[g] = p >= total ? n_exc : rank_of(mask, rsums, p);
}

// The hits of one chunk (or of the whole call) in region-major order.
struct Hits {
    std::vector<int32_t> reg, st, en;
    std::vector<int64_t> src, toff{0};
    std::vector<uint8_t> text, quals;
};

struct Result {
    std::vector<int64_t> region_off;
    Hits h;
    // nwr_discover: the regions in result order, their whole-call counts, nwr_fetch_regions' stats
    bool discovered = false;
    std::vector<nwr_region> regions;
    std::vector<int64_t> n_records;
    int64_t stats[4] = {0, 0, 0, 0};
    // NWR_PACKED: the batch in HBM, the result's own (it outlives the context that made it)
    bool packed = false;
    int device = 0;
    int64_t n_exc = 0;
    float pack_ms = 0.0f;
    std::vector<uint16_t> lens16;
    std::vector<int64_t> gexc;      // [n_regions + 1]
    hd::DevBuf<uint32_t> d_words;
    hd::DevBuf<uint16_t> d_lens16;
    hd::DevBuf<int64_t> d_exc_pos, d_gbase;
    hd::DevBuf<uint8_t> d_exc_byte;
    hipEvent_t ready = nullptr;     // recorded behind the packer
    ~Result() {
        if (!packed) return;
        (void)hipSetDevice(device);
        if (ready) (void)hipEventDestroy(ready);
    }
};

}  // namespace nwr

struct nwr_ctx : hd::DevContext {
    int64_t chunk_records = 0;      // 0: by bytes
    hd::DevBuf<uint8_t> d_data;
    hd::DevBuf<int64_t> d_off, d_rstart, d_rend;
    hd::DevBuf<int32_t> d_rref;
    hd::DevBuf<uint32_t> d_counts, d_sums, d_ooff, d_text, d_quals;
    hd::DevBuf<unsigned long long> d_totals;
    hd::DevBuf<uint4> d_hits;
    hd::DevBuf<nwr::EmitHit> d_eh;
    // nwr_discover
    int hash_bits = 64;             // CRISPR_NWR_HASH_BITS
    hd::DevBuf<unsigned long long> d_w0, d_w1, d_ctr;
    hd::DevBuf<uint32_t> d_tcount, d_slot, d_lslot;
    hd::DevBuf<int32_t> d_map, d_lreg;
    hd::DevBuf<nwr::Listed> d_list;
    // NWR_PACKED: what the packer needs beside the result's own buffers
    hd::DevBuf<nwr::Seg> d_seg;
    hd::DevBuf<uint32_t> d_mask, d_psums, d_rsums;
    hd::DevBuf<int64_t> d_ptotal, d_rpos, d_gexc;
};

namespace {

using hd::fail;

inline uint32_t h16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t h32(const uint8_t* p) { return h16(p) | (h16(p + 2) << 16); }

int finish_chunk(nwr_ctx* c, const nwr_bam* bam, int64_t r0, int64_t r1, const std::vector<int64_t>& off, nwr::Args a,
                 int64_t nh, void (*write_kernel)(const nwr::Args), bool whole, const std::vector<int32_t>& perm,
                 int64_t n_regions, std::vector<int64_t>* cursor, nwr::Hits* out, float* kernel_ms);

// Where the chunk that starts at record r0 ends.
int64_t chunk_end(const nwr_ctx* c, const nwr_bam* bam, int64_t r0, int64_t n) {
    if (c->chunk_records > 0) return std::min(n, r0 + c->chunk_records);
    const int64_t r1 = std::min(n, r0 + nwr::kChunkRecords);
    const int64_t* o = bam->off.data();
    const int64_t* e = std::upper_bound(o + r0 + 1, o + r1 + 1, o[r0] + nwr::kChunkBytes);
    return std::max<int64_t>(r0 + 1, (e - o) - 1);      // (one record at least, whatever its size)
}

// The chunk's records and their starts to d_data / d_off; off gets the starts.
int upload_chunk(nwr_ctx* c, const nwr_bam* bam, int64_t r0, int64_t r1, bool offsets_too, std::vector<int64_t>* off,
                 float* upload_ms) {
    const int64_t cn = r1 - r0, base = bam->off[(size_t)r0], nbytes = bam->off[(size_t)r1] - base;
    off->resize((size_t)cn + 1);
    for (int64_t i = 0; i <= cn; ++i) (*off)[(size_t)i] = bam->off[(size_t)(r0 + i)] - base;
    if (!upload_ms) return NW_OK;      // (the records are in d_data already)
    HIP_TRY(c, c->d_data.reserve((size_t)nbytes));
    HIP_TRY(c, c->d_off.reserve((size_t)cn + 1));
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(c, hipMemcpyAsync(c->d_data.p, bam->data.data() + base, (size_t)nbytes, hipMemcpyHostToDevice, c->stream));
    if (offsets_too)
        HIP_TRY(c, hipMemcpyAsync(c->d_off.p, off->data(), sizeof(int64_t) * (size_t)(cn + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *upload_ms += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return NW_OK;
}

// Pass 1 of nwr_discover over one chunk: spans into the table, the records' slots.
int span_chunk(nwr_ctx* c, const nwr_bam* bam, int64_t r0, int64_t r1, int32_t flags, const nwr::Table& t, float* kernel_ms,
               float* upload_ms) {
    std::vector<int64_t> off;
    const int rc = upload_chunk(c, bam, r0, r1, true, &off, upload_ms);
    if (rc != NW_OK) return rc;
    nwr::SpanArgs sa{};
    sa.data = c->d_data.p;
    sa.off = c->d_off.p;
    sa.cn = (int32_t)(r1 - r0);
    sa.flags = flags;
    sa.t = t;
    sa.slot = c->d_slot.p + r0;
    sa.ctr = c->d_ctr.p;
    HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
    hipLaunchKernelGGL(nwr::nwr_span_kernel, dim3((unsigned)((sa.cn + nwr::kBlk - 1) / nwr::kBlk)), dim3(nwr::kBlk), 0, c->stream, sa);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    *kernel_ms += ms;
    return NW_OK;
}

// Pass 2 over one chunk: the records of the emitted regions as hits, ordered and emitted.
int emit_chunk(nwr_ctx* c, const nwr_bam* bam, int64_t r0, int64_t r1, int32_t flags, bool resident, int64_t n_regions,
               std::vector<int64_t>* cursor, nwr::Hits* out, float* kernel_ms, float* upload_ms) {
    hipStream_t st = c->stream;
    const int64_t cn = r1 - r0, blocks = (cn + nwr::kBlk - 1) / nwr::kBlk;
    HIP_TRY(c, c->d_counts.reserve((size_t)cn));
    HIP_TRY(c, c->d_sums.reserve((size_t)blocks));
    HIP_TRY(c, c->d_totals.reserve(2));
    HIP_TRY(c, hipMemsetAsync(c->d_totals.p, 0, 2 * sizeof(unsigned long long), st));
    nwr::Args a{};
    a.cn = (int32_t)cn;
    a.flags = flags;
    a.counts = c->d_counts.p;
    a.sums = c->d_sums.p;
    a.blocks = blocks;
    a.totals = c->d_totals.p;
    a.slot = c->d_slot.p + r0;
    a.map = c->d_map.p;
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(nwr::nwr_mark_kernel, dim3((unsigned)blocks), dim3(nwr::kBlk), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    unsigned long long totals[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(totals, a.totals, sizeof totals, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    *kernel_ms += ms;
    const int64_t nh = (int64_t)totals[nwr::kHits];
    if (nh > nwr::kMaxHits)
        return fail(c, NW_E_UNSUPPORTED, "%lld hits in the chunk of records %lld to %lld: at most 2^30 (use a smaller CRISPR_NWR_CHUNK)",
                    (long long)nh, (long long)r0, (long long)r1);
    if (nh == 0) return NW_OK;      // (a chunk of off-target records alone is not uploaded again)
    std::vector<int64_t> off;
    // (a packed call's write kernel reads no record byte: the packer uploads the chunk when its turn comes)
    const int rc = upload_chunk(c, bam, r0, r1, false, &off, resident || (flags & NWR_PACKED) ? nullptr : upload_ms);
    if (rc != NW_OK) return rc;
    a.data = c->d_data.p;
    static const std::vector<int32_t> no_perm;
    return finish_chunk(c, bam, r0, r1, off, a, nh, nwr::nwr_mark_write_kernel, true, no_perm, n_regions, cursor, out, kernel_ms);
}

// One chunk: records [r0, r1) of bam; its hits in region-major order (the caller's regions).
int run_chunk(nwr_ctx* c, const nwr_bam* bam, int64_t r0, int64_t r1, nwr::Args a, const std::vector<int32_t>& perm,
              int64_t n_regions, std::vector<int64_t>* cursor, nwr::Hits* out, int64_t* n_no_seq, float* kernel_ms,
              float* upload_ms) {
    hipStream_t st = c->stream;
    const int64_t cn = r1 - r0, base = bam->off[(size_t)r0], nbytes = bam->off[(size_t)r1] - base;
    const int64_t blocks = (cn + nwr::kBlk - 1) / nwr::kBlk;
    std::vector<int64_t> off((size_t)cn + 1);
    for (int64_t i = 0; i <= cn; ++i) off[(size_t)i] = bam->off[(size_t)(r0 + i)] - base;
    HIP_TRY(c, c->d_data.reserve((size_t)nbytes));
    HIP_TRY(c, c->d_off.reserve((size_t)cn + 1));
    HIP_TRY(c, c->d_counts.reserve((size_t)cn));
    HIP_TRY(c, c->d_sums.reserve((size_t)blocks));
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(c, hipMemcpyAsync(c->d_data.p, bam->data.data() + base, (size_t)nbytes, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_off.p, off.data(), sizeof(int64_t) * (size_t)(cn + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(c->d_totals.p, 0, 2 * sizeof(unsigned long long), st));
    HIP_TRY(c, hipStreamSynchronize(st));
    *upload_ms += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    a.data = c->d_data.p;
    a.off = c->d_off.p;
    a.cn = (int32_t)cn;
    a.counts = c->d_counts.p;
    a.sums = c->d_sums.p;
    a.blocks = blocks;
    a.totals = c->d_totals.p;
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(nwr::nwr_count_kernel, dim3((unsigned)blocks), dim3(nwr::kBlk), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    unsigned long long totals[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(totals, a.totals, sizeof totals, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    *kernel_ms += ms;
    *n_no_seq += (int64_t)totals[nwr::kNoSeq];
    const int64_t nh = (int64_t)totals[nwr::kHits];
    if (nh > nwr::kMaxHits)
        return fail(c, NW_E_UNSUPPORTED, "%lld hits in the chunk of records %lld to %lld: at most 2^30 (use a smaller CRISPR_NWR_CHUNK)",
                    (long long)nh, (long long)r0, (long long)r1);
    if (nh == 0) return NW_OK;
    return finish_chunk(c, bam, r0, r1, off, a, nh, nwr::nwr_write_kernel, false, perm, n_regions, cursor, out, kernel_ms);
}

// The rest of a chunk once its hits are counted (a.counts, a.sums, nh of them) and its records
// are in d_data: scan, write, the host's order step, emit.  `whole`: the hits carry no st / en,
// every read is its record's whole sequence (nwr_discover).
int finish_chunk(nwr_ctx* c, const nwr_bam* bam, int64_t r0, int64_t r1, const std::vector<int64_t>& off, nwr::Args a,
                 int64_t nh, void (*write_kernel)(const nwr::Args), bool whole, const std::vector<int32_t>& perm,
                 int64_t n_regions, std::vector<int64_t>* cursor, nwr::Hits* out, float* kernel_ms) {
    hipStream_t st = c->stream;
    const int64_t cn = r1 - r0, blocks = a.blocks;
    float ms = 0.0f;
    HIP_TRY(c, c->d_hits.reserve((size_t)nh));
    a.hits = c->d_hits.p;
    HIP_TRY(c, hipEventRecord(c->ev[2], st));
    hipLaunchKernelGGL(nwr::nwr_scan_kernel, dim3(1), dim3(nwr::kScanBlk), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(write_kernel, dim3((unsigned)blocks), dim3(nwr::kBlk), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[3], st));
    std::vector<uint4> hits((size_t)nh);
    HIP_TRY(c, hipMemcpyAsync(hits.data(), a.hits, sizeof(uint4) * (size_t)nh, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
    *kernel_ms += ms;

    // region-major, record order within a region: a stable counting sort on the caller's region
    const bool by_ref = whole || (a.flags & NWR_BY_REFERENCE) != 0;      // the hit's region is the caller's already
    std::vector<int64_t>& cur = *cursor;
    std::fill(cur.begin(), cur.end(), 0);
    for (const uint4& h : hits) {
        if ((int64_t)h.x >= (by_ref ? n_regions : (int64_t)perm.size()) || (int64_t)h.y >= cn)
            return fail(c, NW_E_STATE, "inconsistent hit");
        ++cur[(size_t)(by_ref ? (int32_t)h.x : perm[h.x]) + 1];
    }
    for (int64_t g = 0; g < n_regions; ++g) cur[(size_t)g + 1] += cur[(size_t)g];
    out->reg.resize((size_t)nh);
    out->src.resize((size_t)nh);
    out->st.resize((size_t)nh);
    out->en.resize((size_t)nh);
    std::vector<nwr::EmitHit> eh((size_t)nh);
    std::vector<int32_t> len((size_t)nh);
    for (uint4 h : hits) {
        const int32_t g = by_ref ? (int32_t)h.x : perm[h.x];
        const size_t k = (size_t)cur[(size_t)g]++;
        const uint8_t* r = bam->data.data() + bam->off[(size_t)(r0 + h.y)];
        const int64_t l_seq = (int32_t)h32(r + nw_bam::kLSeq);
        if (whole) h.z = 0, h.w = (uint32_t)l_seq;
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
        return fail(c, NW_E_UNSUPPORTED, "%lld output bytes in the chunk of records %lld to %lld: under 2^32 (use a smaller CRISPR_NWR_CHUNK)",
                    (long long)total, (long long)r0, (long long)r1);
    if (total == 0 || (a.flags & NWR_PACKED)) return NW_OK;      // (packed: the bases are read by pack_result)
    std::vector<uint32_t> ooff((size_t)nh + 1);
    for (int64_t k = 0; k <= nh; ++k) ooff[(size_t)k] = (uint32_t)out->toff[(size_t)k];
    const int64_t words = (total + 3) / 4;
    HIP_TRY(c, c->d_eh.reserve((size_t)nh));
    HIP_TRY(c, c->d_ooff.reserve((size_t)nh + 1));
    HIP_TRY(c, c->d_text.reserve((size_t)words));
    HIP_TRY(c, c->d_quals.reserve((size_t)words));
    HIP_TRY(c, hipMemcpyAsync(c->d_eh.p, eh.data(), sizeof(nwr::EmitHit) * (size_t)nh, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_ooff.p, ooff.data(), sizeof(uint32_t) * (size_t)(nh + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(c->ev[4], st));
    hipLaunchKernelGGL(nwr::nwr_emit_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, c->d_data.p, c->d_eh.p,
                       c->d_ooff.p, nh, total, c->d_text.p, c->d_quals.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[5], st));
    out->text.resize((size_t)words * 4);
    out->quals.resize((size_t)words * 4);
    HIP_TRY(c, hipMemcpyAsync(out->text.data(), c->d_text.p, (size_t)words * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(out->quals.data(), c->d_quals.p, (size_t)words * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[4], c->ev[5]));
    *kernel_ms += ms;
    out->text.resize((size_t)total);
    out->quals.resize((size_t)total);
    return NW_OK;
}

// The chunks' hits (each region-major) as one region-major list, the chunks in order in a region.
void merge_chunks(std::vector<nwr::Hits>& chunks, int64_t n_regions, nwr::Result* res, bool packed) {
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
            if (packed) break;      // (no chunk holds text)
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

// NWR_PACKED, after merge_chunks: the merged hits of R as the aligner's batch in R's own buffers.
// ranges are the call's chunks; a one-chunk call still has its records in d_data.
int pack_result(nwr_ctx* c, const nwr_bam* bam, const std::vector<std::pair<int64_t, int64_t>>& ranges, nwr::Result* R,
                float* upload_ms) {
    hipStream_t st = c->stream;
    const nwr::Hits& h = R->h;
    const int64_t nh = (int64_t)h.reg.size(), total = h.toff.back(), n_regions = (int64_t)R->region_off.size() - 1;
    R->packed = true;
    R->device = c->device;
    R->gexc.assign((size_t)n_regions + 1, 0);
    R->lens16.resize((size_t)nh);
    for (int64_t k = 0; k < nh; ++k) {
        const int64_t len = h.toff[(size_t)k + 1] - h.toff[(size_t)k];
        if (len > 65535)
            return fail(c, NW_E_UNSUPPORTED, "record %lld gives a read of %lld bases: a packed read holds at most 65535",
                        (long long)h.src[(size_t)k], (long long)len);
        R->lens16[(size_t)k] = (uint16_t)len;
    }
    if ((uint64_t)total >= (1ull << 32))
        return fail(c, NW_E_UNSUPPORTED, "%lld bases in the call: 2^32 or more in one packed call are not supported",
                    (long long)total);
    if (nh == 0) return NW_OK;
    HIP_TRY(c, hipEventCreate(&R->ready));
    const int64_t nwords = (total + 15) / 16;
    const int64_t mblocks = ((total + 31) / 32 + nwr::kRankBlk - 1) / nwr::kRankBlk + 1, mwords = mblocks * nwr::kRankBlk;
    HIP_TRY(c, R->d_words.reserve((size_t)nwords + 16));      // (the adoption's copies stay inside)
    HIP_TRY(c, R->d_lens16.reserve((size_t)nh));
    HIP_TRY(c, hipMemsetAsync(R->d_words.p, 0, sizeof(uint32_t) * (size_t)(nwords + 16), st));
    HIP_TRY(c, hipMemcpyAsync(R->d_lens16.p, R->lens16.data(), sizeof(uint16_t) * (size_t)nh, hipMemcpyHostToDevice, st));
    if (total == 0) {
        HIP_TRY(c, hipEventRecord(R->ready, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        return NW_OK;
    }

    // every final hit: where its bases start within its own chunk's records, and its chunk
    std::vector<nwr::EmitHit> eh((size_t)nh);
    std::vector<uint32_t> ooff((size_t)nh + 1);
    std::vector<std::vector<nwr::Seg>> segs(ranges.size());
    std::vector<int64_t> starts(ranges.size());
    for (size_t x = 0; x < ranges.size(); ++x) starts[x] = ranges[x].first;
    int64_t run_lo = 0;
    size_t run_chunk_ix = 0;
    auto close_run = [&](int64_t k) {      // final hits [run_lo, k) lie in chunk run_chunk_ix
        if (k > run_lo && h.toff[(size_t)k] > h.toff[(size_t)run_lo])
            segs[run_chunk_ix].push_back(nwr::Seg{run_lo, k, 0, (uint32_t)h.toff[(size_t)run_lo], (uint32_t)h.toff[(size_t)k]});
    };
    for (int64_t k = 0; k < nh; ++k) {
        const int64_t rec = h.src[(size_t)k];
        const size_t x = (size_t)(std::upper_bound(starts.begin(), starts.end(), rec) - starts.begin()) - 1;
        if (k == 0) run_chunk_ix = x;
        if (x != run_chunk_ix) {
            close_run(k);
            run_lo = k;
            run_chunk_ix = x;
        }
        const uint8_t* r = bam->data.data() + bam->off[(size_t)rec];
        const int64_t l_seq = (int32_t)h32(r + nw_bam::kLSeq);
        eh[(size_t)k].seq = bam->off[(size_t)rec] - bam->off[(size_t)ranges[x].first] + nw_bam::kName + r[nw_bam::kLReadName] +
                            4 * (int64_t)h16(r + nw_bam::kNCigar);
        eh[(size_t)k].l_seq = (int32_t)l_seq;
        eh[(size_t)k].st = (int32_t)std::min<int64_t>(h.st[(size_t)k], l_seq);
        ooff[(size_t)k] = (uint32_t)h.toff[(size_t)k];
    }
    close_run(nh);
    ooff[(size_t)nh] = (uint32_t)total;

    HIP_TRY(c, c->d_eh.reserve((size_t)nh));
    HIP_TRY(c, c->d_ooff.reserve((size_t)nh + 1));
    HIP_TRY(c, c->d_mask.reserve((size_t)mwords));
    HIP_TRY(c, c->d_rsums.reserve((size_t)mblocks));
    HIP_TRY(c, c->d_ptotal.reserve(1));
    HIP_TRY(c, hipMemcpyAsync(c->d_eh.p, eh.data(), sizeof(nwr::EmitHit) * (size_t)nh, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_ooff.p, ooff.data(), sizeof(uint32_t) * (size_t)(nh + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(c->d_mask.p, 0, sizeof(uint32_t) * (size_t)mwords, st));

    // a sweep per chunk; its exceptions wait in a list of their own for the mask to be whole
    struct Local {
        hd::DevBuf<int64_t> pos;
        hd::DevBuf<uint8_t> byte;
        int64_t n = 0;
    };
    std::vector<std::unique_ptr<Local>> locals;
    float ms = 0.0f;
    int64_t sum_exc = 0;
    for (size_t x = 0; x < ranges.size(); ++x) {
        std::vector<nwr::Seg>& sg = segs[x];
        if (sg.empty()) continue;
        int64_t nt = 0;
        for (nwr::Seg& s : sg) {
            s.t0 = nt;
            nt += (int64_t)(((uint64_t)s.p_hi + 15) / 16) - (int64_t)(s.p_lo / 16);
        }
        if (ranges.size() > 1) {
            std::vector<int64_t> off;
            const int rc = upload_chunk(c, bam, ranges[x].first, ranges[x].second, false, &off, upload_ms);
            if (rc != NW_OK) return rc;
        }
        nwr::PackArgs a{};
        a.data = c->d_data.p;
        a.eh = c->d_eh.p;
        a.ooff = c->d_ooff.p;
        a.nseg = (int32_t)sg.size();
        a.nthreads = nt;
        a.words = R->d_words.p;
        a.mask = c->d_mask.p;
        a.blocks = (nt + nwr::kPackBlk - 1) / nwr::kPackBlk;
        HIP_TRY(c, c->d_seg.reserve(sg.size()));
        HIP_TRY(c, c->d_psums.reserve((size_t)a.blocks));
        HIP_TRY(c, hipMemcpyAsync(c->d_seg.p, sg.data(), sizeof(nwr::Seg) * sg.size(), hipMemcpyHostToDevice, st));
        a.seg = c->d_seg.p;
        a.sums = c->d_psums.p;
        HIP_TRY(c, hipEventRecord(c->ev[0], st));
        hipLaunchKernelGGL(nwr::nwr_pack_words_kernel, dim3((unsigned)a.blocks), dim3(nwr::kPackBlk), 0, st, a);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(nwr::nwr_pack_scan_kernel, dim3(1), dim3(nwr::kScanBlk), 0, st, a.sums, a.blocks, c->d_ptotal.p);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->ev[1], st));
        int64_t ne = 0;
        HIP_TRY(c, hipMemcpyAsync(&ne, c->d_ptotal.p, sizeof ne, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));      // (the segments above are read by the copy)
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        R->pack_ms += ms;
        if (ne < 0 || ne > total - sum_exc) return fail(c, NW_E_STATE, "inconsistent exception count");
        if (ne == 0) continue;
        sum_exc += ne;
        locals.emplace_back(new Local());
        Local& l = *locals.back();
        l.n = ne;
        HIP_TRY(c, l.pos.reserve((size_t)ne));
        HIP_TRY(c, l.byte.reserve((size_t)ne));
        a.n_exc = ne;
        a.exc_pos = l.pos.p;
        a.exc_byte = l.byte.p;
        HIP_TRY(c, hipEventRecord(c->ev[0], st));
        hipLaunchKernelGGL(nwr::nwr_pack_exc_kernel, dim3((unsigned)a.blocks), dim3(nwr::kPackBlk), 0, st, a);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->ev[1], st));
        HIP_TRY(c, hipStreamSynchronize(st));      // (the next chunk overwrites d_data)
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        R->pack_ms += ms;
    }
    if (sum_exc > 0) {
        // the mask is whole: every exception's place in the call's list, and the regions' bounds
        std::vector<int64_t> rpos((size_t)n_regions + 1);
        for (int64_t g = 0; g <= n_regions; ++g) rpos[(size_t)g] = h.toff[(size_t)R->region_off[(size_t)g]];
        HIP_TRY(c, R->d_exc_pos.reserve((size_t)sum_exc));
        HIP_TRY(c, R->d_exc_byte.reserve((size_t)sum_exc));
        HIP_TRY(c, c->d_rpos.reserve((size_t)n_regions + 1));
        HIP_TRY(c, c->d_gexc.reserve((size_t)n_regions + 1));
        HIP_TRY(c, hipMemcpyAsync(c->d_rpos.p, rpos.data(), sizeof(int64_t) * (size_t)(n_regions + 1), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipEventRecord(c->ev[0], st));
        hipLaunchKernelGGL(nwr::nwr_rank_sums_kernel, dim3((unsigned)mblocks), dim3(nwr::kRankBlk), 0, st,
                           (const uint32_t*)c->d_mask.p, c->d_rsums.p);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(nwr::nwr_pack_scan_kernel, dim3(1), dim3(nwr::kScanBlk), 0, st, c->d_rsums.p, mblocks, c->d_ptotal.p);
        HIP_TRY(c, hipGetLastError());
        for (const auto& l : locals) {
            hipLaunchKernelGGL(nwr::nwr_exc_place_kernel, dim3((unsigned)((l->n + 255) / 256)), dim3(256), 0, st,
                               (const int64_t*)l->pos.p, (const uint8_t*)l->byte.p, l->n, (const uint32_t*)c->d_mask.p,
                               (const uint32_t*)c->d_rsums.p, sum_exc, R->d_exc_pos.p, R->d_exc_byte.p);
            HIP_TRY(c, hipGetLastError());
        }
        hipLaunchKernelGGL(nwr::nwr_exc_bounds_kernel, dim3((unsigned)((n_regions + 1 + 255) / 256)), dim3(256), 0, st,
                           (const int64_t*)c->d_rpos.p, n_regions + 1, total, (const uint32_t*)c->d_mask.p,
                           (const uint32_t*)c->d_rsums.p, sum_exc, c->d_gexc.p);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->ev[1], st));
        int64_t in_mask = 0;
        HIP_TRY(c, hipMemcpyAsync(&in_mask, c->d_ptotal.p, sizeof in_mask, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(R->gexc.data(), c->d_gexc.p, sizeof(int64_t) * (size_t)(n_regions + 1), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipEventRecord(R->ready, st));
        HIP_TRY(c, hipStreamSynchronize(st));      // (the chunks' lists go out of scope)
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        R->pack_ms += ms;
        if (in_mask != sum_exc) return fail(c, NW_E_STATE, "inconsistent exception mask");
    } else {
        HIP_TRY(c, hipEventRecord(R->ready, st));
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    R->n_exc = sum_exc;
    return NW_OK;
}

}  // namespace

extern "C" {

int nwr_create(int device, nwr_ctx** out) {
    const int rc = hd::create_context(device, 6, out);
    if (rc != NW_OK) return rc;
    nwr_ctx* c = *out;
    if (const char* e = std::getenv("CRISPR_NWR_CHUNK"))
        c->chunk_records = std::max<int64_t>(0, std::min<int64_t>(std::atoll(e), nwr::kChunkRecords));
    c->hash_bits = grp::env_hash_bits("CRISPR_NWR_HASH_BITS");
    return NW_OK;
}

void nwr_destroy(nwr_ctx* c) { hd::destroy_context(c); }

const char* nwr_last_error(const nwr_ctx* c) { return c ? c->err.c_str() : "null context"; }

int nwr_extract(nwr_ctx* c, const nwr_bam* bam, const nwr_region* regions, int64_t n_regions, int32_t flags,
                nwr_result* res) {
    if (!c) return NW_E_INVALID;
    if (!bam || !res) return fail(c, NW_E_INVALID, "null argument");
    std::memset(res, 0, sizeof *res);
    if (flags & ~(NWR_BY_REFERENCE | NWR_EQX_AS_MATCH | NWR_PACKED)) return fail(c, NW_E_INVALID, "unknown flags %d", (int)flags);
    const bool packed = (flags & NWR_PACKED) != 0;
    const bool by_ref = (flags & NWR_BY_REFERENCE) != 0;
    if (by_ref) n_regions = (int64_t)bam->ref_len.size();
    if (n_regions < 0 || (!by_ref && n_regions > 0 && !regions)) return fail(c, NW_E_INVALID, "null regions");
    if (n_regions > NWR_MAX_REGIONS)
        return fail(c, NW_E_UNSUPPORTED, "%lld regions: at most %d are supported", (long long)n_regions, NWR_MAX_REGIONS);
    const int64_t n = (int64_t)bam->off.size() - 1;
    nwr::Result* R = new nwr::Result();
    R->region_off.assign((size_t)n_regions + 1, 0);
    res->n_regions = n_regions;
    res->handle = R;
    if (packed) {      // (an empty result is a packed one all the same)
        R->packed = true;
        R->device = c->device;
        R->gexc.assign((size_t)n_regions + 1, 0);
    }
    if (n <= 0 || n_regions == 0) return NW_OK;

    auto bail = [&](int rc) {
        delete R;
        res->handle = nullptr;
        return rc;
    };
    nwr::Args a{};
    a.flags = flags;
    std::vector<int32_t> perm;
    if (hipSetDevice(c->device) != hipSuccess) return bail(fail(c, NW_E_HIP, "hipSetDevice failed"));
    int rc = [&]() -> int {
        HIP_TRY(c, c->d_totals.reserve(2));
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
        HIP_TRY(c, c->d_rref.reserve((size_t)n_regions));
        HIP_TRY(c, c->d_rstart.reserve((size_t)n_regions));
        HIP_TRY(c, c->d_rend.reserve((size_t)n_regions));
        HIP_TRY(c, hipMemcpy(c->d_rref.p, rref.data(), sizeof(int32_t) * (size_t)n_regions, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(c->d_rstart.p, rstart.data(), sizeof(int64_t) * (size_t)n_regions, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(c->d_rend.p, rend.data(), sizeof(int64_t) * (size_t)n_regions, hipMemcpyHostToDevice));
        a.nreg = (int32_t)n_regions;
        a.rref = c->d_rref.p;
        a.rstart = c->d_rstart.p;
        a.rend = c->d_rend.p;
        return NW_OK;
    }();
    if (rc != NW_OK) return bail(rc);

    std::vector<nwr::Hits> chunks;
    std::vector<int64_t> cursor((size_t)n_regions + 1);
    std::vector<std::pair<int64_t, int64_t>> ranges;
    for (int64_t r0 = 0; r0 < n;) {
        const int64_t r1 = chunk_end(c, bam, r0, n);
        nwr::Hits h;
        rc = run_chunk(c, bam, r0, r1, a, perm, n_regions, &cursor, &h, &res->n_no_seq, &res->kernel_ms, &res->upload_ms);
        if (rc != NW_OK) return bail(rc);
        if (!h.reg.empty()) chunks.push_back(std::move(h));
        ranges.emplace_back(r0, r1);
        r0 = r1;
    }
    merge_chunks(chunks, n_regions, R, packed);
    if (packed && (rc = pack_result(c, bam, ranges, R, &res->upload_ms)) != NW_OK) return bail(rc);
    res->n_hits = (int64_t)R->h.reg.size();
    res->n_bytes = R->h.toff.back();
    return NW_OK;
}

int nwr_discover(nwr_ctx* c, const nwr_bam* bam, int32_t flags, int64_t min_reads, nwr_result* res) {
    if (!c) return NW_E_INVALID;
    if (!bam || !res) return fail(c, NW_E_INVALID, "null argument");
    std::memset(res, 0, sizeof *res);
    if (flags & ~(NWR_EQX_AS_MATCH | NWR_PACKED)) return fail(c, NW_E_INVALID, "unknown flags %d", (int)flags);
    const bool packed = (flags & NWR_PACKED) != 0;
    const int64_t n = (int64_t)bam->off.size() - 1;
    if (n > ((int64_t)1 << 30))
        return fail(c, NW_E_UNSUPPORTED, "%lld records: at most 2^30 in one nwr_discover call", (long long)n);
    nwr::Result* R = new nwr::Result();
    R->discovered = true;
    R->region_off.assign(1, 0);
    res->handle = R;
    if (packed) {
        R->packed = true;
        R->device = c->device;
        R->gexc.assign(1, 0);
    }
    if (n <= 0) return NW_OK;
    if (hipSetDevice(c->device) != hipSuccess) {
        delete R;
        res->handle = nullptr;
        return fail(c, NW_E_HIP, "hipSetDevice failed");
    }

    std::vector<nwr::Hits> chunks;
    std::vector<std::pair<int64_t, int64_t>> ranges;
    int64_t n_regions = 0;
    int rc = [&]() -> int {
        hipStream_t st = c->stream;
        // the table: a power of two of at least twice the records, so the load stays <= 1/2
        const grp::TableGeometry tg = grp::table_geometry(n, c->hash_bits);
        const size_t slots = tg.slots;
        HIP_TRY(c, c->d_w0.reserve(slots));
        HIP_TRY(c, c->d_w1.reserve(slots));
        HIP_TRY(c, c->d_tcount.reserve(slots));
        HIP_TRY(c, c->d_slot.reserve((size_t)n));
        HIP_TRY(c, c->d_ctr.reserve(nwr::kCounters));
        HIP_TRY(c, hipMemsetAsync(c->d_w0.p, 0, sizeof(unsigned long long) * slots, st));
        HIP_TRY(c, hipMemsetAsync(c->d_w1.p, 0, sizeof(unsigned long long) * slots, st));
        HIP_TRY(c, hipMemsetAsync(c->d_tcount.p, 0, sizeof(uint32_t) * slots, st));
        HIP_TRY(c, hipMemsetAsync(c->d_ctr.p, 0, sizeof(unsigned long long) * nwr::kCounters, st));
        nwr::Table t{};
        t.w0 = c->d_w0.p;
        t.w1 = c->d_w1.p;
        t.count = c->d_tcount.p;
        t.cap_mask = tg.cap_mask;
        t.shift = tg.shift;
        t.hash_mask = tg.hash_mask;

        for (int64_t r0 = 0; r0 < n; r0 = ranges.back().second) ranges.emplace_back(r0, chunk_end(c, bam, r0, n));
        for (const auto& r : ranges) {
            const int rc1 = span_chunk(c, bam, r.first, r.second, flags, t, &res->kernel_ms, &res->upload_ms);
            if (rc1 != NW_OK) return rc1;
        }
        unsigned long long ctr[nwr::kCounters];
        HIP_TRY(c, hipMemcpy(ctr, c->d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost));
        if (ctr[nwr::kError])
            return fail(c, NW_E_STATE, "the span table's probe bound was reached (%zu slots, %lld records)", slots, (long long)n);
        const int64_t nd = (int64_t)ctr[nwr::kDistinct];
        if (nd < 0 || nd > n || (int64_t)ctr[nwr::kKept] > n) return fail(c, NW_E_STATE, "inconsistent counters");
        res->n_no_seq = (int64_t)ctr[nwr::kDropped];
        R->stats[0] = (int64_t)ctr[nwr::kAligned];
        R->stats[1] = (int64_t)ctr[nwr::kKept];
        if (nd == 0) return NW_OK;

        // the used slots to the host; the regions in key order
        std::vector<nwr::Listed> list((size_t)nd);
        HIP_TRY(c, c->d_list.reserve((size_t)nd));
        HIP_TRY(c, hipEventRecord(c->ev[0], st));
        hipLaunchKernelGGL(nwr::nwr_compact_kernel, dim3((unsigned)((slots + nwr::kBlk - 1) / nwr::kBlk)), dim3(nwr::kBlk), 0, st, t,
                           c->d_list.p, (uint64_t)nd, c->d_ctr.p);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->ev[1], st));
        HIP_TRY(c, hipMemcpyAsync(list.data(), c->d_list.p, sizeof(nwr::Listed) * (size_t)nd, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(ctr, c->d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        float ms = 0.0f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        res->kernel_ms += ms;
        if ((int64_t)ctr[nwr::kListed] != nd) return fail(c, NW_E_STATE, "inconsistent table");
        std::vector<nwr_region> key((size_t)nd);
        int64_t sum = 0;
        for (int64_t e = 0; e < nd; ++e) {
            nwr::unpack_key(list[(size_t)e].w0, list[(size_t)e].w1, &key[(size_t)e]);
            sum += list[(size_t)e].count;
            if ((uint64_t)list[(size_t)e].slot > t.cap_mask) return fail(c, NW_E_STATE, "inconsistent table");
        }
        if (sum != R->stats[1]) return fail(c, NW_E_STATE, "inconsistent table");
        std::vector<int64_t> order((size_t)nd);
        std::iota(order.begin(), order.end(), 0);
        std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {      // (the keys are distinct)
            const nwr_region &p = key[(size_t)x], &q = key[(size_t)y];
            if (p.ref_id != q.ref_id) return p.ref_id < q.ref_id;
            if (p.bpstart != q.bpstart) return p.bpstart < q.bpstart;
            return p.bpend < q.bpend;
        });
        if (nd > 0x7FFFFFFF) return fail(c, NW_E_UNSUPPORTED, "%lld regions", (long long)nd);
        n_regions = nd;
        R->regions.resize((size_t)nd);
        R->n_records.resize((size_t)nd);
        std::vector<uint32_t> lslot((size_t)nd);
        std::vector<int32_t> lreg((size_t)nd);
        int64_t emitted = 0;
        for (int64_t g = 0; g < nd; ++g) {
            const size_t e = (size_t)order[(size_t)g];
            R->regions[(size_t)g] = key[e];
            R->n_records[(size_t)g] = list[e].count;
            lslot[(size_t)g] = list[e].slot;
            const bool emit = (int64_t)list[e].count >= min_reads;
            lreg[(size_t)g] = emit ? (int32_t)g : -1;
            emitted += emit;
        }
        R->stats[2] = emitted;
        if (emitted > NWR_MAX_REGIONS)
            return fail(c, NW_E_UNSUPPORTED, "%lld regions to emit: at most %d are supported (raise min_reads)",
                        (long long)emitted, NWR_MAX_REGIONS);
        if (emitted == 0) return NW_OK;
        HIP_TRY(c, c->d_lslot.reserve((size_t)nd));
        HIP_TRY(c, c->d_lreg.reserve((size_t)nd));
        HIP_TRY(c, c->d_map.reserve(slots));
        HIP_TRY(c, hipMemcpyAsync(c->d_lslot.p, lslot.data(), sizeof(uint32_t) * (size_t)nd, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(c->d_lreg.p, lreg.data(), sizeof(int32_t) * (size_t)nd, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipEventRecord(c->ev[0], st));
        hipLaunchKernelGGL(nwr::nwr_scatter_kernel, dim3((unsigned)((nd + nwr::kBlk - 1) / nwr::kBlk)), dim3(nwr::kBlk), 0, st,
                           c->d_lslot.p, c->d_lreg.p, nd, t.cap_mask, c->d_map.p);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->ev[1], st));
        HIP_TRY(c, hipStreamSynchronize(st));
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        res->kernel_ms += ms;

        // pass 2: a one-chunk call still has its records in d_data
        std::vector<int64_t> cursor((size_t)nd + 1);
        for (const auto& r : ranges) {
            nwr::Hits h;
            const int rc2 = emit_chunk(c, bam, r.first, r.second, flags, ranges.size() == 1, nd, &cursor, &h, &res->kernel_ms,
                                       &res->upload_ms);
            if (rc2 != NW_OK) return rc2;
            if (!h.reg.empty()) chunks.push_back(std::move(h));
        }
        return NW_OK;
    }();
    if (rc == NW_OK) {
        merge_chunks(chunks, n_regions, R, packed);
        if (packed) rc = pack_result(c, bam, ranges, R, &res->upload_ms);
    }
    if (rc != NW_OK) {
        delete R;
        res->handle = nullptr;
        return rc;
    }
    res->n_regions = n_regions;
    res->n_hits = (int64_t)R->h.reg.size();
    res->n_bytes = R->h.toff.back();
    return NW_OK;
}

int nwr_fetch_regions(const nwr_result* res, nwr_region* regions, int64_t* n_records, int64_t stats[4]) {
    if (!res || !res->handle) return NW_E_INVALID;
    const nwr::Result* R = (const nwr::Result*)res->handle;
    if (!R->discovered) return NW_E_STATE;
    const size_t nr = R->regions.size();
    if (regions && nr) std::memcpy(regions, R->regions.data(), sizeof(nwr_region) * nr);
    if (n_records && nr) std::memcpy(n_records, R->n_records.data(), sizeof(int64_t) * nr);
    if (stats) std::memcpy(stats, R->stats, sizeof R->stats);
    return NW_OK;
}

int nwr_fetch(const nwr_result* res, int64_t* region_offsets, int64_t* src, int32_t* st, int32_t* en,
              int64_t* text_offsets, uint8_t* text, uint8_t* quals) {
    if (!res || !res->handle) return NW_E_INVALID;
    const nwr::Result* R = (const nwr::Result*)res->handle;
    const nwr::Hits& h = R->h;
    const size_t nh = h.reg.size(), nb = (size_t)h.toff.back();
    if (R->packed && (text || quals)) return NW_E_STATE;      // (a packed result holds neither)
    if (region_offsets) std::memcpy(region_offsets, R->region_off.data(), sizeof(int64_t) * R->region_off.size());
    if (src && nh) std::memcpy(src, h.src.data(), sizeof(int64_t) * nh);
    if (st && nh) std::memcpy(st, h.st.data(), sizeof(int32_t) * nh);
    if (en && nh) std::memcpy(en, h.en.data(), sizeof(int32_t) * nh);
    if (text_offsets) std::memcpy(text_offsets, h.toff.data(), sizeof(int64_t) * (nh + 1));
    if (text && nb) std::memcpy(text, h.text.data(), nb);
    if (quals && nb) std::memcpy(quals, h.quals.data(), nb);
    return NW_OK;
}

int nwr_packed_info(const nwr_result* res, uint16_t* lens, int64_t* region_exc, int64_t* n_exc, float* kernel_ms) {
    if (!res || !res->handle) return NW_E_INVALID;
    const nwr::Result* R = (const nwr::Result*)res->handle;
    if (!R->packed) return NW_E_STATE;
    if (lens && !R->lens16.empty()) std::memcpy(lens, R->lens16.data(), sizeof(uint16_t) * R->lens16.size());
    if (region_exc) std::memcpy(region_exc, R->gexc.data(), sizeof(int64_t) * R->gexc.size());
    if (n_exc) *n_exc = R->n_exc;
    if (kernel_ms) *kernel_ms = R->pack_ms;
    return NW_OK;
}

int nwr_fetch_packed(const nwr_result* res, uint8_t* packed, int64_t cap, int64_t* exc_pos, uint8_t* exc_byte, int64_t* needed) {
    if (!res || !res->handle) return NW_E_INVALID;
    const nwr::Result* R = (const nwr::Result*)res->handle;
    if (!R->packed) return NW_E_STATE;
    const int64_t nbytes = (R->h.toff.back() + 3) / 4, ne = R->n_exc;
    if (needed) *needed = nbytes;
    if (cap < nbytes) return NW_E_CAPACITY;
    if (nbytes == 0) return NW_OK;
    if (hipSetDevice(R->device) != hipSuccess) return NW_E_HIP;
    // (the packer has finished: nwr_extract and nwr_discover are synchronous)
    if (packed && hipMemcpy(packed, R->d_words.p, (size_t)nbytes, hipMemcpyDeviceToHost) != hipSuccess) return NW_E_HIP;
    if (exc_pos && ne > 0 && hipMemcpy(exc_pos, R->d_exc_pos.p, sizeof(int64_t) * (size_t)ne, hipMemcpyDeviceToHost) != hipSuccess)
        return NW_E_HIP;
    if (exc_byte && ne > 0 && hipMemcpy(exc_byte, R->d_exc_byte.p, (size_t)ne, hipMemcpyDeviceToHost) != hipSuccess)
        return NW_E_HIP;
    return NW_OK;
}

int nwr_adopt_region(const nwr_result* res, nw_ctx* ctx, int64_t g) {
    if (!res || !res->handle || !ctx) return NW_E_INVALID;
    nwr::Result* R = (nwr::Result*)res->handle;
    if (!R->packed) return NW_E_STATE;
    const int64_t n_regions = (int64_t)R->region_off.size() - 1;
    if (g < 0 || g >= n_regions) return NW_E_INVALID;
    const int64_t j0 = R->region_off[(size_t)g], m = R->region_off[(size_t)g + 1] - j0;
    if (m <= 0) return NW_E_INVALID;      // (a region without hits has nothing to adopt)
    int rc = nw_front::check_state(ctx);
    if (rc != NW_OK) return rc;
    if (nw_front::device_of(ctx) != R->device) return NW_E_INVALID;
    if (hipSetDevice(R->device) != hipSuccess) return NW_E_HIP;
    // every kLenGroup-th offset counted from the region's own first read
    const int64_t ngroups = m / nw::kLenGroup + 1;
    std::vector<int64_t> gb((size_t)ngroups);
    for (int64_t q = 0; q < ngroups; ++q) gb[(size_t)q] = R->h.toff[(size_t)(j0 + q * nw::kLenGroup)];
    if (R->d_gbase.reserve((size_t)ngroups) != hipSuccess) return NW_E_NOMEM;
    if (hipMemcpy(R->d_gbase.p, gb.data(), sizeof(int64_t) * (size_t)ngroups, hipMemcpyHostToDevice) != hipSuccess) return NW_E_HIP;
    const int64_t e0 = R->gexc[(size_t)g], ne = R->gexc[(size_t)g + 1] - e0;
    // the whole call's stream and the region's slice of the exceptions, both in the call's
    // coordinates: set_packed_batch copies bytes offsets[0] / 4 .. (offsets[m] + 3) / 4 of it
    const nw_front::PackedSrc src{(const uint8_t*)R->d_words.p,
                                  R->d_lens16.p + j0,
                                  R->d_gbase.p,
                                  ne > 0 ? R->d_exc_pos.p + e0 : nullptr,
                                  ne > 0 ? R->d_exc_byte.p + e0 : nullptr,
                                  true,
                                  R->ready};
    return nw_front::set_packed_batch(ctx, src, R->h.toff.data() + j0, R->lens16.data() + j0, m, ne);
}

void nwr_release(nwr_result* res) {
    if (!res) return;
    delete (nwr::Result*)res->handle;
    res->handle = nullptr;
}

}  // extern "C"
