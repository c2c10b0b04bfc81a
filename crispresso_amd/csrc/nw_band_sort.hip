// nw_band_sort.hip -- the band path's lists: nw_band_segsort (the reads that need the DP, sorted
// by length: the first level's list, the seeded and the wide-first lists) and nw_band_redo_compact
// (the positions a level flagged, in order: the next level's list).  nw_band_device.h: the band.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "nw_band_device.h"

namespace nw {

// ============================================================================
// Length sort, one launch: segments of kSegReads reads, each sorted by key in LDS
// (stable: read order within a key), the reads that need the DP (every key but the
// exact-copy key) placed at the segment's base in the DP list -- an exclusive prefix of
// the segments' DP counts found by look-back (nw_common.h lookback_excl).  Pairs are
// consecutive DP-list positions: reads of one length within a segment (most of a
// CRISPResso segment shares the amplicon's length), so a pair's band holds both reads.
// Replaces a global counting sort (per-block histograms, two scans, scatter: four
// launches of ~8 us each per chunk).  The last segment writes the DP count (*band_count).
// ============================================================================
constexpr int kSegReads = 4096, kSegThreads = 1024, kSegWaves = kSegThreads / 64;

__host__ __device__ inline int segsort_lds_bytes(int lb_cap) { return 4 * (kSegWaves + 1) * (lb_cap + 3) + 4 * 32; }

__global__ __launch_bounds__(kSegThreads) void nw_band_segsort(const KernelArgs a, unsigned epoch) {
    extern __shared__ int seg_sm[];
    // keys: lengths 0 .. cap, cap + 1 (too long for the band), EX = cap + 2 (exact copy, no DP),
    // then the seeded reads' diagonal keys
    // ... and the wide-first reads' length keys
    const int NB = a.band_lb_cap + 3 + a.seed_keys + a.wf_keys, EX = a.band_lb_cap + 2;
    int* cnt = seg_sm;                  // [kSegWaves][NB]: per-wave counts, then prefix over waves
    int* kbase = seg_sm + kSegWaves * NB;   // [NB]: bucket totals, then their exclusive prefix
    int* misc = kbase + NB;             // [0], [4] look-back results (band list, seeded list), [2] error, [16..31] wave sums
    const int KW = a.wf_list ? a.band_lb_cap + 3 + a.seed_keys : NB;   // keys >= KW: wide-first reads (their own list)
    const int KS = a.seed_list ? a.band_lb_cap + 3 : KW;   // keys in [KS, KW): seeded reads (their own list)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < kSegWaves * NB + NB; k += kSegThreads) seg_sm[k] = 0;
    if (tid < 32) misc[tid] = 0;
    __syncthreads();
    const long long r0 = (long long)blockIdx.x * kSegReads + 4 * tid;
    int key[4], rank[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long r = r0 + i;
        const int k = r < a.n ? a.sort_key[r] : EX;
        // lanes with the same key this round (11 key bits cover NB <= 2048)
        unsigned long long m = ~0ull;
#pragma unroll
        for (int bit = 0; bit < 11; ++bit) {
            const unsigned long long bb = __ballot((k >> bit) & 1);
            m &= ((k >> bit) & 1) ? bb : ~bb;
        }
        const unsigned long long below = m & ((1ull << lane) - 1ull);
        const int old = cnt[wave * NB + k];
        __builtin_amdgcn_wave_barrier();
        if (below == 0ull) cnt[wave * NB + k] = old + (int)__builtin_popcountll(m);
        lds_fence();
        key[i] = k;
        rank[i] = old + (int)__builtin_popcountll(below);
    }
    __syncthreads();
    // per key: prefix over the waves (in place) and the key's total
    for (int k = tid; k < NB; k += kSegThreads) {
        int run = 0;
        for (int w = 0; w < kSegWaves; ++w) {
            const int v = cnt[w * NB + k];
            cnt[w * NB + k] = run;
            run += v;
        }
        kbase[k] = k == EX ? 0 : run;
    }
    __syncthreads();
    // exclusive prefix of the key totals (thread t: keys [t * per, (t + 1) * per))
    const int per = (NB + kSegThreads - 1) / kSegThreads;
    const int k0 = tid * per, k1 = min(NB, k0 + per);
    int mine = 0;
    for (int k = k0; k < k1; ++k) mine += kbase[k];
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    if (lane == 63) misc[16 + wave] = incl;
    __syncthreads();
    int before = 0, dp = 0;
#pragma unroll
    for (int w = 0; w < kSegWaves; ++w) {
        before += w < wave ? misc[16 + w] : 0;
        dp += misc[16 + w];
    }
    int run = before + incl - mine;
    for (int k = k0; k < k1; ++k) {
        const int v = kbase[k];
        kbase[k] = run;
        run += v;
    }
    __syncthreads();
    // the seeded keys are the tail of the key range: their prefix past the band list's total is
    // their place in the seeded list
    // the seeded list: an odd segment count gets its last entry twice (a pair of one read: the walks take
    // its first position), so every pair of that list lies within one segment's sorted run
    const int dpK = KW < NB ? kbase[KW] : dp, dpW = dp - dpK;   // (the wide-first list: no padding, the wide band holds any pair)
    const int dpB = KS < NB ? kbase[KS] : dp, dpS0 = dpK - dpB, dpS = dpS0 + (dpS0 & 1);
    if (wave == 0) {
        const unsigned base = lookback_excl(a.lb_status, blockIdx.x, epoch, (unsigned)dpB, &misc[2]);
        if (lane == 0) misc[0] = (int)base;
    } else if (wave == 1 && a.seed_list) {   // the seeded list: the look-back words after the band list's
        const unsigned base = lookback_excl(a.lb_status + gridDim.x + 1, blockIdx.x, epoch, (unsigned)dpS, &misc[2]);
        if (lane == 0) misc[4] = (int)base;
    } else if (wave == 2 && a.wf_list) {   // the wide-first list: the third set of look-back words
        const unsigned base = lookback_excl(a.lb_status + 2 * (gridDim.x + 1), blockIdx.x, epoch, (unsigned)dpW, &misc[2]);
        if (lane == 0) misc[5] = (int)base;
    }
    __syncthreads();
    const long long base = misc[0], baseS = misc[4], baseW = misc[5];
    int32_t* order = const_cast<int32_t*>(a.band_order);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = key[i];
        if (k >= KW) {
            a.wf_list[baseW + (kbase[k] - dpK) + cnt[wave * NB + k] + rank[i]] = (int32_t)(r0 + i);
        } else if (k >= KS) {
            const int q = (kbase[k] - dpB) + cnt[wave * NB + k] + rank[i];
            a.seed_list[baseS + q] = (int32_t)(r0 + i);
            if (q == dpS0 - 1 && dpS != dpS0) {   // the segment's odd count padded to a pair
                a.seed_list[baseS + q + 1] = (int32_t)(r0 + i);
                atomicAdd(a.fallback_count + kCntSeedPad, 1);   // the path counters leave the padding out
            }
        }
        else if (k != EX) order[base + kbase[k] + cnt[wave * NB + k] + rank[i]] = (int32_t)(r0 + i);
    }
    if (tid == 0) {
        if (misc[2]) a.fallback_count[kCntLookback] = 1;   // look-back cut off: the call reports an error
        if (blockIdx.x == gridDim.x - 1) {
            // (the wide-first reads are DP reads of the chunk: counted here, listed apart)
            *const_cast<int32_t*>(a.band_count) = (int32_t)(base + dpB + baseW + dpW);
            if (a.wf_list) *a.wf_count = (int32_t)(baseW + dpW);
            if (a.seed_list) *a.seed_count = (int32_t)(baseS + dpS);
        }
    }
}

// ============================================================================
// Redo list of the second level: the sorted positions the first level flagged,
// compacted in sorted order (block sums, one scan block, scatter): no atomics,
// deterministic, and consecutive entries (the second level's pairs) have similar
// lengths.  Positions [0, *band_count) are the first level's.
// ============================================================================
constexpr int kRedoBlock = 1024;   // positions per block (256 threads x 4)

__device__ int block_excl_scan_i32(int v, int* total) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        before += w < wave ? wsum[w] : 0;
        all += wsum[w];
    }
    __syncthreads();
    *total = all;
    return before + incl - v;
}

// One launch: flags of block b's 1024 positions, its exclusive prefix by look-back,
// scatter; the last block writes the count (*redo_count).  pairs: positions 2q, 2q + 1 are kept
// together when either is flagged (the seeded list's pairs stay pairs).
__global__ __launch_bounds__(256) void nw_band_redo_compact(const KernelArgs a, unsigned epoch, int pairs) {
    __shared__ int sh[2];
    if (a.tail_prio) __builtin_amdgcn_s_setprio(3);
    const long long nb = *a.band_count;
    const long long n = band_list_count(a);
    const long long k0 = (long long)blockIdx.x * kRedoBlock + threadIdx.x * 4;
    int f[4], s = 0;
    const bool all = l1_skipped(a);   // the first level was skipped: every position goes on
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        f[t] = k0 + t < n ? (all ? 1 : a.redo_flags[k0 + t]) : 0;
    }
    if (pairs) {   // (k0 is even: positions k0 .. k0 + 3 are two whole pairs)
        f[0] = f[1] = f[0] | f[1];
        f[2] = f[3] = f[2] | f[3];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        f[t] = f[t] && k0 + t < n;
        s += f[t];
    }
    if (threadIdx.x == 0) sh[1] = 0;
    int total;
    const int local = block_excl_scan_i32(s, &total);
    if (threadIdx.x < 64) {
        const unsigned e = lookback_excl(a.lb_status, blockIdx.x, epoch, (unsigned)total, &sh[1]);
        if (threadIdx.x == 0) sh[0] = (int)e;
    }
    __syncthreads();
    long long pos = sh[0] + local;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (f[t]) a.redo_list[pos++] = (int32_t)band_list_read(a, k0 + t, nb);
    if (threadIdx.x == 0) {
        if (sh[1]) a.fallback_count[kCntLookback] = 1;
        if (blockIdx.x == gridDim.x - 1) *a.redo_count = (int32_t)(sh[0] + total);
    }
}

hipError_t launch_redo_compact(const KernelArgs& a, int64_t nmax, unsigned epoch, hipStream_t s, bool pairs) {
    const int nblk = (int)std::max<int64_t>(1, (nmax + kRedoBlock - 1) / kRedoBlock);
    hipLaunchKernelGGL(nw_band_redo_compact, dim3(nblk), dim3(256), 0, s, a, epoch, pairs ? 1 : 0);
    return hipGetLastError();
}

// classify (exact copies, sort keys) then the segment sort; a.band_count receives the
// DP count, a.lb_status holds ceil(n / kSegReads) look-back words
hipError_t launch_band_sort(const KernelArgs& a, unsigned epoch, hipStream_t s) {
    launch_band_classify(a, s);
    const int nseg = (int)std::max<int64_t>(1, (a.n + kSegReads - 1) / kSegReads);
    hipLaunchKernelGGL(nw_band_segsort, dim3(nseg), dim3(kSegThreads), (size_t)segsort_lds_bytes(a.band_lb_cap + a.seed_keys + a.wf_keys), s, a,
                       epoch);
    return hipGetLastError();
}
// words of the single-pass scans over n reads: the largest of the segment sort's two lists
// (the seeded list after the band list's ceil(n / kSegReads) + 1 words), the redo and ops
// compactions (1024-read blocks)
int64_t band_lookback_words(int64_t n) {
    const int64_t seg = std::max<int64_t>(1, (n + kSegReads - 1) / kSegReads);
    return std::max<int64_t>(std::max<int64_t>(1, (n + 1023) / 1024) + 1, 3 * seg + 3);   // band, seeded, wide-first list
}

}  // namespace nw
