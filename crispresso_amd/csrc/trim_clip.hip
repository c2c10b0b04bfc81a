// Adapter clipping on gfx950 with Trimmomatic 0.33 ILLUMINACLIP + MINLEN semantics
// (include/crispr_trim.h).
//
// Replaces the Trimmomatic process CRISPResso runs before the merge
// (CRISPResso/CRISPRessoCORE.py:1620-1640); the algorithm is the one
// oracle/trimmomatic_oracle.py restates (IlluminaClip.process, ClipSeq, PrefixPair,
// maximum_range, _cut, run_pe's MINLEN).
//
// One wavefront per read pair; the adapter tables (a few KB) are copied to LDS once per
// block.  prefix1 + read 1 and prefix2 + read 2 are staged in
// LDS as bytes, qualities (prefix bases 100) and one-hot nibbles packed 8 to a dword,
// zero-padded, so the 16-mer at any position is three dword reads and a shift.
//   * Palindrome mode: lane l tests the seed of overlap step skip + l, + 64, ...
//     (ref / test of the restatement's alternating walk in closed form); a ballot gives
//     the hit steps in increasing order; each hit's overlap is scored: the lanes
//     classify the bases into fp32 terms in LDS, the sum is formed left to right.
//   * Simple mode: lane l holds the read 16-mer at position l, l + 64, ... and meets
//     every adapter 16-mer j (adapter positions 0, 4, 8, ...) with it; a ballot gives the
//     seeds, offset = position - 4j; each is scored the same way, the terms reduced by
//     the restatement's maximum_range on one lane (sequential by definition).  The keep
//     length is the smallest passing offset over all adapters, so the order of the seeds
//     does not matter, and an offset at or past the keep length found so far is skipped.
// The fp32 sums are formed in the restatement's order (no reassociation, no fma: the
// terms are only added).  Integer / LDS work, tens of bytes per pair: VALU / LDS bound.
//
// The host side of both entries is below the kernel: nwt_trim_batch (this kernel alone) and
// nwt_trim_program (this kernel, then the steps kernel of trim_steps.hip on the same buffers)
// share the table building, the validation, the upload and the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "trim_device.h"

namespace nwt {

constexpr int kMaxPacks = 32;   // adapter 16-mers at 0, 4, 8, ...: (128 - 15 + 3) / 4 = 29
constexpr int kPrefixQual = 100;

struct alignas(16) Tables {
    int32_t n_adapters, n_pp;
    int32_t alen[NWT_MAX_ADAPTERS], arole[NWT_MAX_ADAPTERS], ank[NWT_MAX_ADAPTERS];
    int32_t plen[NWT_MAX_PREFIX_PAIRS];
    uint64_t apack[NWT_MAX_ADAPTERS][kMaxPacks];
    uint8_t aseq[NWT_MAX_ADAPTERS][NWT_MAX_ADAPTER];
    uint8_t p1[NWT_MAX_PREFIX_PAIRS][NWT_MAX_ADAPTER], p2[NWT_MAX_PREFIX_PAIRS][NWT_MAX_ADAPTER];
    float mism[128];   // float32(-q / 10.0), the division in double
};

// Program::tables holds one Tables, aligned within the bytes
inline Tables* host_tables(Program& P) {
    const uintptr_t a = (uintptr_t)P.tables.data();
    return (Tables*)((a + alignof(Tables) - 1) & ~(uintptr_t)(alignof(Tables) - 1));
}

struct Args {
    const uint8_t* seq1;
    const uint8_t* qual1;
    const int64_t* off1;
    const uint8_t* seq2;
    const uint8_t* qual2;
    const int64_t* off2;
    int64_t n;
    int32_t* keep1;
    int32_t* keep2;
    const Tables* t;
    int32_t seed_max, min_ov, min_prefix, keep_both, minlen, paired;
    float pal_thr, simple_thr, log10_4;
    int32_t lb;   // LDS bytes per staged prefix + read (16-B multiple, >= longest + 16)
    int32_t lw;   // dwords per nibble array (even, >= lb / 8 + 4)
    int32_t wpb;  // waves per block
};

__host__ __device__ __forceinline__ unsigned nib(uint8_t c) {
    return c == 'A' ? 1u : c == 'T' ? 2u : c == 'C' ? 4u : c == 'G' ? 8u : 0u;
}
__device__ __forceinline__ uint8_t comp(uint8_t c) {
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}
// 16 nibbles from position pos (first in the top nibble) of an array packed 8 to a dword
__device__ __forceinline__ uint64_t fwd16(const uint32_t* w, int pos) {
    const int k = pos >> 3, s = (pos & 7) * 4;
    const uint64_t top = ((uint64_t)w[k] << 32) | w[k + 1];
    return s ? (top << s) | (uint64_t)(w[k + 2] >> (32 - s)) : top;
}
// the 16-mer's reverse complement: nibble order reversed, A <-> T and C <-> G
__device__ __forceinline__ uint64_t rc16(uint64_t w) {
    w = __builtin_bswap64(w);
    w = ((w & 0x0f0f0f0f0f0f0f0full) << 4) | ((w >> 4) & 0x0f0f0f0f0f0f0f0full);
    return ((w & 0x5555555555555555ull) << 1) | ((w >> 1) & 0x5555555555555555ull);
}
__device__ __forceinline__ void wsync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// maximum_range of the restatement over v[0 .. n), n >= 1 (one lane; v is overwritten)
__device__ float maximum_range(float* v, int n) {
    float total = 0.0f;
    int m = 0;
    for (int t = 0; t < n; ++t) {
        const float x = v[t];
        if ((total > 0.0f && x < 0.0f) || (total < 0.0f && x > 0.0f)) {
            v[m++] = total;   // m <= t
            total = x;
        } else {
            total = total + x;
        }
    }
    v[m++] = total;
    bool again = true;
    while (again) {
        again = false;
        if (m < 3) break;
        int w = 1, r = 1;   // v[0 .. w) is the list so far, v[r .. m) still to visit
        while (r < m) {
            const float x = v[r];
            if (r < m - 1 && x < 0.0f && v[w - 1] > -x && v[r + 1] > -x) {
                v[w - 1] = (v[w - 1] + x) + v[r + 1];
                r += 2;
                again = true;
            } else {
                v[w++] = x;
                ++r;
            }
        }
        m = w;
    }
    float best = 0.0f;
    for (int t = 0; t < m; ++t)
        if (v[t] > best) best = v[t];
    return best;
}

__global__ __launch_bounds__(64 * kWpb) void nwt_clip_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the adapter tables, copied to LDS once per block (every later read of them is an LDS read)
    for (unsigned k = threadIdx.x; k < sizeof(Tables) / 4; k += blockDim.x)
        ((uint32_t*)smem)[k] = ((const uint32_t*)a.t)[k];
    __syncthreads();
    const Tables& T = *(const Tables*)smem;
    unsigned char* base = smem + sizeof(Tables) + (size_t)wave * ((size_t)8 * a.lb + (size_t)8 * a.lw);
    float* vals = (float*)base;                      // lb floats: the terms of one score
    uint32_t* na = (uint32_t*)(base + 4 * a.lb);     // nibbles of prefix1 + read 1
    uint32_t* nb = na + a.lw;                        // nibbles of prefix2 + read 2
    unsigned char* sa = (unsigned char*)(nb + a.lw); // prefix1 + read 1
    unsigned char* qa = sa + a.lb;                   // qualities (prefix 100)
    unsigned char* sb = qa + a.lb;                   // prefix2 + read 2
    unsigned char* qb = sb + a.lb;
    for (int64_t p = (int64_t)blockIdx.x * a.wpb + wave; p < a.n; p += (int64_t)gridDim.x * a.wpb) {
        const int64_t o1 = a.off1[p];
        const int n1 = (int)(a.off1[p + 1] - o1);
        const int64_t o2 = a.paired ? a.off2[p] : 0;
        const int n2 = a.paired ? (int)(a.off2[p + 1] - o2) : 0;
        int keep1 = INT_MAX, keep2 = INT_MAX;
        // table entries come out of LDS into vector registers: tell the compiler they are uniform
        const int n_pp = __builtin_amdgcn_readfirstlane(T.n_pp);
        const int n_adapters = __builtin_amdgcn_readfirstlane(T.n_adapters);
        const int rounds = n_pp > 0 ? n_pp : 1;
        int pl = 0;
        for (int pp = 0; pp < rounds; ++pp) {
            pl = n_pp > 0 ? __builtin_amdgcn_readfirstlane(T.plen[pp]) : 0;
            const int len1 = pl + n1, len2 = pl + n2;
            wsync();   // the previous round's readers are done
            for (int k = lane; k < pl; k += 64) {
                sa[k] = T.p1[pp][k];
                sb[k] = T.p2[pp][k];
                qa[k] = qb[k] = (uint8_t)kPrefixQual;
            }
            for (int k = lane; k < n1; k += 64) {
                sa[pl + k] = a.seq1[o1 + k];
                qa[pl + k] = (uint8_t)(a.qual1[o1 + k] - 33);
            }
            for (int k = lane; k < n2; k += 64) {
                sb[pl + k] = a.seq2[o2 + k];
                qb[pl + k] = (uint8_t)(a.qual2[o2 + k] - 33);
            }
            wsync();
            for (int k = lane; k < a.lw; k += 64) {
                uint32_t wa = 0, wb = 0;
                for (int t = 0; t < 8; ++t) {
                    const int pos = 8 * k + t;
                    wa = (wa << 4) | (pos < len1 ? nib(sa[pos]) : 0u);
                    wb = (wb << 4) | (pos < len2 ? nib(sb[pos]) : 0u);
                }
                na[k] = wa;
                nb[k] = wb;
            }
            wsync();
            if (n_pp == 0 || !a.paired || n1 < 16 || n2 < 16) continue;
            // PrefixPair.compare: ref + test = pl + count; ref advances at even counts up to cap
            const int np1 = len1 - 15, np2 = len2 - 15;
            const int skip = pl > 16 ? pl - 16 : 0;
            const int cap = min(np1, np2) - 1 - pl;
            const int max_count = max(len1, len2) - 15 - a.min_prefix;
            bool done = false;
            for (int cb = skip; cb < max_count && !done; cb += 64) {
                const int count = cb + lane;
                bool hit = false;
                if (count < max_count) {
                    const int ref = pl + min((count >> 1) - (skip >> 1), cap);
                    const int test = pl + count - ref;
                    if (test < np2)
                        hit = __builtin_popcountll(fwd16(na, ref) ^ rc16(fwd16(nb, test))) <= a.seed_max;
                    if (!hit && test < np1)
                        hit = __builtin_popcountll(rc16(fwd16(nb, ref)) ^ fwd16(na, test)) <= a.seed_max;
                }
                uint64_t hm = __ballot(hit);
                while (hm) {
                    const int cnt = cb + (int)__builtin_ctzll(hm);
                    hm &= hm - 1;
                    const int total = cnt + pl + 16;
                    const int skip1 = total > len2 ? total - len2 : 0;
                    const int skip2 = total > len1 ? total - len1 : 0;
                    const int actual = total - skip1 - skip2;
                    for (int i = lane; i < actual; i += 64) {
                        const int x1 = i + skip1, x2 = skip2 + actual - i - 1;
                        const uint8_t c1 = sa[x1], c2 = comp(sb[x2]);
                        float v = a.log10_4;
                        if (c1 == 'N' || c2 == 'N')
                            v = 0.0f;
                        else if (c1 != c2)
                            v = T.mism[min((int)qa[x1], (int)qb[x2])];
                        vals[i] = v;
                    }
                    wsync();
                    float sum = 0.0f;
                    for (int i = 0; i < actual; ++i) sum = sum + vals[i];   // left to right, every lane
                    wsync();
                    if (sum >= a.pal_thr) {
                        const int k = total - 2 * pl;
                        if (k < keep1) {
                            keep1 = k;
                            keep2 = a.keep_both ? k : 0;
                        }
                        done = true;
                        break;
                    }
                }
            }
        }
        // ClipSeq.compare over the adapters of each read; the staged arrays hold the read from pl on
        for (int sel = 1; sel <= (a.paired ? 2 : 1); ++sel) {
            const unsigned char* S = (sel == 1 ? sa : sb) + pl;
            const unsigned char* Q = (sel == 1 ? qa : qb) + pl;
            const uint32_t* N = sel == 1 ? na : nb;
            const int n = sel == 1 ? n1 : n2;
            int keep = sel == 1 ? keep1 : keep2;
            const int ilim = n - a.min_ov;   // read positions below it seed
            // The read's keep length is the smallest offset, over all adapters, whose score
            // reaches the threshold (each adapter's first passing offset in increasing order is
            // its smallest), so the seeds may be visited in any order: lane l holds the read
            // 16-mer at position ib + l once and meets every adapter 16-mer with it; a seed whose
            // offset is not below the keep length found so far cannot lower it and is skipped.
            for (int ib = 0; ib < ilim; ib += 64) {
                const int i = ib + lane;
                const bool live = i < ilim;
                uint64_t w = 0, mask = ~0ull;
                if (live) {
                    w = fwd16(N, pl + i);
                    const int rem = n - i;
                    if (rem < 16) mask = ~0ull << ((16 - rem) * 4);
                }
                for (int ad = 0; ad < n_adapters; ++ad) {
                    const int role = __builtin_amdgcn_readfirstlane(T.arole[ad]);
                    if (role != 0 && role != sel) continue;
                    const int m = __builtin_amdgcn_readfirstlane(T.alen[ad]);
                    const int nk = __builtin_amdgcn_readfirstlane(T.ank[ad]);
                    // all of the adapter's 16-mers first, without control flow (the table reads
                    // pipeline); seeds are rare, the scoring below is the slow path
                    uint32_t hits = 0;
#pragma unroll 4
                    for (int j = 0; j < nk; ++j)
                        hits |= (uint32_t)(__builtin_popcountll((w ^ T.apack[ad][j]) & mask) <= a.seed_max) << j;
                    if (!live) hits = 0;
                    if (__ballot(hits != 0) == 0) continue;
                    for (int j = 0; j < nk; ++j) {
                        uint64_t hm = __ballot(((hits >> j) & 1u) != 0 && i - 4 * j < keep);
                        while (hm) {
                            const int off = ib + (int)__builtin_ctzll(hm) - 4 * j;
                            hm &= hm - 1;
                            if (off >= keep) continue;   // keep was lowered since the ballot
                            const int rec_len = off > 0 ? n - off : n;
                            const int clip_len = off < 0 ? m + off : m;
                            const int cmp = min(rec_len, clip_len);
                            if (cmp <= a.min_ov) continue;
                            const int rp = off > 0 ? off : 0, cp = off < 0 ? -off : 0;
                            for (int t = lane; t < cmp; t += 64) {
                                const uint8_t c1 = S[rp + t], c2 = T.aseq[ad][cp + t];
                                float v = a.log10_4;
                                if (c1 == 'N' || c2 == 'N')
                                    v = 0.0f;
                                else if (c1 != c2)
                                    v = T.mism[Q[rp + t]];
                                vals[t] = v;
                            }
                            wsync();
                            float sc = 0.0f;
                            if (lane == 0) sc = maximum_range(vals, cmp);
                            sc = __shfl(sc, 0);
                            wsync();
                            if (sc >= a.simple_thr) keep = off;
                        }
                    }
                }
            }
            if (sel == 1)
                keep1 = keep;
            else
                keep2 = keep;
        }
        if (lane == 0) {
            int k1 = keep1 >= n1 ? n1 : keep1 <= 0 ? 0 : keep1;
            if (k1 < a.minlen) k1 = 0;
            a.keep1[p] = k1;
            if (a.paired) {
                int k2 = keep2 >= n2 ? n2 : keep2 <= 0 ? 0 : keep2;
                if (k2 < a.minlen) k2 = 0;
                a.keep2[p] = k2;
            }
        }
    }
}

thread_local std::string g_err;

// `who` is the entry's name: every message starts with it
int fail(const char* who, int code, const std::string& msg) {
    g_err = std::string(who) + ": " + msg;
    return code;
}

// offsets from 0, ascending, every read <= NWT_MAX_READ; the longest read's length in *lmax
int check_offsets(const char* who, const int64_t* off, int64_t n, int* lmax) {
    if (off[0] != 0) return fail(who, -1, "offsets must start at 0");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t l = off[i + 1] - off[i];
        if (l < 0) return fail(who, -1, "offsets not ascending");
        if (l > NWT_MAX_READ) return fail(who, -3, "reads longer than 4096 bases are not supported");
        *lmax = (int)std::max<int64_t>(*lmax, l);
    }
    return 0;
}

bool quals_ok(const uint8_t* q, int64_t n) {
    unsigned bad = 0;
    for (int64_t i = 0; i < n; ++i) bad |= (unsigned)(q[i] < 33) | (unsigned)(q[i] > 126);
    return bad == 0;
}

// The reads of a batch (n > 0): offsets and quality bytes; the longest read in *lmax.
int check_reads(const char* who, const uint8_t* qual1, const int64_t* off1, const uint8_t* qual2, const int64_t* off2,
                int64_t n, bool paired, int* lmax) {
    int rc = check_offsets(who, off1, n, lmax);
    if (rc == 0 && paired) rc = check_offsets(who, off2, n, lmax);
    if (rc != 0) return rc;
    if (!quals_ok(qual1, off1[n]) || (paired && !quals_ok(qual2, off2[n])))
        return fail(who, -1, "a quality byte outside 33..126 (phred 33)");
    return 0;
}

int check_counts(const char* who, const uint8_t* adapters, const int32_t* adapter_off, const int32_t* adapter_role,
                 int32_t n_adapters, const uint8_t* prefixes, const int32_t* prefix_off, int32_t n_prefix_pairs) {
    if (n_adapters < 0 || n_prefix_pairs < 0 || (n_adapters > 0 && (!adapters || !adapter_off || !adapter_role)) ||
        (n_prefix_pairs > 0 && (!prefixes || !prefix_off)))
        return fail(who, -1, "null argument or negative count");
    return 0;
}

// ILLUMINACLIP's parameters, adapters and prefix pairs into the kernel's tables; the longest
// prefix in *plmax.
int build_tables(const char* who, const nwt_params* params, const uint8_t* adapters, const int32_t* adapter_off,
                 const int32_t* adapter_role, int32_t n_adapters, const uint8_t* prefixes, const int32_t* prefix_off,
                 int32_t n_prefix_pairs, Tables& T, int* plmax) {
    if (params->seed_mismatches < 0 || params->palindrome_threshold < 0 || params->simple_threshold < 0 ||
        params->min_prefix < 0 || params->minlen < 0)
        return fail(who, -1, "negative parameter");
    if (n_adapters > NWT_MAX_ADAPTERS) return fail(who, -3, "more than 16 adapters are not supported");
    if (n_prefix_pairs > NWT_MAX_PREFIX_PAIRS) return fail(who, -3, "more than 4 prefix pairs are not supported");
    memset(&T, 0, sizeof(T));
    T.n_adapters = n_adapters;
    T.n_pp = n_prefix_pairs;
    if (n_adapters > 0 && adapter_off[0] != 0) return fail(who, -1, "adapter offsets must start at 0");
    for (int k = 0; k < n_adapters; ++k) {
        const int len = adapter_off[k + 1] - adapter_off[k];
        if (len < 0) return fail(who, -1, "adapter offsets not ascending");
        if (adapter_role[k] < 0 || adapter_role[k] > 2) return fail(who, -1, "adapter role must be 0, 1 or 2");
        if (len > NWT_MAX_ADAPTER) return fail(who, -3, "adapters longer than 128 bases are not supported");
        if (len < NWT_MIN_SIMPLE_ADAPTER)
            return fail(who, -3, "simple-mode adapters shorter than 24 bases (Trimmomatic's short and "
                                 "medium clipping classes) are not supported");
        const uint8_t* s = adapters + adapter_off[k];
        T.alen[k] = len;
        T.arole[k] = adapter_role[k];
        T.ank[k] = (len - 15 + 3) / 4;
        memcpy(T.aseq[k], s, len);
        for (int j = 0; j < T.ank[k]; ++j) {
            uint64_t w = 0;
            for (int t = 0; t < 16; ++t) w = (w << 4) | nib(s[4 * j + t]);
            T.apack[k][j] = w;
        }
    }
    *plmax = 0;
    if (n_prefix_pairs > 0 && prefix_off[0] != 0) return fail(who, -1, "prefix offsets must start at 0");
    for (int k = 0; k < n_prefix_pairs; ++k) {
        const int l1 = prefix_off[2 * k + 1] - prefix_off[2 * k], l2 = prefix_off[2 * k + 2] - prefix_off[2 * k + 1];
        if (l1 < 0 || l2 < 0) return fail(who, -1, "prefix offsets not ascending");
        if (l1 > NWT_MAX_ADAPTER || l2 > NWT_MAX_ADAPTER)
            return fail(who, -3, "prefixes longer than 128 bases are not supported");
        const int m = std::min(l1, l2);   // both cut to the shorter one's length from their 3' ends
        T.plen[k] = m;
        memcpy(T.p1[k], prefixes + prefix_off[2 * k] + (l1 - m), m);
        memcpy(T.p2[k], prefixes + prefix_off[2 * k + 1] + (l2 - m), m);
        *plmax = std::max(*plmax, m);
    }
    for (int q = 0; q < 128; ++q) T.mism[q] = (float)(-(double)q / 10.0);
    return 0;
}

// The clip kernel on an uploaded batch; keeps to d_k1 / d_k2.
bool run_clip(Batch& b, const nwt_params* params, const Tables* d_t, int lmax, int plmax, int64_t n, bool paired,
              int32_t* d_k1, int32_t* d_k2, float* ms) {
    Args a{};
    a.lb = (lmax + plmax + 16 + 15) & ~15;
    a.lw = a.lb / 8 + 4;
    const size_t lds_wave = (size_t)8 * a.lb + (size_t)8 * a.lw;
    // 1 wave: reads in the thousands of bases (<= 38 KB a wave, under 64 KB with the tables)
    a.wpb = sizeof(Tables) + lds_wave * kWpb <= 65536 ? kWpb : 1;
    const size_t lds = sizeof(Tables) + lds_wave * a.wpb;
    a.seq1 = b.s1;
    a.qual1 = b.q1;
    a.off1 = b.o1;
    a.seq2 = b.s2;
    a.qual2 = b.q2;
    a.off2 = b.o2;
    a.n = n;
    a.keep1 = d_k1;
    a.keep2 = d_k2;
    a.t = d_t;
    a.seed_max = 2 * params->seed_mismatches;
    const float log10_4 = 0.60206f;
    a.min_ov = std::min(15, (int)((double)params->simple_threshold / (double)log10_4));
    a.min_prefix = params->min_prefix;
    a.keep_both = params->keep_both != 0;
    a.minlen = params->minlen;
    a.paired = paired;
    a.pal_thr = (float)params->palindrome_threshold;
    a.simple_thr = (float)params->simple_threshold;
    a.log10_4 = log10_4;
    if (!b.begin()) return false;
    hipLaunchKernelGGL(nwt_clip_kernel, dim3(b.grid(n, a.wpb)), dim3(64 * a.wpb), lds, nullptr, a);
    return b.elapsed(ms);
}

// nwt_trim_program's checks of its program (after the null checks), the steps by value and
// ILLUMINACLIP's tables.
int program_check(const char* who, const nwt_params* clip, const uint8_t* adapters, const int32_t* adapter_off,
                  const int32_t* adapter_role, int32_t n_adapters, const uint8_t* prefixes, const int32_t* prefix_off,
                  int32_t n_prefix_pairs, const nwt_step* steps, int32_t n_steps, Program& P) {
    if (n_steps > NWT_MAX_STEPS) return fail(who, -1, "more than 16 steps are not supported");
    P.sa = StepsArgs{};
    for (int k = 0; k < n_steps; ++k) {
        const nwt_step& st = steps[k];
        if (st.op < NWT_OP_LEADING || st.op > NWT_OP_MINLEN) return fail(who, -1, "unknown step op");
        if (st.arg < 0 || st.arg > NWT_MAX_STEP_ARG) return fail(who, -1, "a step argument outside 0..2^20");
        const bool qual = st.op == NWT_OP_LEADING || st.op == NWT_OP_TRAILING || st.op == NWT_OP_AVGQUAL;
        if (qual && st.arg > NWT_MAX_STEP_QUAL) return fail(who, -1, "a quality threshold above 1000");
        if (st.op == NWT_OP_SLIDINGWINDOW &&
            (st.arg < 1 || !(st.r >= 0.0f) || !(st.r <= 3.0e38f) || !(st.R >= 0.0f) || !(st.R <= 3.0e38f)))
            return fail(who, -1, "SLIDINGWINDOW needs a window of at least 1 and a finite quality >= 0");
        P.sa.steps[k] = st;
    }
    P.sa.n_steps = n_steps;
    P.clip = clip != nullptr;
    P.plmax = 0;
    if (clip) {
        if (clip->minlen != 0) return fail(who, -1, "the clip parameters' minlen must be 0 (MINLEN is a step)");
        P.params = *clip;
        P.tables.resize(sizeof(Tables) + alignof(Tables));
        return build_tables(who, clip, adapters, adapter_off, adapter_role, n_adapters, prefixes, prefix_off,
                            n_prefix_pairs, *host_tables(P), &P.plmax);
    }
    return 0;
}

// The device arrays a program needs beside the reads, owned by b: the windows (d_out: start1,
// keep1, start2, keep2) and, with a clip, its lengths and tables.
bool program_alloc(Batch& b, Program& P, int64_t n, int32_t* d_out[4]) {
    bool have = true;
    for (int k = 0; k < 4; ++k) have = (d_out[k] = (int32_t*)b.dev(sizeof(int32_t) * n)) != nullptr && have;
    P.d_c1 = P.clip ? (int32_t*)b.dev(sizeof(int32_t) * n) : nullptr;
    P.d_c2 = P.clip ? (int32_t*)b.dev(sizeof(int32_t) * n) : nullptr;
    P.d_t = P.clip ? b.dev(sizeof(Tables)) : nullptr;
    return have && (!P.clip || (P.d_c1 && P.d_c2 && P.d_t));
}

// The clip kernel (with a clip), then the steps kernel, on the uploaded batch (null stream).
bool program_run(Batch& b, Program& P, int lmax, int64_t n, bool paired, int32_t* const d_out[4], float* kernel_ms) {
    if (P.clip &&
        !(hipMemcpy(P.d_t, host_tables(P), sizeof(Tables), hipMemcpyHostToDevice) == hipSuccess &&
          run_clip(b, &P.params, (const Tables*)P.d_t, lmax, P.plmax, n, paired, P.d_c1, P.d_c2,
                   kernel_ms ? kernel_ms + 0 : nullptr)))
        return false;
    StepsArgs& sa = P.sa;
    sa.seq[0] = b.s1, sa.qual[0] = b.q1, sa.off[0] = b.o1;
    sa.seq[1] = b.s2, sa.qual[1] = b.q2, sa.off[1] = b.o2;
    sa.keep_in[0] = P.d_c1, sa.keep_in[1] = paired ? P.d_c2 : nullptr;
    sa.start[0] = d_out[0], sa.keep[0] = d_out[1], sa.start[1] = d_out[2], sa.keep[1] = d_out[3];
    sa.n = n;
    sa.paired = paired;
    const size_t lds_wave = steps_lds_per_wave(lmax, &sa.lb);
    // 1 wave: reads in the thousands of bases (<= 21 KB a wave)
    sa.wpb = lds_wave * kWpb <= 65536 ? kWpb : 1;
    if (!b.begin()) return false;
    launch_steps(sa, b.grid(paired ? 2 * n : n, sa.wpb), lds_wave * sa.wpb);
    return b.elapsed(kernel_ms ? kernel_ms + 1 : nullptr);
}

int hip_failure(const char* who) {
    return fail(who, -4, std::string("HIP error: ") + hipGetErrorString(hipGetLastError()));
}

}  // namespace nwt

extern "C" const char* nwt_last_error(void) { return nwt::g_err.c_str(); }

extern "C" int nwt_trim_batch(int device, const nwt_params* params, const uint8_t* adapters,
                              const int32_t* adapter_off, const int32_t* adapter_role, int32_t n_adapters,
                              const uint8_t* prefixes, const int32_t* prefix_off, int32_t n_prefix_pairs,
                              const uint8_t* seq1, const uint8_t* qual1, const int64_t* off1, const uint8_t* seq2,
                              const uint8_t* qual2, const int64_t* off2, int64_t n, int32_t* keep1, int32_t* keep2,
                              float* kernel_ms) {
    using namespace nwt;
    const char* who = "nwt_trim_batch";
    const bool paired = seq2 != nullptr;
    if (!params || n < 0) return fail(who, -1, "null argument or negative count");
    int rc = check_counts(who, adapters, adapter_off, adapter_role, n_adapters, prefixes, prefix_off, n_prefix_pairs);
    if (rc != 0) return rc;
    if (n > 0 && (!seq1 || !qual1 || !off1 || !keep1 || (paired && (!qual2 || !off2 || !keep2))))
        return fail(who, -1, "null argument");
    std::vector<Tables> tv(1);
    int plmax = 0;
    rc = build_tables(who, params, adapters, adapter_off, adapter_role, n_adapters, prefixes, prefix_off,
                      n_prefix_pairs, tv[0], &plmax);
    if (rc != 0) return rc;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n == 0) return 0;
    int lmax = 0;
    rc = check_reads(who, qual1, off1, qual2, off2, n, paired, &lmax);
    if (rc != 0) return rc;

    if (hipSetDevice(device) != hipSuccess) return fail(who, -4, "hipSetDevice failed");
    Batch b;
    const bool have = b.alloc_reads(off1[n], paired ? off2[n] : 0, n);
    int32_t* d_k1 = (int32_t*)b.dev(sizeof(int32_t) * n);
    int32_t* d_k2 = (int32_t*)b.dev(sizeof(int32_t) * n);
    Tables* d_t = (Tables*)b.dev(sizeof(Tables));
    if (!have || !d_k1 || !d_k2 || !d_t) return fail(who, -4, "hipMalloc failed");
    bool ok = hipMemcpy(d_t, &tv[0], sizeof(Tables), hipMemcpyHostToDevice) == hipSuccess &&
              b.upload(device, seq1, qual1, off1, seq2, qual2, off2, n, paired) &&
              run_clip(b, params, d_t, lmax, plmax, n, paired, d_k1, d_k2, kernel_ms);
    ok = ok && hipMemcpy(keep1, d_k1, sizeof(int32_t) * n, hipMemcpyDeviceToHost) == hipSuccess &&
         (!paired || hipMemcpy(keep2, d_k2, sizeof(int32_t) * n, hipMemcpyDeviceToHost) == hipSuccess);
    if (!ok) return hip_failure(who);
    return 0;
}

extern "C" int nwt_trim_program(int device, const nwt_params* clip, const uint8_t* adapters,
                                const int32_t* adapter_off, const int32_t* adapter_role, int32_t n_adapters,
                                const uint8_t* prefixes, const int32_t* prefix_off, int32_t n_prefix_pairs,
                                const nwt_step* steps, int32_t n_steps, const uint8_t* seq1, const uint8_t* qual1,
                                const int64_t* off1, const uint8_t* seq2, const uint8_t* qual2, const int64_t* off2,
                                int64_t n, int32_t* start1, int32_t* keep1, int32_t* start2, int32_t* keep2,
                                float* kernel_ms) {
    using namespace nwt;
    const char* who = "nwt_trim_program";
    const bool paired = seq2 != nullptr;
    if (n < 0 || n_steps < 0 || (n_steps > 0 && !steps)) return fail(who, -1, "null argument or negative count");
    int rc = 0;
    if (clip) {
        rc = check_counts(who, adapters, adapter_off, adapter_role, n_adapters, prefixes, prefix_off, n_prefix_pairs);
        if (rc != 0) return rc;
    }
    if (n > 0 && (!seq1 || !qual1 || !off1 || !start1 || !keep1 || (paired && (!qual2 || !off2 || !start2 || !keep2))))
        return fail(who, -1, "null argument");
    Program P;
    rc = program_check(who, clip, adapters, adapter_off, adapter_role, n_adapters, prefixes, prefix_off,
                       n_prefix_pairs, steps, n_steps, P);
    if (rc != 0) return rc;
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.0f;
    if (n == 0) return 0;
    int lmax = 0;
    rc = check_reads(who, qual1, off1, qual2, off2, n, paired, &lmax);
    if (rc != 0) return rc;

    if (hipSetDevice(device) != hipSuccess) return fail(who, -4, "hipSetDevice failed");
    Batch b;
    const bool have = b.alloc_reads(off1[n], paired ? off2[n] : 0, n);
    int32_t* d_out[4];   // start1, keep1, start2, keep2
    if (!program_alloc(b, P, n, d_out) || !have) return fail(who, -4, "hipMalloc failed");
    bool ok = b.upload(device, seq1, qual1, off1, seq2, qual2, off2, n, paired) &&
              program_run(b, P, lmax, n, paired, d_out, kernel_ms);
    int32_t* host[4] = {start1, keep1, start2, keep2};
    for (int k = 0; ok && k < (paired ? 4 : 2); ++k)
        ok = hipMemcpy(host[k], d_out[k], sizeof(int32_t) * n, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return hip_failure(who);
    return 0;
}
