// nw_band.hip -- the band path's first stage: nw_band_classify (sort keys; the reads that need
// no DP -- exact copies, the substitution, indel and window certificates -- get their records
// here) and nw_band_cert (the deferred certificates on dense lists).  The band, its proof and
// the layout: nw_band_device.h; the later stages: nw_band_sort.hip, nw_band_fill.hip, nw_band_walk.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "nw_band_device.h"

#define NW_CAND 8            // classify: exact-copy candidates compared together

namespace nw {

namespace {

// The range [lb, ub) of each of K keys among n sorted keys (LDS): branch-free binary searches in
// lockstep, one step per power of two from top (the largest <= n; wave-uniform), so every key's two
// probes of a step are in flight together (K = 8: 16 LDS loads per round trip, not one)
template <int K>
__device__ __forceinline__ void sorted_ranges(const unsigned* skey, int n, const unsigned* key, int* lb, int* ub) {
#pragma unroll
    for (int t = 0; t < K; ++t) lb[t] = ub[t] = 0;
    for (int step = n > 0 ? 1 << (31 - __builtin_clz((unsigned)n)) : 0; step > 0; step >>= 1) {
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const int pl = lb[t] + step, pu = ub[t] + step;
            const unsigned kl = skey[min(pl, n) - 1], ku = skey[min(pu, n) - 1];
            lb[t] = pl <= n && kl < key[t] ? pl : lb[t];
            ub[t] = pu <= n && ku <= key[t] ? pu : ub[t];
        }
    }
}

}  // namespace

// ---- nw_band_classify: the reads it finishes without the DP --------------------------
// Sort key of every read: its length bucket, or cap + 2 for a read identical to the
// amplicon (case-insensitive, A C G T only).  Such a read needs no DP: its full
// diagonal scores S = maxsub * La, every other alignment pairs at most La - 1
// residues (S > UB of the one-diagonal band, the certificate of nw_band_device.h), so the
// alignment is the diagonal and the start cell the corner: this kernel writes its
// strings and record right away, and the sort keeps it out of the band passes.
// Wavefront batches of 64 reads, kCand compares in flight; 4 bytes per lane and compare:
// (byte | 0x20) folds case, the amplicon's folded dwords are 0 at non-ACGT bases.
//
// Reads of the amplicon's length with ONE substitution (A C G T against A C G T; ops output,
// an A C G T amplicon of at most 256 bp) need no DP either.  With k mismatches on the main
// diagonal its sum is D = m (La - 1) - x for k = 1 (m = maxsub, x = -mismatch = 4 m / 5).  Any
// alignment with an internal gap pairs at most La - 1 residues and pays at least the gap
// open O: <= m (La - 1) - O < D when O > x (EMBOSS's 10 vs 4, scaled).  One without is a
// single diagonal d with free end gaps: |d| >= 2 pairs at most La - 2 residues (m (La - 2) <
// D as m > x); d = +1 / -1 score m p - x (La - 1 - p) for p matches of their La - 1 pairs,
// below D exactly when p <= La - 2: each needs one mismatch (shifted byte compares, ballots).
// So the diagonal is the unique optimum; along it M(i, i) = D_i >= m i - m - x >= X(i, i),
// Y(i, i) (<= m (i - 1) - O), so M wins every traceback tie: the record is the diagonal's,
// as the exact copy's.  ~8 % of C2's reads (a third of the 1-3 substitution
// class and of the 1 % noise class) leave the DP this way.

__device__ __forceinline__ unsigned ld_dw(const uint8_t* p) { return *(const unsigned*)p; }

#ifndef NW_NO_SUB3
#define NW_NO_SUB3 0   // A/B builds only (scripts/diag/build_variant.sh): classify without the 3-substitution certificate
#endif
#ifndef NW_NO_INDEL1
#define NW_NO_INDEL1 0   // ... without the one-indel certificate
#endif
constexpr int kIndelMax = 10;   // classify's one-indel certificate: gaps of at most this many residues
constexpr int kCand = NW_CAND; // exact-copy candidates compared together (2 dword loads each in flight)

// Packed input (KernelArgs::pk_words): the 4 bases at batch position p as bytes A C T G (an
// exception's place reads as A: its read is flagged).  The stream's dword k holds positions
// pk_pos0 + 16 k .. + 15, 2 bits each; the device copy has a spare dword past its end.
__device__ __forceinline__ unsigned pk_decode4(const KernelArgs& a, long long p) {
    const long long q = p - a.pk_pos0;
    const unsigned* w = a.pk_words + (q >> 4);
    const unsigned x = __builtin_amdgcn_alignbit(w[1], w[0], (unsigned)(2 * (q & 15))) & 0xffu;
    const unsigned sel = (x | (x << 6) | (x << 12) | (x << 18)) & 0x03030303u;   // one code per byte
    return __builtin_amdgcn_perm(0u, 0x47544341u, sel);   // 0 1 2 3 -> 'A' 'C' 'T' 'G'
}

// the low 8 bits of x (4 bases) as bytes A C T G
__device__ __forceinline__ unsigned pk_expand(unsigned x) {
    x &= 0xffu;
    return __builtin_amdgcn_perm(0u, 0x47544341u, (x | (x << 6) | (x << 12) | (x << 18)) & 0x03030303u);
}

// pk_decode4 at a 4-aligned position (the four bases sit in one stream dword: one load)
__device__ __forceinline__ unsigned pk_decode4_al(const KernelArgs& a, long long p) {
    const long long q = p - a.pk_pos0;
    const unsigned x = (a.pk_words[q >> 4] >> (unsigned)(2 * (q & 15))) & 0xffu;
    const unsigned sel = (x | (x << 6) | (x << 12) | (x << 18)) & 0x03030303u;
    return __builtin_amdgcn_perm(0u, 0x47544341u, sel);
}

// First exception at or after batch position `pos` in [pk_e0, pk_e1): a 64-ary search by one
// wavefront (every lane samples a pivot; ~3 dependent loads for a million exceptions).
__device__ inline long long exc_lower_bound(const KernelArgs& a, long long pos, int lane) {
    long long lo = a.pk_e0, hi = a.pk_e1;
    while (hi - lo > 64) {
        const long long step = (hi - lo + 63) / 64;
        const long long idx = lo + lane * step;
        const bool below = idx < hi && a.pk_exc_pos[idx] < pos;
        const int k = (int)__builtin_popcountll(__ballot(below));   // pivots below pos: lanes 0 .. k - 1
        const long long nlo = k == 0 ? lo : lo + (long long)(k - 1) * step + 1;
        hi = min(hi, lo + (long long)k * step);
        lo = nlo;
    }
    const long long idx = lo + lane;
    const bool below = idx < hi && a.pk_exc_pos[idx] < pos;
    return lo + (long long)__builtin_popcountll(__ballot(below));
}

// (classify and nw_band_cert) the bases 16 t + i < len of a 2-bit word (one bit per base)
__device__ __forceinline__ unsigned vmask16(int t, int len) {
    const int b = len - 16 * t;
    return b >= 16 ? 0x55555555u : (b <= 0 ? 0u : 0x55555555u >> (32 - 2 * b));
}
// 16 bases of the packed stream from batch position p
__device__ __forceinline__ unsigned pk_word16(const KernelArgs& a, long long p) {
    const long long q = p - a.pk_pos0;
    const unsigned* w = a.pk_words + (q >> 4);
    return __builtin_amdgcn_alignbit(w[1], w[0], (unsigned)(2 * (q & 15)));
}
// 16 bases of the amplicon from position p (its 2-bit words in LDS)
__device__ __forceinline__ unsigned amp_word16(const unsigned* amp2s, int p) {
    return __builtin_amdgcn_alignbit(amp2s[(p >> 4) + 1], amp2s[p >> 4], (unsigned)(2 * (p & 15)));
}
// A lane's read of the amplicon's length at batch position my_off: its 2-bit words shifted to base 0
// (rw[16] = 0; bases past the read are masked by the users); c: the lane holds such a read
__device__ __forceinline__ void load_read_words(const KernelArgs& a, bool c, long long my_off, unsigned (&rw)[17]) {
    const int nw = (a.La + 15) >> 4;   // <= 16
    const long long q0 = my_off - a.pk_pos0;
    const unsigned* src = a.pk_words + (q0 >> 4);
    const unsigned s2 = (unsigned)(2 * (q0 & 15));
    unsigned wd[17];
#pragma unroll
    for (int t = 0; t < 17; ++t) wd[t] = c && t <= nw ? src[t] : 0u;   // <= the read's last dword + 1
#pragma unroll
    for (int t = 0; t < 16; ++t) rw[t] = __builtin_amdgcn_alignbit(wd[t + 1], wd[t], s2);
    rw[16] = 0u;
}
// Its main diagonal against the amplicon's words (LDS): mismatches k, the first, second and last
// mismatching base (-1: none); xf_, xl_ (classify<true, true>; null: not wanted): the read's 2-bit difference
// from the amplicon at f and at l -- the read's base there is the amplicon's XOR it
__device__ __forceinline__ void main_diag_mism(const unsigned (&rw)[17], const unsigned* amp2s, int La, int* k_, int* f_,
                                               int* f2_, int* l_, unsigned* xf_ = nullptr, unsigned* xl_ = nullptr) {
    const int nw = (La + 15) >> 4;
    int k = 0, f = -1, f2 = -1, l = -1;
    unsigned xfw = 0u, xlw = 0u;   // the difference words holding f and l
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        if (t >= nw) continue;
        const unsigned x = rw[t] ^ amp2s[t];
        const unsigned m = (x | (x >> 1)) & vmask16(t, La);
        k += __builtin_popcount(m);
        if (m != 0u && f >= 0 && f2 < 0) f2 = 16 * t + (__builtin_ctz(m) >> 1);
        if (m != 0u && f < 0) {
            f = 16 * t + (__builtin_ctz(m) >> 1);
            xfw = x;
            const unsigned m2 = m & (m - 1u);
            if (m2 != 0u) f2 = 16 * t + (__builtin_ctz(m2) >> 1);
        }
        if (m != 0u) {
            l = 16 * t + ((31 - __builtin_clz(m)) >> 1);
            xlw = x;
        }
    }
    *k_ = k;
    *f_ = f;
    *f2_ = f2;
    *l_ = l;
    if (xf_) *xf_ = (xfw >> (2 * (f & 15))) & 3u;
    if (xl_) *xl_ = (xlw >> (2 * (l & 15))) & 3u;
}

// The shifted diagonals of a read that equals the amplicon but at its bases f <= l (classify's one- and
// two-substitution certificates, lane path): on diagonal +-sh it mismatches exactly where the amplicon
// mismatches itself at that shift (A_sh[q] = amp[q] != amp[q + sh]), but at the one pair per substituted
// base p that holds the read's base p -- pair q = p - sh of d = +sh (read q + sh against amplicon q), pair
// q = p of d = -sh (read q against amplicon q + sh).  So a diagonal's count, and its counts over q >= qa and
// q <= qb, are the prefix counts C_sh of A_sh (the image's last words, nw_host.cpp cls_image: word q holds
// C_1, C_2, C_3 [q] in its bytes, constant from q = La - sh on) corrected at those pairs.  Per lane: the
// words f - 3 .. f + 1 and l - 3 .. l + 1 (clamped to [0, La]) and 16 amplicon bases from f - 3 and l - 3.
struct Sub12Tab {
    unsigned cf[5], cl[5];   // prefix-count words f - 3 + j, l - 3 + j
    unsigned af, al;         // amplicon bases from max(f - 3, 0) / max(l - 3, 0)
    int of, ol;              // f's / l's place in them (<= 3)
    unsigned rf, rl, tot;    // the read's bases f and l; the totals (word La)
    int La, f, l;
    __device__ __forceinline__ void load(const unsigned* selfc, const unsigned* amp2s, int La_, int f_, int l_, unsigned xf,
                                         unsigned xl) {
        La = La_;
        f = f_;
        l = l_;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            cf[j] = selfc[min(max(f - 3 + j, 0), La)];
            cl[j] = selfc[min(max(l - 3 + j, 0), La)];
        }
        tot = selfc[La];
        const int bf = min(max(f - 3, 0), La), bl = min(max(l - 3, 0), La);   // (a lane without a mismatch: f = l = -1)
        of = max(f, 0) - bf;
        ol = max(l, 0) - bl;
        af = amp_word16(amp2s, bf);
        al = amp_word16(amp2s, bl);
        rf = ((af >> (2 * of)) & 3u) ^ xf;
        rl = ((al >> (2 * ol)) & 3u) ^ xl;
    }
    // diagonal d = sgn * sh: mismatches, any at q >= qa, any at q <= qb (nw_band_classify's `shifted`); the
    // callers' ranges: ENDS (d = +1: qa = f, qb = l - 2; d = -1: qa = f + 1, qb = l - 1), else qa = 0, qb = La
    template <bool ENDS>
    __device__ __forceinline__ void shifted(int sgn, int sh, int* tot_, bool* ge, bool* le) const {
        const int qa = !ENDS ? 0 : (sgn > 0 ? f : f + 1), qb = !ENDS ? La : (sgn > 0 ? l - 2 : l - 1);
        const int bs = 8 * (sh - 1), n = max(0, La - sh);
        auto cnt = [&](unsigned w) { return (int)((w >> bs) & 0xffu); };
        // C_sh at qa and at qb + 1, clamped to [0, n]
        int ca, cb;
        if (!ENDS) {
            ca = 0;
            cb = cnt(tot);
        } else if (sgn > 0) {
            ca = cnt(cf[3]);   // qa = f
            cb = cnt(cl[2]);   // qb + 1 = l - 1
        } else {
            ca = cnt(cf[4]);   // qa = f + 1
            cb = cnt(cl[3]);   // qb + 1 = l
        }
        int t = cnt(tot), g = t - ca, e = cb;
        // the pair holding the read's base p (j = 3 + q - p: the prefix-count words q and q + 1 of p's five)
        auto fix = [&](int p, const unsigned (&c)[5], unsigned aw, int o, unsigned rp) {
            const int q = sgn > 0 ? p - sh : p, j = sgn > 0 ? 3 - sh : 3;
            const bool in = q >= 0 && q < n;
            const unsigned other = (aw >> (2 * max(o + (sgn > 0 ? -sh : sh), 0))) & 3u;   // amp[q] / amp[q + sh]
            const int d = in ? (int)(rp != other) - (cnt(c[j + 1]) - cnt(c[j])) : 0;
            t += d;
            if (q >= qa) g += d;
            if (q <= qb) e += d;
        };
        fix(f, cf, af, of, rf);
        if (l != f) fix(l, cl, al, ol, rl);
        *tot_ = t;
        *ge = g > 0;
        *le = e > 0;
    }
};

// The three-substitution certificate's per-read checks (i)-(iii) (classify, below; lanes s3: reads of the
// amplicon's length with three mismatches on the main diagonal, at bases f < f2 < l; the caller checked
// sub3_ok).  Called by the whole wavefront; fact: the wavefront's LDS for the diagonals' mismatch places
// (kSub3FactWords).  The diagonal loop stays rolled (its scans unrolled once: the kernel's code fits the
// instruction cache), the facts the pair test (ii) needs go through LDS.
constexpr int kSub3FactWords = 14 * 64;   // diagonals -3 .. 3: first two | last two mismatches, per lane
__device__ __forceinline__ bool cert_sub3(const KernelArgs& a, const unsigned* amp2s, const unsigned (&rw)[17], bool s3,
                                          int f, int f2, int l, long long my_off, unsigned* fact) {
    const int La = a.La, nw = (La + 15) >> 4, sc5 = a.band_maxsub / 5, lane = threadIdx.x & 63;
    const int m3 = a.band_maxsub, x3 = 4 * sc5, O3 = a.gap_open, D3 = 3 * (m3 + x3);
    // jogs (iii): diagonals +-1 against the 16 read bases from f + 1 (up to l - 1), one
    // word each from the packed stream (random sequence mismatches there; a read whose
    // diagonals +-1 match all 16 is left to the DP)
    bool jog_in[2] = {false, false};
    if (s3) {
        const int len = min(16, l - f - 1);
        const unsigned lm = len <= 0 ? 0u : (len >= 16 ? 0x55555555u : (0x55555555u >> (32 - 2 * len)));
        const unsigned rd = pk_word16(a, my_off + f + 1);
        const unsigned zp = rd ^ amp_word16(amp2s, f), zm = rd ^ amp_word16(amp2s, f + 2);   // d = +1 / -1
        jog_in[1] = ((zp | (zp >> 1)) & lm) != 0u;
        jog_in[0] = ((zm | (zm >> 1)) & lm) != 0u;
    }
    bool ok3 = s3;
    // per diagonal d = -5 .. 5: mismatches (capped at 3), the first two and the last two (read index;
    // last ones + 1) over the diagonal's pairs; (i) single diagonals 1 <= |d| <= 5 need more than
    // (3 (m + x) - m |d|) / (m + x) mismatches each
#pragma unroll 1
    for (int d = -5; d <= 5; ++d) {
        int a1 = f, a2 = f2, b1 = l + 1, b2 = f2 + 1;   // d = 0: the main diagonal's three (k == 3)
        if (d != 0) {
            const int sh = d > 0 ? d : -d;
            a1 = La; a2 = La; b1 = 0; b2 = 0;
            // the first two and the last two by scans from either end that stop once every lane has
            // found two (random sequence: within a word); the count up to 3 follows (3 when the
            // second-last lies past the second)
            auto word = [&](int t) -> unsigned {
                // d > 0: read base j = i + d against amplicon base i (words of i); d < 0: read
                // base j against amplicon base j - d (words of j)
                const unsigned am = d > 0 ? amp2s[t]
                                          : __builtin_amdgcn_alignbit(amp2s[t + 1], amp2s[t], (unsigned)(2 * sh));
                const unsigned rd = d > 0 ? __builtin_amdgcn_alignbit(rw[t + 1], rw[t], (unsigned)(2 * sh)) : rw[t];
                const unsigned z = rd ^ am;
                return (z | (z >> 1)) & vmask16(t, La - sh);
            };
            const int o0 = d > 0 ? d : 0;   // read index of a word's base 0, past 16 t
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                if (__ballot(s3 && a2 == La && t < nw) == 0ull) break;
                const unsigned mk = word(t);
                const int off = 16 * t + o0;
                if (mk != 0u && a1 == La) {
                    a1 = off + (__builtin_ctz(mk) >> 1);
                    const unsigned m2 = mk & (mk - 1u);
                    if (m2 != 0u) a2 = off + (__builtin_ctz(m2) >> 1);
                } else if (mk != 0u && a2 == La) {
                    a2 = off + (__builtin_ctz(mk) >> 1);
                }
            }
#pragma unroll
            for (int t = 15; t >= 0; --t) {
                if (__ballot(s3 && b2 == 0 && a1 < La) == 0ull) break;
                if (t >= nw) continue;
                const unsigned mk = word(t);
                const int off = 16 * t + o0;
                if (mk != 0u && b1 == 0) {
                    const int hb = 31 - __builtin_clz(mk);
                    b1 = off + (hb >> 1) + 1;
                    const unsigned mh = mk & ~(1u << hb);
                    if (mh != 0u) b2 = off + ((31 - __builtin_clz(mh)) >> 1) + 1;
                } else if (mk != 0u && b2 == 0) {
                    b2 = off + ((31 - __builtin_clz(mk)) >> 1) + 1;
                }
            }
            // (|d| >= 4: the score test needs one mismatch, no pair test reads the diagonal)
            const int cc = a1 == La ? 0 : (a2 == La ? 1 : (b2 > a2 ? 3 : 2));
            ok3 = ok3 && m3 * sh + (m3 + x3) * cc > D3;
        }
        if (d >= -3 && d <= 3) {
            fact[(d + 3) * 128 + lane] = (unsigned)a1 | ((unsigned)a2 << 16);
            fact[(d + 3) * 128 + 64 + lane] = (unsigned)b1 | ((unsigned)b2 << 16);
        }
    }
    // (ii) one gap, prefix on d1, suffix on d2 (|d| <= 3), with at most w_max mismatches in all: it exists
    // iff, in read coordinates, the prefix's mismatches on d1 end before the suffix's on d2 begin (the
    // suffix starts max(0, d2 - d1) read bases later: those are the gap's)
    unsigned fa[7], fb[7];
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        fa[e] = fact[e * 128 + lane];
        fb[e] = fact[e * 128 + 64 + lane];
    }
#pragma unroll
    for (int e1 = 0; e1 < 7; ++e1) {
#pragma unroll
        for (int e2 = 0; e2 < 7; ++e2) {
            if (e1 == e2) continue;
            const int d1 = e1 - 3, d2 = e2 - 3, g = d2 > d1 ? d2 - d1 : d1 - d2;
            // unpaired residues of the amplicon (= of the read): its leading / trailing overhang
            // and the gap's residues when the gap is in the read (the diagonal falls)
            const int U = (d1 < 0 ? -d1 : 0) + (d2 > 0 ? d2 : 0) + (d1 > d2 ? d1 - d2 : 0);
            const int slack = D3 - m3 * U - O3 - (g - 1) * a.gap_extend;   // (m + x) w must not exceed it
            if (slack < 0) continue;
            const int wmax = slack / (m3 + x3);
            const int gb = d2 > d1 ? d2 - d1 : 0;   // read bases in the gap
            const int df1 = (int)(fa[e1] & 0xffffu), df2 = (int)(fa[e1] >> 16);
            const int dg1 = (int)(fb[e2] & 0xffffu), dg2 = (int)(fb[e2] >> 16);
            bool exists = dg1 - gb <= df1;
            if (wmax >= 1) exists = exists || dg2 - gb <= df1 || dg1 - gb <= df2;
            if (wmax >= 2) exists = true;   // (not reached with the gate's parameters: reject)
            ok3 = ok3 && !exists;
        }
    }
    // (iii) jogs through d = +-1: a mismatch of that diagonal in [f + 1, l - 1] (read index)
    return ok3 && l - f >= 2 && jog_in[0] && jog_in[1];
}

// The one-indel certificate (classify, below; lanes ci: reads of La -+ kab bases, 1 <= kab <= the
// certificate's largest gap, at batch position my_off).  True: certified, *gk_ the gap's read index q
// (runs M q, the gap, M the rest).  Called by the whole wavefront.
// ONEPASS: the candidate's own two diagonals (shifts 0 and kab, the only scans that run to the gap -- between
// them nearly every word of the read) in one unrolled pass without exit tests; false: by the `ends` scans,
// as every other shift (CRISPR_NW_INDEL_ONEPASS=0: the reference the tests hold the pass to).  A template
// parameter: the kernel's code has to fit the instruction cache.
template <bool ONEPASS>
__device__ __forceinline__ bool cert_indel(const KernelArgs& a, const unsigned* amp2s, bool ci, long long my_off, int my_len,
                                           int* gk_) {
    const int La = a.La, n2 = (La + 15) / 16 + 2, sc5 = a.band_maxsub / 5;
    const int dl = my_len - La, kab = dl < 0 ? -dl : dl;
    const bool del = dl < 0;
    const int Ls = del ? my_len : La, Ll = del ? La : my_len;
    unsigned rw[18];
    {
        const long long q0 = my_off - a.pk_pos0;
        const unsigned* src = a.pk_words + (q0 >> 4);
        const unsigned s2 = (unsigned)(2 * (q0 & 15));
        const int nrw = (my_len + 15) >> 4;
        unsigned wd[18];
#pragma unroll
        for (int t = 0; t < 18; ++t) wd[t] = ci && t <= nrw ? src[t] : 0u;
#pragma unroll
        for (int t = 0; t < 17; ++t) rw[t] = __builtin_amdgcn_alignbit(wd[t + 1], wd[t], s2);
        rw[17] = 0u;
    }
    auto vmask = [](int t, int len) -> unsigned {   // bases 16 t + i < len
        const int b = len - 16 * t;
        return b >= 16 ? 0x55555555u : (b <= 0 ? 0u : 0x55555555u >> (32 - 2 * b));
    };
    const int mm = a.band_maxsub, xx = 4 * sc5;
    const int S = mm * Ls - a.gap_open - (kab - 1) * a.gap_extend;
    bool ok = false;
    int gk = 0;
    // the longer sequence l and the shorter s: the amplicon's words from LDS, the read's from
    // registers, picked per lane (deletion and insertion reads in one pass over the shifts)
    if (ci) {
        auto am = [&](int t) -> unsigned { return t < n2 ? amp2s[t] : 0u; };
        // (ONEPASS: picked once, by selects -- the amplicon's words past its last read as its spare zero word)
        unsigned pl[18], ps[17];
        if constexpr (ONEPASS) {
#pragma unroll
            for (int t = 0; t < 18; ++t) {
                const unsigned av = amp2s[min(t, n2 - 1)];
                pl[t] = del ? av : rw[t];
                if (t < 17) ps[t] = del ? rw[t] : av;
            }
        }
        auto wl = [&](int t) -> unsigned {
            if constexpr (ONEPASS) return pl[t];
            else return del ? am(t) : rw[t];
        };
        auto ws = [&](int t) -> unsigned {
            if constexpr (ONEPASS) return ps[t];
            else return del ? rw[t] : am(t);
        };
        bool o = true;
        // first and last mismatch of a shift (one side's sequence shifted by sh against the
        // other's, P positions): scans from either end that stop as soon as every lane has found
        // one (random sequence mismatches within a word; only the two diagonals of the
        // candidate run to the gap).  Mismatches: 0 (f == P), 1 (f == g - 1) or >= 2 -- all the
        // score test needs (its bound falls with the count)
        auto ends = [&](auto lw, auto rw2, int sh, int P, int* f, int* g) {
            int ff = P, gg = 0;
#pragma unroll
            for (int t = 0; t < 17; ++t) {
                if (__ballot(ff == P && 16 * t < P) == 0ull) break;
                const unsigned z = __builtin_amdgcn_alignbit(lw(t + 1), lw(t), (unsigned)(2 * sh)) ^ rw2(t);
                const unsigned mk = (z | (z >> 1)) & vmask(t, P);
                ff = (ff == P && mk != 0u) ? 16 * t + (int)(__builtin_ctz(mk) >> 1) : ff;
            }
#pragma unroll
            for (int t = 16; t >= 0; --t) {
                if (__ballot(gg == 0 && ff < P) == 0ull) break;   // (words past P: mk == 0)
                const unsigned z = __builtin_amdgcn_alignbit(lw(t + 1), lw(t), (unsigned)(2 * sh)) ^ rw2(t);
                const unsigned mk = (z | (z >> 1)) & vmask(t, P);
                gg = (gg == 0 && mk != 0u) ? 16 * t + (int)((31 - __builtin_clz(mk)) >> 1) + 1 : gg;
            }
            *f = ff;
            *g = gg;
        };
        auto cnt = [](int f, int g, int P) { return f == P ? 0 : (f == g - 1 ? 1 : 2); };
        // shifts sh = 0 .. kab + 3 of l; for sh <= kab the pair test G[s2] > F[s1] (s1 < s2) as a
        // running maximum of F: every earlier shift's for s2 < kab, shifts 1 .. kab - 1 for s2 =
        // kab (the pair (0, kab) is the candidate).  F / G are indices of s, P = Ls there.
        // the shifts past kab and the other side's need only enough mismatches for the score test
        // (the smallest c with m (P - c) - x c < S, 0 .. 2; more: the DP): forward scans that stop
        // once that many are found
        auto enough = [&](auto lw, auto rw2, int sh, int P) -> bool {
            int need = 0;
            while (need <= 2 && !(mm * (P - need) - xx * need < S)) ++need;
            int c = 0;
#pragma unroll
            for (int t = 0; t < 17; ++t) {
                if (__ballot(c < need && need <= 2 && 16 * t < P) == 0ull) break;
                const unsigned z = __builtin_amdgcn_alignbit(lw(t + 1), lw(t), (unsigned)(2 * sh)) ^ rw2(t);
                c += c < need ? __builtin_popcount((z | (z >> 1)) & vmask(t, P)) : 0;
            }
            return need <= 2 && c >= need;
        };
        int f0 = Ls, fmax_all = -1, fmax_1 = -1;
        if constexpr (ONEPASS) {
            // Shifts 0 and kab over all 17 words, no ballot and no exit: per word both mismatch masks (one bit
            // per base, here the odd one: ((z << 1) | z) & mask is one instruction) under one length mask --
            // 0xaaaaaaaa below the lane's last word wl_ = Ls >> 4, the partial mask pm there, 0 past it; wl_ and
            // pm hoisted.  Shift 0 wants F (the first mismatch) and shift kab G (the last, + 1): the first / the
            // last word with a nonzero mask and its index (a compare and two selects per word each), ctz / clz
            // once after the loop.  The count classes (0, 1, >= 2 mismatches: what cnt takes from f and g) come
            // from the masks' popcounts.  (126 VGPRs, as the scans' 127: 4 wavefronts per SIMD.)
            const int wl_ = Ls >> 4;
            const unsigned pm = (Ls & 15) ? 0xaaaaaaaau >> (32 - 2 * (Ls & 15)) : 0u;
            const unsigned s2k = (unsigned)(2 * kab);
            unsigned w0 = 0u, wk = 0u;   // shift 0's first nonzero mask word, shift kab's last
            int i0 = 0, ik = 0, n0 = 0, nk = 0;   // their word indices; the two diagonals' mismatches
#pragma unroll
            for (int t = 0; t < 17; ++t) {
                const unsigned vm = t < wl_ ? 0xaaaaaaaau : (t == wl_ ? pm : 0u);
                const unsigned lo = wl(t), sw = ws(t);
                const unsigned zk = __builtin_amdgcn_alignbit(wl(t + 1), lo, s2k) ^ sw, z0 = lo ^ sw;
                const unsigned mk = ((zk << 1) | zk) & vm, m0 = ((z0 << 1) | z0) & vm;
                nk += __builtin_popcount(mk);
                n0 += __builtin_popcount(m0);
                wk = mk != 0u ? mk : wk;   // the last nonzero word so far
                ik = mk != 0u ? t : ik;
                i0 = w0 == 0u ? t : i0;    // the first: words are taken while none was nonzero
                w0 = w0 == 0u ? m0 : w0;
            }
            f0 = w0 != 0u ? 16 * i0 + (int)(__builtin_ctz(w0) >> 1) : Ls;
            gk = wk != 0u ? 16 * ik + (int)((31 - __builtin_clz(wk)) >> 1) + 1 : 0;
            const int c0 = min(n0, 2), ck = min(nk, 2);
            const bool o0 = mm * (Ls - c0) - xx * c0 < S, ok_k = mm * (Ls - ck) - xx * ck < S;
            o = o0;   // shift 0; its F seeds the running maximum
            fmax_all = f0;
            for (int sh = 1; sh < kab; ++sh) {
                int f, g;
                ends(wl, ws, sh, Ls, &f, &g);
                const int c = cnt(f, g, Ls);
                o = o && mm * (Ls - c) - xx * c < S && g > fmax_all;
                fmax_all = max(fmax_all, f);
                fmax_1 = max(fmax_1, f);
            }
            o = o && ok_k && gk > fmax_1;   // shift kab, against shifts 1 .. kab - 1
        } else {
            for (int sh = 0; sh <= kab; ++sh) {
                int f, g;
                ends(wl, ws, sh, Ls, &f, &g);
                const int c = cnt(f, g, Ls);
                o = o && mm * (Ls - c) - xx * c < S;
                if (sh == 0) f0 = f;
                if (sh > 0) o = o && g > (sh == kab ? fmax_1 : fmax_all);
                if (sh == kab) gk = g;
                fmax_all = max(fmax_all, f);
                if (sh > 0) fmax_1 = max(fmax_1, f);
            }
        }
        for (int sh = kab + 1; sh <= kab + 3; ++sh) o = o && enough(wl, ws, sh, Ll - sh);
        for (int sh = 1; sh <= 3; ++sh) o = o && enough(ws, wl, sh, Ls - sh);   // s shifted against l
        ok = ci && o && gk >= 1 && gk <= f0;
    }
    *gk_ = gk;
    return ok;
}

// (write_read_bytes) the dword v of batch positions p .. p + 3 into the bytes of the read [o, e) among them
__device__ __forceinline__ void store_read_dword(uint8_t* dst, long long p, long long o, long long e, unsigned v) {
    if (p >= o && p + 4 <= e) {
        *(unsigned*)(dst + p) = v;
    } else {
        for (int b = 0; b < 4; ++b)
            if (p + b >= o && p + b < e) dst[p + b] = (uint8_t)(v >> (8 * b));
    }
}

// Packed input: the bytes of the reads in dp (the lanes' reads at my_off, my_len; the whole wavefront)
// decoded into a.reads -- each read's own bytes exactly, and every byte stored once, as its final value:
// the reads in excm hold exception bytes (the block's slice [x0, x1) of the call's list), which replace
// the decoded 'A' of their places in registers, before the store.
// Within one pass a read's bytes are written by its own wavefront only (neighbouring reads' bytes are
// never touched: no races between blocks or chunks of the pass).  Across the two passes of a dual call
// (both decode the same reads into the same buffer, on concurrent streams) the rule is DESIGN.md 4c's:
// while a kernel of one pass may read a byte, the other pass stores nothing but that byte's final value
// to it -- which holds because no store here ever carries a provisional byte.
__device__ __forceinline__ void write_read_bytes(const KernelArgs& a, unsigned long long dp, long long my_off, int my_len,
                                                 unsigned long long excm = 0ull, long long x0 = 0, long long x1 = 0) {
    const int lane = threadIdx.x & 63;
    // the reads holding exceptions (rare): one at a time, each dword patched from the exception list
    for (unsigned long long de = dp & excm; de; de &= de - 1) {
        const int u = (int)__builtin_ctzll(de);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)my_off, u);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(my_off >> 32), u);
        const long long o = (long long)(((unsigned long long)hi << 32) | lo);
        const long long e = o + __builtin_amdgcn_readlane(my_len, u);
        for (long long p = (o & ~3ll) + 4 * lane; p < e; p += 256) {
            unsigned v = pk_decode4_al(a, p);
            long long t = x0, th = x1;   // the first exception at or after p
            while (t < th) {
                const long long mid = (t + th) >> 1;
                if (a.pk_exc_pos[mid] < p) t = mid + 1;
                else th = mid;
            }
            for (; t < x1; ++t) {
                const long long q = a.pk_exc_pos[t];
                if (q >= p + 4) break;
                const unsigned sh = 8u * (unsigned)(q - p);
                v = (v & ~(0xffu << sh)) | ((unsigned)pk_exc_store_byte(a.pk_exc_byte[t]) << sh);
            }
            store_read_dword(const_cast<uint8_t*>(a.reads), p, o, e, v);
        }
    }
    dp &= ~excm;
    // kWr reads at a time, lane l their dwords l, l + 64, ...: all their loads in flight
    // before any store (one read per round trip measured 2.7x the byte-input classify)
    constexpr int kWr = 8;
    uint8_t* dst = const_cast<uint8_t*>(a.reads);
    while (dp) {
        long long o[kWr], e[kWr];
        int rounds = 0;
#pragma unroll
        for (int t = 0; t < kWr; ++t) {
            o[t] = e[t] = 0;
            if (dp) {
                const int u = (int)__builtin_ctzll(dp);
                dp &= dp - 1;
                const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)my_off, u);
                const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(my_off >> 32), u);
                o[t] = (long long)(((unsigned long long)hi << 32) | lo);
                e[t] = o[t] + __builtin_amdgcn_readlane(my_len, u);
                const int span = (int)(e[t] - (o[t] & ~3ll));
                rounds = max(rounds, (span + 255) >> 8);
            }
        }
        for (int rd2 = 0; rd2 < rounds; ++rd2) {
            unsigned v[kWr];
#pragma unroll
            for (int t = 0; t < kWr; ++t) {
                const long long p = (o[t] & ~3ll) + 256 * rd2 + 4 * lane;
                v[t] = p < e[t] ? pk_decode4_al(a, p) : 0u;
            }
#pragma unroll
            for (int t = 0; t < kWr; ++t) {
                const long long p = (o[t] & ~3ll) + 256 * rd2 + 4 * lane;
                if (p >= e[t]) continue;
                store_read_dword(dst, p, o[t], e[t], v[t]);
            }
        }
    }
}


// (5 wavefronts per SIMD; forced to 6 / 8 with 31 / 60 VGPRs spilled it ran 0.188 / 0.223 vs 0.150 ms per resident
// pass in round 5; at 6 again once nothing spilled at 5: 39 spilled, 0.350 vs 0.327 ms)
#ifndef NW_CLASSIFY_WPE
#define NW_CLASSIFY_WPE 5
#endif
// TAB (packed input): the lane path's one- and two-substitution certificates take their shifted diagonals'
// facts from the amplicon's self-mismatch prefix counts (the image's last words) instead of word passes
// over the read -- a template parameter: the kernel's code has to fit the instruction cache
template <bool PK, bool TAB = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NW_CLASSIFY_WPE))) void nw_band_classify(const KernelArgs a) {
    extern __shared__ unsigned amp_sh[];   // [nd] folded amplicon dwords (0 at non-ACGT), [nd] raw dwords
    constexpr int kRbw = 66;               // a window read's 16-base words (Lb < La <= 1024) + a zero word
    __shared__ unsigned s_rbw[4][kRbw];
    __shared__ unsigned s_known[18];       // the known sequence's 2-bit words (KernelArgs::known2; La <= 256)
    const int La = a.La, nd = (La + 3) / 4;
    // the chunk's counters (fallback / redo counts, spill bump and error flag): zeroed
    // here, the first kernel of the chain, instead of by memset launches
    if (blockIdx.x == 0 && threadIdx.x < kChunkCounters) a.fallback_count[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x < kSpillCtl && a.ops) a.ops_ctl[threadIdx.x] = 0;
    if (blockIdx.x == 0 && a.zero_ctl64 && (int)threadIdx.x < a.zero_ctl64_n) a.zero_ctl64[threadIdx.x] = 0;
    // packed input, block b: the chunk's reads of call block B = call_lo / kPkBlock + b, [bl, bh)
    // (kPkBlock reads, one per thread; four blocks per group of kLenGroup lengths).  Its lengths'
    // loads go out before the image copy's barrier.
    constexpr int kPkBlock = 256;
    static_assert(kLenGroup % kPkBlock == 0, "blocks tile the length groups");
    const long long pB = a.pk_call_lo / kPkBlock + blockIdx.x;
    const long long pbl = max(0ll, pB * kPkBlock - a.pk_call_lo), pbh = min(a.n, (pB + 1) * kPkBlock - a.pk_call_lo);
    const long long pG = pB * kPkBlock / kLenGroup, pg0 = pG * kLenGroup;
    const long long prr = pB * kPkBlock + threadIdx.x - a.pk_call_lo;   // chunk-relative
    long long pk_l = 0, pk_pre = 0;   // this thread's read length; the group's lengths before the block (<= 3 per thread)
    if (PK && a.pk_len) {
        pk_l = prr < pbh ? (long long)a.pk_len[pB * kPkBlock + threadIdx.x] : 0ll;
        for (long long q = pg0 + threadIdx.x; q < pB * kPkBlock; q += kPkBlock) pk_pre += a.pk_len[q];
    }
    // the amplicon's folded and raw dwords and the window seeds: the host-built image, one copy
    // (the byte-input launch sizes LDS for the amplicon dwords only: no window seeds there)
    const int img_words = PK ? a.cls_words : 2 * nd;
    for (int k = threadIdx.x; k < img_words; k += blockDim.x) amp_sh[k] = a.cls_img[k];
    if (PK && a.known2 && threadIdx.x < 18) s_known[threadIdx.x] = threadIdx.x < (La + 15) / 16 ? a.known2[threadIdx.x] : 0u;
    __syncthreads();
    const int sc5 = a.band_maxsub / 5;
    // the one-substitution certificate (above): ops output, one 256-byte chunk, EDNAFULL's
    // 5 / -4 scaled, a gap open above the mismatch cost
    const bool amp_acgt_all = a.amp_acgt != 0;
    const bool sub1_ok = amp_acgt_all && a.ops && nd <= 64 && a.band_maxsub == 5 * sc5 && a.gap_open > 4 * sc5 &&
                         a.gap_extend >= 0;
    // two substitutions (x = 9/5 maxsub: a mismatch's loss against a match, D = m La - 2 x): with an
    // internal gap and <= La - 2 pairs O > 2 x - 2 m; La - 1 pairs and two gaps 2 O > 2 x - m, one gap
    // and a mismatch O > x - m; |d| >= 4 m (La - 4) < D: x < 2 m; d = +-1 / +-2 / +-3 need 2 / 1 / 1
    // mismatches (EDNAFULL); one gap, one end gap, no mismatch: excluded per read (below)
    const int mt2 = a.band_maxsub, xl = 9 * sc5;
    const bool sub2_ok = sub1_ok && 2 * a.gap_open > 2 * xl - mt2 && a.gap_open > 2 * xl - 2 * mt2 &&
                         a.gap_open > xl - mt2 && xl < 2 * mt2 && (2 * xl - mt2) / xl + 1 == 2 &&
                         (2 * xl - 2 * mt2) / xl + 1 == 1 && (2 * xl - 3 * mt2) / xl + 1 == 1;
    // one indel of k residues (below): certified for k <= indel_kmax, the largest k with m > (k - 1) E (no
    // alternative leaves a read or amplicon residue unpaired or mismatched), O > (k - 1) E (no alternative
    // with two internal gaps) and O + (k - 1) E < 4 m (no single diagonal pairing four residues fewer)
    int indel_kmax = 0;
    if (PK && !NW_NO_INDEL1 && sub1_ok && a.amp2)
        for (int k = 1; k <= kIndelMax; ++k) {
            const int p = (k - 1) * a.gap_extend;
            if (!(a.band_maxsub > p && a.gap_open > p && a.gap_open + p < 4 * a.band_maxsub)) break;
            indel_kmax = k;
        }
    // three substitutions (below): with D = m La - 3 (m + x), every alignment but the diagonal scores below
    // D when, beyond the per-read checks, x < m (|d| >= 6), 4 m + O, 2 m + 2 O and 3 O exceed 3 (m + x)
    // (one gap leaving 4 or more residues unpaired, two gaps leaving 2, three gaps) and a jog through a
    // neighbouring diagonal (two gaps, one residue of each sequence unpaired) with one mismatch scores below D
    const int m3 = a.band_maxsub, x3 = 4 * sc5, O3 = a.gap_open, D3 = 3 * (m3 + x3);
    const bool sub3_ok = !NW_NO_SUB3 && sub2_ok && x3 < m3 && 4 * m3 + O3 > D3 && 2 * m3 + 2 * O3 > D3 && 3 * O3 > D3 &&
                         m3 + 2 * O3 + (m3 + x3) > D3;
    // Wide first (KernelArgs::wf_list): a plain read of the amplicon's length with k substitutions scores
    // m La - (m + x) k on its main diagonal, and the 16-diagonal walk certifies an alignment only when
    // its score exceeds m pmax - O, pmax the longest diagonal just outside the band (an equal-length
    // pair: diagonals -7 .. 8, pmax = La - 8).  From (m + x) k >= m (La - pmax) + O on it cannot pass.
    int wf_k = 0;   // 0: off
    if (PK && a.wf_keys > 0 && a.ops && nd <= 64 && amp_acgt_all && a.amp2 && a.band_maxsub == 5 * sc5) {
        int d16 = 0;
        band_geometry2(La, La, La, &d16, 16);
        const int outside = min(1 - d16, d16 + 16);   // La - pmax
        wf_k = max(1, (a.band_maxsub * outside + a.gap_open + 9 * sc5 - 1) / (9 * sc5));
    }
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    const unsigned tail_mask = (La & 3) ? (0xffffffffu >> (8 * (4 - (La & 3)))) : 0xffffffffu;
    const int sd = (int)(a.stride / 4);
    // Window reads (packed input, ops output): a read shorter than the amplicon that equals one of its
    // windows amplicon[s, s + Lb) (A C G T, case-insensitive) scores m Lb, the most any alignment can
    // (pairs <= Lb, each <= m; a gap costs > 0), and every alignment that does is such a window: the
    // start-cell scan (last column bottom -> top) takes the largest such s, and along its diagonal M =
    // m j beats X, Y <= m j - O, so the traceback is the diagonal with free end gaps: s amplicon
    // residues before, La - s - Lb after.  One substitution (D = m (Lb - 1) - x): an alignment with an
    // internal gap pairs <= Lb residues and pays >= O, <= m Lb - O < D when O > m + x; a single
    // diagonal pairs its overlap P(d): P <= Lb - 2 scores <= m (Lb - 2) < D (m > x), P = Lb - 1 needs one
    // mismatch and P = Lb two (checked for every such diagonal, below) -- D is then the unique optimum
    // and M wins every tie along it (X, Y <= m j - O < m j - m - x <= M).  The window's offset comes from
    // the read's first (or, for a substitution there, last) 16 bases looked up among the amplicon's
    // sorted 16-mers (Profile::seed_key).
    unsigned* amp2s = amp_sh + 2 * nd;
    const int n2 = (La + 15) / 16 + 2, nseed = a.n_seed;
    unsigned* skey = amp2s + n2;
    uint16_t* spos = (uint16_t*)(skey + nseed);
    const unsigned* selfc = amp_sh + (a.cls_words - a.sub12_words);   // [La + 1] self-mismatch prefix counts (TAB)
    const bool win_ok = PK && amp_acgt_all && a.ops && a.band_maxsub == 5 * sc5 && a.gap_extend >= 0 && a.amp2 &&
                        a.gap_open > xl && nseed > 0 && La <= 1024;
    // 16 bases of the packed stream from batch position p, and of the amplicon from position p (LDS)
    auto rword = [&](long long p) -> unsigned {
        const long long q = p - a.pk_pos0;
        const unsigned* w = a.pk_words + (q >> 4);
        return __builtin_amdgcn_alignbit(w[1], w[0], (unsigned)(2 * (q & 15)));
    };
    auto aword = [&](int p) -> unsigned {
        return __builtin_amdgcn_alignbit(amp2s[(p >> 4) + 1], amp2s[p >> 4], (unsigned)(2 * (p & 15)));
    };
    // mismatches of read bases [roff + j0, + len) against amplicon [s, s + len), counted up to cap + 1:
    // 16 words (256 bases) per round with every load in flight before any compare
    auto mism = [&](long long roff, int j0, int s, int len, int cap) -> int {
        int cnt = 0;
        for (int w0 = 0; w0 < len && cnt <= cap; w0 += 256) {
            unsigned x[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) x[t] = w0 + 16 * t < len ? rword(roff + j0 + w0 + 16 * t) : 0u;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int w = w0 + 16 * t;
                if (w >= len) continue;
                unsigned y = x[t] ^ aword(s + w);
                if (len - w < 16) y &= (1u << (2 * (len - w))) - 1u;
                cnt += __builtin_popcount((y | (y >> 1)) & 0x55555555u);
            }
        }
        return cnt;
    };
    auto ham16 = [&](unsigned x, unsigned y) { const unsigned z = x ^ y; return __builtin_popcount((z | (z >> 1)) & 0x55555555u); };
    // a wavefront batch of the 64 reads r0 .. r0 + 63 (below r_end): lane u holds read r0 + u's
    // offset and length; exc: the reads holding an exception byte (packed input), their block's
    // slice [x0, x1) of the call's exception list
    auto batch = [&](long long r0, long long r_end, long long my_off, int my_len, bool exc, long long x0, long long x1) {
        const long long r = r0 + lane;
        unsigned long long cand = __ballot(my_len == La && !exc);   // reads of the amplicon's length
        unsigned long long exact = 0ull, sub1 = 0ull, sub2 = 0ull;
        unsigned long long pend3 = 0ull, pend_i = 0ull;   // queued for nw_band_cert (KernelArgs::cert_q)
        unsigned long long known = 0ull;   // copies of the known sequence (KernelArgs::known2)
        unsigned long long jog = 0ull;     // reads closer to the known sequence than to the amplicon (below)
        unsigned long long wf_sub = 0ull;  // reads of the amplicon's length with wf_k substitutions or more
        // compare kCand candidates at a time (their loads in flight together); when the read
        // fits one 256-byte chunk (La <= 256) its exact copy's rows are written right
        // away from the words already in registers
        const bool one_chunk = nd <= 64;
        unsigned long long emit_later = 0ull;
        if constexpr (PK) {
            // Packed input, ops output, an A C G T amplicon of at most 256 bp: one read per lane.  Its
            // 2-bit words (one shift of the stream's dwords) against the amplicon's give the
            // mismatches of the main diagonal; a read with one or two takes the certificates above
            // from the shifted diagonals' masks (the wave-per-candidate loop below decides the same
            // from byte compares).  Mismatch masks: one bit per base (bit 2 i of word t: base 16 t + i).
            if (a.ops && one_chunk && amp_acgt_all && a.amp2 && cand) {
                const bool c = ((cand >> lane) & 1ull) != 0ull;
                cand = 0ull;
                const int nw = (La + 15) >> 4;   // <= 16
                auto vmask = [](int t, int len) -> unsigned {   // bases 16 t + i < len
                    const int b = len - 16 * t;
                    return b >= 16 ? 0x55555555u : (b <= 0 ? 0u : 0x55555555u >> (32 - 2 * b));
                };
                unsigned rw[17];
                load_read_words(a, c, my_off, rw);
                int k, f, f2, l;   // mismatches of the main diagonal, first, second and last base
                unsigned xor_f = 0u, xor_l = 0u;   // (TAB) the read's 2-bit difference from the amplicon at f and at l
                if constexpr (TAB) main_diag_mism(rw, amp2s, La, &k, &f, &f2, &l, &xor_f, &xor_l);
                else main_diag_mism(rw, amp2s, La, &k, &f, &f2, &l);
                exact = __ballot(c && k == 0);
                wf_sub = __ballot(c && wf_k > 0 && k >= wf_k);
                const bool s1 = c && sub1_ok && k == 1, s2 = c && sub2_ok && k == 2;
                // diagonal d = sgn * sh (q <= La - 1 - sh): mismatches (counted up to 2), any at q >= qa, any at q <= qb
                auto shifted = [&](int sgn, int sh, int qa, int qb, int* tot, bool* ge, bool* le) {
                    int n = 0;
                    unsigned g = 0u, e = 0u;
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        if (t >= nw) continue;
                        const unsigned am = sgn > 0 ? amp2s[t]
                                                    : __builtin_amdgcn_alignbit(amp2s[t + 1], amp2s[t], (unsigned)(2 * sh));
                        const unsigned rd = sgn > 0 ? __builtin_amdgcn_alignbit(rw[t + 1], rw[t], (unsigned)(2 * sh)) : rw[t];
                        const unsigned x = rd ^ am;
                        const unsigned m = (x | (x >> 1)) & vmask(t, La - sh);
                        n += __builtin_popcount(m);
                        g |= m & ~vmask(t, qa);      // bases >= qa
                        e |= m & vmask(t, qb + 1);   // bases <= qb
                    }
                    *tot = n;
                    *ge = g != 0u;
                    *le = e != 0u;
                };
                if (__ballot(s1 || s2)) {
                    // S_+-1 below D: one mismatch on each (k = 1); two substitutions at bases f < l: two on
                    // each, d = +1 one at q >= f and one at q <= l - 2, d = -1 at q >= f + 1 and q <= l - 1
                    int tp, tm;
                    bool gp, lp, gm, lm;
                    Sub12Tab tb;
                    if constexpr (TAB) {
                        tb.load(selfc, amp2s, La, f, l, xor_f, xor_l);
                        tb.shifted<true>(1, 1, &tp, &gp, &lp);
                        tb.shifted<true>(-1, 1, &tm, &gm, &lm);
                    } else {
                        shifted(1, 1, f, l - 2, &tp, &gp, &lp);
                        shifted(-1, 1, f + 1, l - 1, &tm, &gm, &lm);
                    }
                    sub1 = __ballot(s1 && tp >= 1 && tm >= 1);
                    bool ok2 = s2 && tp >= 2 && tm >= 2 && gp && lp && gm && lm;
                    if (__ballot(ok2)) {   // d = +-2, +-3: one mismatch each
#pragma unroll
                        for (int sh = 2; sh <= 3; ++sh) {
                            int t2, t3;
                            bool x0, x1;
                            if constexpr (TAB) {
                                tb.shifted<false>(1, sh, &t2, &x0, &x1);
                                tb.shifted<false>(-1, sh, &t3, &x0, &x1);
                            } else {
                                shifted(1, sh, 0, La, &t2, &x0, &x1);
                                shifted(-1, sh, 0, La, &t3, &x0, &x1);
                            }
                            ok2 = ok2 && t2 >= 1 && t3 >= 1;
                        }
                    }
                    sub2 = __ballot(ok2);
                }
                // Three substitutions (round 6; bases f < f2 < l of the main diagonal, D = m La - 3 (m + x)).
                // An alignment scores m (La - U) - (m + x) w - (its gaps' cost), U residues of each sequence
                // unpaired and w mismatches; below D when m U + (m + x) w + gaps > 3 (m + x).  Left open by
                // the gate above: (i) single diagonals 1 <= |d| <= 5 with too few mismatches (each must have
                // more than (3 (m + x) - m |d|) / (m + x)); (ii) one gap between diagonals d1 (prefix) and d2
                // (suffix), |d1|, |d2| <= 3, with at most w_max mismatches in all -- it exists iff, in read
                // coordinates, the prefix's mismatches on d1 end before the suffix's on d2 begin (the suffix
                // starts max(0, d2 - d1) read bases later: those are the gap's); (iii) a jog 0 -> +-1 -> 0
                // with no mismatch: its middle covers the read bases (f, l] (d = +1) / [f, l) (d = -1), so a
                // mismatch of that diagonal in [f + 1, l - 1] excludes both.  Then the diagonal is the unique
                // optimum and M beats X and Y along it (a tie would be a second alignment scoring D).  The checks
                // (cert_sub3) run in nw_band_cert, on the queued candidates.
                const bool s3 = c && sub3_ok && k == 3;
                pend3 = __ballot(s3);   // checked by nw_band_cert
                if (a.known2) {   // a copy of the known sequence that no certificate above took
                    int k2 = 0;
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        if (t >= nw) continue;
                        const unsigned x = rw[t] ^ s_known[t];
                        k2 += __builtin_popcount((x | (x >> 1)) & vmask(t, La));
                    }
                    known = __ballot(c && k != 0 && k2 == 0) & ~(sub1 | sub2);
                    pend3 &= ~known;   // (a known copy takes its record from the known alignment)
                    // A read of the amplicon's length closer to the known sequence (the other pass's amplicon)
                    // than to this one: a variant of it carries the amplicons' difference -- C3's 10-base HDR
                    // block, two 10-base gaps against this amplicon, more than 16 diagonals hold.  It skips
                    // the first band level (its sort key marks it; nw_band_fill<16> leaves its pair inactive,
                    // the walk hands it to the 32-diagonal level) instead of failing there first.
                    jog = __ballot(c && k2 < k && k > 3) & ~(sub1 | sub2 | known);
                }
            }
        }
        while (cand) {
            int us[kCand];
            unsigned diff[kCand], raw[kCand];
#pragma unroll
            for (int t = 0; t < kCand; ++t) {
                us[t] = cand ? (int)__builtin_ctzll(cand) : -1;
                if (cand) cand &= cand - 1;
                diff[t] = 0u;
                raw[t] = 0u;
            }
            for (int c0 = 0; c0 < nd; c0 += 64) {
                const int k4 = c0 + lane;
                // every candidate's loads issued before any is used (branch-free: a missing
                // candidate re-reads candidate 0, lanes past the read re-read its last dword)
                const int kc = k4 < nd ? k4 : nd - 1;
                uint2 w[kCand];
                int sh[kCand];
#pragma unroll
                for (int t = 0; t < kCand; ++t) {
                    const int u = us[t] < 0 ? us[0] : us[t];
                    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)my_off, u);
                    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(my_off >> 32), u);
                    const long long off = (long long)(((unsigned long long)hi << 32) | lo);
                    if constexpr (PK) {   // the read's bytes 4 kc .. 4 kc + 3 from the 2-bit stream
                        const long long q0 = off - a.pk_pos0;   // wave-uniform: 64-bit math in SGPRs
                        const unsigned tq = (unsigned)(q0 & 15) + 4u * (unsigned)kc;
                        w[t] = *(const uint2*)(a.pk_words + (q0 >> 4) + (tq >> 4));
                        sh[t] = (int)(2 * (tq & 15));
                    } else {
                        w[t] = *(const uint2*)(a.reads + (off & ~3ll) + 4 * kc);   // 4-aligned dwordx2
                        sh[t] = (int)(off & 3);
                    }
                }
                const unsigned am = k4 < nd ? amp_sh[kc] : 0u;
                const unsigned msk = k4 < nd ? (k4 == nd - 1 ? tail_mask : 0xffffffffu) : 0u;
#pragma unroll
                for (int t = 0; t < kCand; ++t) {
                    if constexpr (PK) raw[t] = pk_expand(__builtin_amdgcn_alignbit(w[t].y, w[t].x, (unsigned)sh[t]));
                    else raw[t] = __builtin_amdgcn_alignbyte(w[t].y, w[t].x, sh[t]);
                    diff[t] |= ((raw[t] | 0x20202020u) ^ am) & msk;
                }
            }
#pragma unroll
            for (int t = 0; t < kCand; ++t) {
                if (us[t] < 0) continue;
                const unsigned long long anyd = __ballot(diff[t] != 0u);
                if (anyd != 0ull) {
                    // one or two substitutions (A C G T in the read): the certificates above
                    if (!sub1_ok) continue;
                    const unsigned zd = ~zero_bytes(diff[t]) & 0x80808080u;   // the lane's mismatching bytes
                    const int nzl = __builtin_popcount(zd);
                    const unsigned long long l2 = __ballot(nzl >= 2);
                    if (__ballot(nzl >= 3) || (l2 && __builtin_popcountll(anyd) > 1) || __builtin_popcountll(anyd) > 2)
                        continue;
                    const int ksub = l2 ? 2 : (int)__builtin_popcountll(anyd);
                    if (ksub == 2 && !sub2_ok) continue;
                    const unsigned rf = raw[t] | 0x20202020u;
                    bool bad = false;
                    for (unsigned z = zd; z; z &= z - 1) {
                        const unsigned cb = (rf >> ((int)__builtin_ctz(z) - 7)) & 0xffu;
                        bad = bad || !(cb == 'a' || cb == 'c' || cb == 'g' || cb == 't');
                    }
                    if (__ballot(bad)) continue;
                    // the shifted diagonals: d = +s pairs read byte q + s with amplicon byte q, d = -s
                    // read byte q with amplicon byte q + s (q <= La - 1 - s); mismatching bytes 0x80
                    const int k4 = lane, kc = k4 < nd ? k4 : nd - 1;   // one chunk (sub1_ok)
                    const unsigned rn = (unsigned)__shfl_down((int)raw[t], 1, 64);
                    const unsigned an = k4 + 1 < nd ? amp_sh[k4 + 1] : 0u;
                    const unsigned am0 = k4 < nd ? amp_sh[kc] : 0u;
                    const int q0 = 4 * k4;   // the lane's first byte
                    auto upto = [&](int qmax) -> unsigned {   // bytes q <= qmax of the lane
                        return qmax >= q0 + 3 ? 0x80808080u : (qmax < q0 ? 0u : (0x80808080u >> (8 * (q0 + 3 - qmax))));
                    };
                    auto mis = [&](int sgn, int sh) -> unsigned {
                        const unsigned x = sgn > 0 ? (__builtin_amdgcn_alignbyte(rn, raw[t], sh) | 0x20202020u) ^ am0
                                                   : rf ^ __builtin_amdgcn_alignbyte(an, am0, sh);
                        return ~zero_bytes(x) & upto(La - 1 - sh);
                    };
                    const unsigned p1m = mis(1, 1), m1m = mis(-1, 1);
                    if (ksub == 1) {
                        // S_+-1 = m p - x (La - 1 - p) is below D exactly when p <= La - 2: one
                        // mismatch on each shifted diagonal (two ballots, no sums)
                        if (__ballot(p1m != 0u) != 0ull && __ballot(m1m != 0u) != 0ull) sub1 |= 1ull << us[t];
                        continue;
                    }
                    // two substitutions at read bytes f < l: d = +-1 need two mismatches each, one at
                    // a read byte > f (no diagonal-0 prefix + one gap + shifted suffix scores above D)
                    // and one at a read byte < l (no shifted prefix + diagonal-0 suffix); d = +-2, +-3
                    // need one (S_d < D); |d| >= 4 and two or more gaps score below D by the checks in sub2_ok
                    const unsigned long long lz = __ballot(zd != 0u);
                    const int lf = (int)__builtin_ctzll(lz), ll = 63 - (int)__builtin_clzll(lz);
                    const int zf = __builtin_amdgcn_readlane((int)zd, lf), zl = __builtin_amdgcn_readlane((int)zd, ll);
                    const int f = 4 * lf + (__builtin_ctz((unsigned)zf) >> 3), l = 4 * ll + ((31 - __builtin_clz((unsigned)zl)) >> 3);
                    auto from = [&](int qmin) -> unsigned { return 0x80808080u & ~upto(qmin - 1); };   // bytes q >= qmin
                    auto two = [&](unsigned m) {   // at least two mismatching bytes over the wave
                        const unsigned long long b1 = __ballot(m != 0u);
                        return __ballot(__builtin_popcount(m) >= 2) != 0ull || __builtin_popcountll(b1) >= 2;
                    };
                    bool ok = two(p1m) && two(m1m);
                    // d = +1: read byte j = q + 1; d = -1: j = q
                    ok = ok && __ballot((p1m & from(f)) != 0u) && __ballot((p1m & upto(l - 2)) != 0u);
                    ok = ok && __ballot((m1m & from(f + 1)) != 0u) && __ballot((m1m & upto(l - 1)) != 0u);
                    ok = ok && __ballot(mis(1, 2) != 0u) && __ballot(mis(-1, 2) != 0u) && __ballot(mis(1, 3) != 0u) &&
                         __ballot(mis(-1, 3) != 0u);
                    if (ok) sub2 |= 1ull << us[t];
                    continue;
                }
                exact |= 1ull << us[t];
                if (a.ops) continue;   // ops output: the wave's exact copies are written together below
                if (!one_chunk) {
                    emit_later |= 1ull << us[t];
                    continue;
                }
                unsigned* o = (unsigned*)(a.out + (r0 + us[t]) * 3 * a.stride);
                if (lane < nd) {
                    o[lane] = amp_sh[nd + lane];
                    o[sd + lane] = 0x7c7c7c7cu;   // '|'
                    o[2 * sd + lane] = raw[t];
                }
                if (lane < 8) {
                    // the record (nw::Stat): aln_len, n_ident, n_sim, n_gaps, score, end_i, end_j, flags
                    const int v = lane == 3 || lane == 7 ? 0 : (lane == 4 ? a.band_maxsub * La : La);
                    ((int*)(a.stats + r0 + us[t]))[lane] = v;
                }
            }
        }
        // One indel (round 6; packed input, ops output, an A C G T amplicon of at most 256 bp, no exception
        // bytes): a read of La -+ k bases, 1 <= k <= indel_kmax.  Call the shorter of read and amplicon s
        // (Ls bases), the longer l; the candidate alignment pairs every residue of s, identically, with
        // one internal gap of k residues of l: S = m Ls - O - (k - 1) E.  Any alignment pairs <= Ls
        // residues; with u of s's residues unpaired, w mismatches and g the gap residues of one internal
        // gap it scores m (Ls - u - w) - x w - O - (g - 1) E, >= S only if m u + (m + x) w <= (k - g) E:
        // u = w = 0 (m > (k - 1) E), so the gap is in l (an l-gap of g <= k: an s-gap leaves s residues
        // unpaired); two or more internal gaps score <= m Ls - 2 O < S (O > (k - 1) E).  A one-gap
        // alignment with u = w = 0 pairs a prefix of s on diagonal shift s1 (l's residue i + s1 against
        // s's i) and the rest on s2 = s1 + g, 0 <= s1 < s2 <= k: it exists iff the last mismatch of
        // shift s2 precedes the first of s1 (G[s2] <= F[s1]); every such pair but (0, k) would score
        // >= S with a different alignment: none may exist.  No internal gap: a single shift pairs
        // P = min(Ls, Ll - s) residues (shifts of s, 1..3, pair Ls - s): each score m (P - c) - x c with
        // c mismatches must stay below S (shifts pairing 4 or more residues fewer do: O + (k - 1) E <
        // 4 m).  Then the optimal alignments are exactly (0, k) with the gap at any q in [G[k], F[0]]
        // (ties), all paired residues identical; the traceback from the corner (score S, first in the
        // scan) stays on the shift-k diagonal while M ties the gap state (M wins ties) and leaves it where
        // a mismatch precedes (q = G[k]): the gap is placed left-most, X when it is in the read, else Y.
        // Runs M q, gap k, M Ls - q; identities Ls, gaps k, length Ll.  Reads of C2's deletion and
        // insertion classes (~15 % of the reads) need no DP: the traceback fill and the wide level lose
        // their bulk (tests/test_gpu_indel.py: homopolymer and tandem-repeat indels against the oracle).
        // The checks (cert_indel) run in nw_band_cert, on the queued candidates.  A shorter read may instead be
        // a window of the amplicon (below; a read one certificate takes fails the other: a window scores m Lb,
        // an alignment with an internal gap less): one whose first and last 16 bases are the amplicon's ends
        // is queued at once, the others after the window check found none.
        bool ci_win = false;   // (a candidate the window check sees first)
        if constexpr (PK) {
            const int dl = my_len - La, kab = dl < 0 ? -dl : dl;
            const bool ci = indel_kmax > 0 && a.ops && one_chunk && amp_acgt_all && r < r_end && !exc && kab >= 1 &&
                            kab <= indel_kmax;
            if (ci && dl < 0 && my_len >= 16 && La >= 16)
                ci_win = pk_word16(a, my_off) != amp2s[0] ||
                         pk_word16(a, my_off + my_len - 16) != amp_word16(amp2s, La - 16);
            pend_i = __ballot(ci && !ci_win);   // checked by nw_band_cert
        }
        // window reads (above): an exact window at the largest offset, else one substitution
        unsigned long long win = 0ull;
        int win_s = 0, win_k = 0;
        if constexpr (PK) {
            if (win_ok) {
                bool cand_w = r < r_end && !exc && my_len >= 32 && my_len < La && !((pend_i >> lane) & 1ull);
                int best1 = -1;   // -2: an exact window at win_s; >= 0: an offset with one mismatch
                if (cand_w) {
                    // a window at s has the read's first 16 bases at s or its last 16 at s + Lb - 16 (one
                    // substitution cannot hit both); the other end word must then be within one mismatch
                    // -- one word compare rejects most offsets (reads with an indel) before the middle
                    const unsigned key0 = rword(my_off), key1 = rword(my_off + my_len - 16);
                    // their offsets among the amplicon's sorted 16-mers: [f, l), the last 8 at most
                    // (repeats: the DP)
                    const unsigned kk[2] = {key0, key1};
                    int lb[2], ub[2];
                    sorted_ranges<2>(skey, nseed, kk, lb, ub);
                    const int l0 = ub[0], f0 = max(lb[0], ub[0] - 8), l1 = ub[1], f1 = max(lb[1], ub[1] - 8);
                    for (int i = l0 - 1; i >= f0; --i) {   // offsets descending: the largest exact window first
                        const int s = spos[i];
                        if (s + my_len > La) continue;
                        const int he = ham16(key1, aword(s + my_len - 16));
                        if (he > 1) continue;
                        const int mm = he + mism(my_off, 16, s + 16, my_len - 32, 1 - he);
                        if (mm == 0) {
                            best1 = -2;
                            win_s = s;
                            break;
                        }
                        if (mm == 1 && best1 == -1) best1 = s;
                    }
                    if (best1 == -1)   // the substitution among the first 16 bases
                        for (int i = l1 - 1; i >= f1; --i) {
                            const int s = (int)spos[i] - (my_len - 16);
                            if (s < 0 || ham16(key0, aword(s)) != 1) continue;
                            if (mism(my_off, 16, s + 16, my_len - 32, 0) == 0) {
                                best1 = s;
                                break;
                            }
                        }
                    if (best1 >= 0) win_s = best1;
                    win_k = best1 >= 0 ? 1 : 0;
                    cand_w = best1 != -1;
                }
                win = __ballot(cand_w);
                // one substitution: every other full-overlap diagonal needs two mismatches, the two
                // diagonals pairing Lb - 1 residues one (the whole wave on each such read)
                // (the read's 16-base words go to LDS once per candidate: the offsets' compares read them
                // there, with no global round trip per offset)
                unsigned* rbw = s_rbw[threadIdx.x >> 6];
                for (unsigned long long need = __ballot(cand_w && win_k == 1); need; need &= need - 1) {
                    const int u = (int)__builtin_ctzll(need);
                    const int s1 = __builtin_amdgcn_readlane(win_s, u), Lb = __builtin_amdgcn_readlane(my_len, u);
                    const unsigned lo32 = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)my_off, u);
                    const unsigned hi32 = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(my_off >> 32), u);
                    const long long ro = (long long)(((unsigned long long)hi32 << 32) | lo32);
                    const int nwd = (Lb + 15) / 16 + 1;   // <= kRbw
                    for (int k = lane; k < nwd; k += 64) rbw[k] = 16 * k < Lb ? rword(ro + 16 * k) : 0u;
                    lds_fence();
                    // mismatches of read bases [j0, j0 + len) against amplicon [s, s + len), up to cap + 1
                    auto mism_l = [&](int j0, int s, int len, int cap) -> int {
                        int cnt = 0;
                        for (int w = 0; w < len && cnt <= cap; w += 16) {
                            const int p = j0 + w;
                            unsigned y = __builtin_amdgcn_alignbit(rbw[(p >> 4) + 1], rbw[p >> 4], (unsigned)(2 * (p & 15))) ^
                                         aword(s + w);
                            if (len - w < 16) y &= (1u << (2 * (len - w))) - 1u;
                            cnt += __builtin_popcount((y | (y >> 1)) & 0x55555555u);
                        }
                        return cnt;
                    };
                    bool bad = false;
                    for (int s2 = lane; s2 <= La - Lb; s2 += 64)
                        if (s2 != s1) bad = bad || mism_l(0, s2, Lb, 1) < 2;
                    if (lane == 0) bad = bad || mism_l(1, 0, Lb - 1, 0) < 1;            // d = +1
                    if (lane == 1) bad = bad || mism_l(0, La - Lb + 1, Lb - 1, 0) < 1;   // d = Lb - La - 1
                    if (__ballot(bad)) win &= ~(1ull << u);
                    lds_fence();   // every lane's reads of rbw before the next candidate's writes
                }
            }
            pend_i |= __ballot(ci_win && !((win >> lane) & 1ull));   // no window: the one-indel check
        }
        // Seeded band: a read the 16-diagonal band cannot hold (La - Lb >= 16, the
        // reference's own 151 bp reads on a 280 bp amplicon) and no window certificate took: the
        // diagonals of every exact hit of its disjoint 16-base blocks among the amplicon's 16-mers.
        // The wide level then centres its band on them and certifies it (nw_band_walk).  A block
        // with more than 8 hits (a repeat) leaves the read to the exact kernel.
        int32_t sinfo = 0, sinfo2 = 0;
        if constexpr (PK) {
            if (win_ok && a.seed_info && r < r_end && !exc && my_len >= 32 && La - my_len >= 16 &&
                !(((exact | sub1 | sub2 | win | known) >> lane) & 1ull)) {
                int dmin = 1 << 20, dmax = -(1 << 20);
                bool ok = true;
                const int nb = my_len >> 4;
                // the refined certificate's facts (nw_band_walk), for reads whose blocks have at most one
                // hit each: blocks without a hit, the blocks on each hit diagonal (at most 4), the
                // cheapest move between two blocks' diagonals in read order -- an increase of d = j - i
                // by D leaves D read bases unpaired: O + (D - 1) E + m D; a decrease: O + (|D| - 1) E
                int n0 = 0, nd = 0, shift = 0xffff;
                bool uniq = true;
                int dd0 = 0, dd1 = 0, dd2 = 0, dd3 = 0, dc0 = 0, dc1 = 0, dc2 = 0, dc3 = 0;
                for (int b0 = 0; b0 < nb && ok; b0 += 8) {   // eight blocks' words in flight together
                    unsigned keys[8];
#pragma unroll
                    for (int t = 0; t < 8; ++t) keys[t] = b0 + t < nb ? rword(my_off + 16 * (b0 + t)) : 0u;
                    int lbs[8], ubs[8];   // each block's hits among the amplicon's sorted 16-mers: [lb, ub)
                    sorted_ranges<8>(skey, nseed, keys, lbs, ubs);
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        const int b = b0 + t;
                        if (b >= nb || !ok) continue;
                        const int l = ubs[t], f = lbs[t];
                        if (l - f > 8) ok = false;   // a repeat: more than 8 hits
                        for (int i = f; ok && i < l; ++i) {
                            const int d = 16 * b - (int)spos[i];
                            dmin = min(dmin, d);
                            dmax = max(dmax, d);
                        }
                        n0 += l == f;
                        uniq = uniq && l - f <= 1;
                        if (uniq && l - f == 1) {
                            const int d = 16 * b - (int)spos[f];
                            auto mv = [&](int d1) {
                                const int D = d - d1;
                                return D > 0 ? a.gap_open + (D - 1) * a.gap_extend + a.band_maxsub * D
                                             : a.gap_open + (-D - 1) * a.gap_extend;
                            };
                            const bool h0 = nd > 0 && dd0 == d, h1 = nd > 1 && dd1 == d, h2 = nd > 2 && dd2 == d,
                                       h3 = nd > 3 && dd3 == d;
                            if (nd > 0 && !h0) shift = min(shift, mv(dd0));
                            if (nd > 1 && !h1) shift = min(shift, mv(dd1));
                            if (nd > 2 && !h2) shift = min(shift, mv(dd2));
                            if (nd > 3 && !h3) shift = min(shift, mv(dd3));
                            dc0 += h0;
                            dc1 += h1;
                            dc2 += h2;
                            dc3 += h3;
                            if (!(h0 || h1 || h2 || h3)) {
                                if (nd == 0) { dd0 = d; dc0 = 1; }
                                else if (nd == 1) { dd1 = d; dc1 = 1; }
                                else if (nd == 2) { dd2 = d; dc2 = 1; }
                                else if (nd == 3) { dd3 = d; dc3 = 1; }
                                uniq = uniq && nd < 4;
                                ++nd;
                            }
                        }
                    }
                }
                if (ok && dmax >= dmin && dmax - dmin <= kWideDiags / 2 && nb < 128) {
                    sinfo = seed_pack(dmin, dmax, nb);
                    if (uniq) sinfo2 = seed2_pack(n0, max(max(dc0, dc1), max(dc2, dc3)), shift);
                }
            }
            if (a.seed_info && r < r_end) a.seed_info[r] = sinfo;
            if (a.seed_info2 && r < r_end) a.seed_info2[r] = sinfo2;
        }
        // wide first: a plain read (no exception byte, not a known sequence's variant) of another length
        // than the amplicon's, or of its length with too many substitutions for the 16-diagonal band
        const bool wf = wf_k > 0 && !exc && my_len > 0 && my_len <= a.band_lb_cap && !((jog >> lane) & 1ull) &&
                        (my_len != La || ((wf_sub >> lane) & 1ull));
        if (r < r_end)
            a.sort_key[r] = (((exact | sub1 | sub2 | win | known) >> lane) & 1ull)
                                ? a.band_lb_cap + 2
                                : (sinfo ? a.band_lb_cap + 3 +
                                               min(a.seed_keys - 1, max(0, ((seed_dmin(sinfo) + seed_dmax(sinfo)) / 2 + La) >> 2))
                                   : wf ? a.band_lb_cap + 3 + a.seed_keys + my_len
                                        : (my_len <= a.band_lb_cap && !((jog >> lane) & 1ull) ? my_len : a.band_lb_cap + 1));
        if (a.ops && r < r_end && ((win >> lane) & 1ull)) {
            // runs: s amplicon residues (Y), the window (M), the rest of the amplicon (Y)
            int q = 0;
            const long long sst = a.ops_stride;
            if (win_s > 0) a.ops[sst * q++ + r] = ((unsigned)RUN_Y << 28) | (unsigned)win_s;
            a.ops[sst * q++ + r] = ((unsigned)RUN_M << 28) | (unsigned)my_len;
            if (La - win_s - my_len > 0) a.ops[sst * q++ + r] = ((unsigned)RUN_Y << 28) | (unsigned)(La - win_s - my_len);
            a.nops[r] = q;
            int4* st = (int4*)(a.stats + r);
            st[0] = make_int4(La, my_len - win_k, my_len - win_k, La - my_len);   // aln_len, n_ident, n_sim, n_gaps
            st[1] = make_int4(a.band_maxsub * (my_len - win_k) - win_k * 4 * sc5, win_s + my_len, my_len, 0);
        }
        // a known copy: record and runs from the known alignment, by the compaction
        if (a.ops && r < r_end && ((known >> lane) & 1ull)) a.nops[r] = kNopsKnown;
        // ops output: every exact copy of the wave's 64 reads at once, lane u its own read's
        // record (2 x 16 B), its one M run of La columns (run 0 of its slot) and run count --
        // coalesced stores instead of three partial-line stores per copy
        if (a.ops && r < r_end && (((exact | sub1 | sub2) >> lane) & 1ull)) {
            // substitutions (0 .. 2; three: nw_band_cert; a mismatch scores -4 / 5 maxsub)
            const int k = (int)((sub1 >> lane) & 1ull) + 2 * (int)((sub2 >> lane) & 1ull);
            a.ops[r] = ((unsigned)RUN_M << 28) | (unsigned)La;
            a.nops[r] = 1;
            int4* st = (int4*)(a.stats + r);
            st[0] = make_int4(La, La - k, La - k, 0);   // aln_len, n_ident, n_sim, n_gaps
            st[1] = make_int4(a.band_maxsub * (La - k) - k * 4 * sc5, La, La, 0);   // score, end_i, end_j, flags
        }
        // the diagonal of every exact copy longer than one chunk: amplicon, '|' markup,
        // read; rows as dwords up to round4(La) (within the row stride)
        while (emit_later) {
            const int u = (int)__builtin_ctzll(emit_later);
            emit_later &= emit_later - 1;
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)my_off, u);
            const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(my_off >> 32), u);
            const long long off = (long long)(((unsigned long long)hi << 32) | lo);
            const uint8_t* base = a.reads + (off & ~3ll);
            unsigned* o = (unsigned*)(a.out + (r0 + u) * 3 * a.stride);
            for (int k4 = lane; k4 < nd; k4 += 64) {
                o[k4] = amp_sh[nd + k4];
                o[sd + k4] = 0x7c7c7c7cu;   // '|'
                o[2 * sd + k4] = __builtin_amdgcn_alignbyte(ld_dw(base + 4 * k4 + 4), ld_dw(base + 4 * k4), (int)(off & 3));
            }
            if (lane < 8) {
                // the record (nw::Stat): aln_len, n_ident, n_sim, n_gaps, score, end_i, end_j, flags
                const int v[8] = {La, La, La, 0, a.band_maxsub * La, La, La, 0};
                int x = 0;
#pragma unroll
                for (int t = 0; t < 8; ++t) x = lane == t ? v[t] : x;
                ((int*)(a.stats + r0 + u))[lane] = x;
            }
        }
        // packed input: the bytes of every read that needs the DP (the only reads a later kernel
        // reads), exactly its own bytes, each stored once as its final value, exception bytes included
        // (write_read_bytes: within a pass no other wave writes them; the other pass of a dual call
        // stores the same values)
        if constexpr (PK)
            write_read_bytes(a, __ballot(r < r_end && my_len > 0 &&
                                         !(((exact | sub1 | sub2 | win | known | pend3 | pend_i) >> lane) & 1ull)),
                             my_off, my_len, __ballot(exc), x0, x1);
        // deferred certificates (KernelArgs::cert_q): the wavefront's queued reads for nw_band_cert, the
        // three-substitution candidates from the front of its 64 entries, the one-indel ones from the back
        if constexpr (PK) {
            if (a.cert_q) {
                const unsigned long long lt = (1ull << lane) - 1ull;
                const long long slot = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
                if ((pend3 >> lane) & 1ull) a.cert_q[slot * 64 + __builtin_popcountll(pend3 & lt)] = (int32_t)r;
                if ((pend_i >> lane) & 1ull) a.cert_q[slot * 64 + 63 - __builtin_popcountll(pend_i & lt)] = (int32_t)r;
                if (lane == 0) a.cert_cnt[slot] = (int32_t)(__builtin_popcountll(pend3) | (__builtin_popcountll(pend_i) << 8));
            }
        }
    };
    if constexpr (!PK) {
        // wavefront batches of 64 reads, grid-strided
        for (long long r0 = ((long long)blockIdx.x * wpb + (threadIdx.x >> 6)) * 64; r0 < a.n;
             r0 += (long long)gridDim.x * wpb * 64) {
            const long long r = r0 + lane;
            const long long my_off = r < a.n ? a.offsets[r] : 0;
            const int my_len = r < a.n ? (int)(a.offsets[r + 1] - my_off) : -1;
            batch(r0, a.n, my_off, my_len, false, 0, 0);
        }
    } else {
        __shared__ long long s_off[kPkBlock + 1];
        __shared__ unsigned char s_exc[kPkBlock];
        __shared__ long long s_wsum[8];
        __shared__ long long s_x[2];
        const long long bl = pbl, bh = pbh;
        const int cnt = (int)(bh - bl), tid = threadIdx.x, wave = tid >> 6;
        int64_t* offs = const_cast<int64_t*>(a.offsets);
        if (a.pk_len) {
            // the offsets from the lengths (nw_align_ops_packed_lens): the group's base offset, the
            // lengths of the group's reads before this block (earlier chunks' included: they are uploaded
            // with the call's first lengths copy), an exclusive scan of the block's own
            const long long G = pG, rr = prr, l = pk_l;
            long long pre = pk_pre;
            long long inc = l;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const long long o = __shfl_up(inc, d, 64);
                const long long op = __shfl_xor(pre, d, 64);
                if (lane >= d) inc += o;
                pre += op;
            }
            if (lane == 63) s_wsum[wave] = inc;
            if (lane == 0) s_wsum[4 + wave] = pre;
            __syncthreads();
            long long o = a.pk_gbase[G] + inc - l + s_wsum[4] + s_wsum[5] + s_wsum[6] + s_wsum[7];
            for (int w2 = 0; w2 < wave; ++w2) o += s_wsum[w2];
            if (rr >= bl && rr < bh) {
                s_off[rr - bl] = o;
                offs[rr] = o;
            }
            if (rr == bh - 1) {   // the end of the block's last read (the chunk's last: offsets[n])
                s_off[cnt] = o + l;
                offs[bh] = o + l;
            }
        } else {
            for (int i = tid; i <= cnt; i += blockDim.x) s_off[i] = a.offsets[bl + i];
        }
        // reads holding exception bytes (not certifiable here; every one of them needs the DP)
        const bool any_exc = a.pk_e1 > a.pk_e0;
        for (int i = tid; i < kPkBlock; i += blockDim.x) s_exc[i] = 0;
        __syncthreads();
        long long x0 = 0, x1 = 0;
        if (any_exc) {
            if (wave == 0) {
                const long long lo_b = exc_lower_bound(a, s_off[0], lane);
                const long long hi_b = exc_lower_bound(a, s_off[cnt], lane);
                if (lane == 0) {
                    s_x[0] = lo_b;
                    s_x[1] = hi_b;
                }
            }
            __syncthreads();
            x0 = s_x[0];
            x1 = s_x[1];
            for (long long t = x0 + tid; t < x1; t += blockDim.x) {
                const long long p = a.pk_exc_pos[t];
                int lo_i = 0, hi_i = cnt - 1;   // the last read starting at or before p
                while (lo_i < hi_i) {
                    const int mid = (lo_i + hi_i + 1) >> 1;
                    if (s_off[mid] <= p) lo_i = mid;
                    else hi_i = mid - 1;
                }
                s_exc[lo_i] = 1;
            }
            __syncthreads();
        }
        const long long r0 = bl + 64 * wave;   // one batch per wavefront
        if (r0 < bh) {
            const long long r = r0 + lane;
            const long long my_off = r < bh ? s_off[r - bl] : 0;
            const int my_len = r < bh ? (int)(s_off[r - bl + 1] - my_off) : -1;
            batch(r0, bh, my_off, my_len, r < bh && s_exc[r - bl] != 0, x0, x1);
        } else if (a.cert_q && lane == 0) {
            a.cert_cnt[(long long)blockIdx.x * 4 + wave] = 0;   // (every wavefront's queue count is written)
        }
        // (every exception byte is in a flagged read, flagged reads all need the DP, and their bytes went
        // out with the exceptions in place: no store of a decoded 'A' that a later one would correct)
    }
}

// ============================================================================
// Deferred certificates (KernelArgs::cert_q), between classify and the sort.  In classify each
// wavefront runs a check for all its 64 lanes when any lane needs it: the three-substitution and
// one-indel checks cost ~70 us of a 1M-read C2 pass there, for the ~20 % of reads that take them.
// Classify queues those reads instead (per wavefront: three-substitution candidates from the front of
// its 64 entries, one-indel candidates from the back, the two counts in cert_cnt) with the DP's sort
// key and no bytes; here one block gathers the queues of kCertSlots classify wavefronts into two dense
// lists in LDS and its wavefronts run the same checks (cert_sub3, cert_indel) 64 reads at a time.  A
// certified read gets its record, runs and the finished key; the others get their bytes for the DP.
// ============================================================================
constexpr int kCertSlots = 16;   // classify wavefronts per block (4 classify blocks)

// ONEPASS: cert_indel's form (KernelArgs::indel_onepass)
template <bool ONEPASS>
__global__ __launch_bounds__(256) void nw_band_cert(const KernelArgs a, int nslots) {
    extern __shared__ unsigned c_amp2[];   // the amplicon's 2-bit words (classify's image from 2 nd)
    __shared__ int s_n3[kCertSlots], s_ni[kCertSlots], s_o3[kCertSlots + 1], s_oi[kCertSlots + 1];
    __shared__ int s_l3[kCertSlots * 64], s_li[kCertSlots * 64];
    __shared__ unsigned s_fact[4][kSub3FactWords];   // cert_sub3's per-wavefront facts
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long slot0 = (long long)blockIdx.x * kCertSlots;
    const int ns = (int)min<long long>(kCertSlots, nslots - slot0);
    if (tid < kCertSlots) {
        const int v = tid < ns ? a.cert_cnt[slot0 + tid] : 0;
        s_n3[tid] = v & 0xff;
        s_ni[tid] = v >> 8;
    }
    __syncthreads();
    if (tid == 0) {
        int x = 0, y = 0;
        for (int i = 0; i < kCertSlots; ++i) {
            s_o3[i] = x;
            s_oi[i] = y;
            x += s_n3[i];
            y += s_ni[i];
        }
        s_o3[kCertSlots] = x;
        s_oi[kCertSlots] = y;
    }
    __syncthreads();
    const int n3 = s_o3[kCertSlots], ni = s_oi[kCertSlots];
    if (n3 + ni == 0) return;   // (block-uniform)
    const int La = a.La, nd = (La + 3) / 4, n2 = (La + 15) / 16 + 2;
    for (int k = tid; k < n2; k += 256) c_amp2[k] = a.cls_img[2 * nd + k];
    for (int p = tid; p < ns * 64; p += 256) {
        const int sl = p >> 6, j = p & 63;
        if (j < s_n3[sl]) s_l3[s_o3[sl] + j] = a.cert_q[(slot0 + sl) * 64 + j];
        else if (j >= 64 - s_ni[sl]) s_li[s_oi[sl] + 63 - j] = a.cert_q[(slot0 + sl) * 64 + j];
    }
    __syncthreads();
    const int sc5 = a.band_maxsub / 5;
    const long long sst = a.ops_stride;
    // three substitutions: reads of the amplicon's length, three mismatches on the main diagonal
    for (int b = 64 * wave; b < n3; b += 256) {
        const bool v = b + lane < n3;
        const long long r = v ? s_l3[b + lane] : 0;
        const long long my_off = v ? a.offsets[r] : a.pk_pos0;
        unsigned rw[17];
        load_read_words(a, v, my_off, rw);
        int k, f, f2, l;
        main_diag_mism(rw, c_amp2, La, &k, &f, &f2, &l);
        const bool ok = cert_sub3(a, c_amp2, rw, v && k == 3, f, f2, l, my_off, s_fact[wave]);
        if (ok) {   // the diagonal with three substitutions (classify's record for them)
            a.ops[r] = ((unsigned)RUN_M << 28) | (unsigned)La;
            a.nops[r] = 1;
            int4* st = (int4*)(a.stats + r);
            st[0] = make_int4(La, La - 3, La - 3, 0);   // aln_len, n_ident, n_sim, n_gaps
            st[1] = make_int4(a.band_maxsub * (La - 3) - 3 * 4 * sc5, La, La, 0);   // score, end_i, end_j, flags
            a.sort_key[r] = a.band_lb_cap + 2;
        }
        write_read_bytes(a, __ballot(v && !ok), my_off, La);
    }
    // one indel: reads of La -+ k bases
    for (int b = 64 * wave; b < ni; b += 256) {
        const bool v = b + lane < ni;
        const long long r = v ? s_li[b + lane] : 0;
        const long long my_off = v ? a.offsets[r] : a.pk_pos0;
        const int my_len = v ? (int)(a.offsets[r + 1] - my_off) : La;
        int gk = 0;
        const bool ok = cert_indel<ONEPASS>(a, c_amp2, v, my_off, my_len, &gk);
        if (ok) {   // runs M q, the gap (X: residues of the read, Y: of the amplicon), M the rest of the shorter
            const bool del = my_len < La;
            const int Ls = del ? my_len : La, kab = del ? La - my_len : my_len - La;
            a.ops[r] = ((unsigned)RUN_M << 28) | (unsigned)gk;
            a.ops[sst + r] = ((unsigned)(del ? RUN_Y : RUN_X) << 28) | (unsigned)kab;
            a.ops[2 * sst + r] = ((unsigned)RUN_M << 28) | (unsigned)(Ls - gk);
            a.nops[r] = 3;
            int4* st = (int4*)(a.stats + r);
            st[0] = make_int4(Ls + kab, Ls, Ls, kab);   // aln_len, n_ident, n_sim, n_gaps
            st[1] = make_int4(a.band_maxsub * Ls - a.gap_open - (kab - 1) * a.gap_extend, La, my_len, 0);
            a.sort_key[r] = a.band_lb_cap + 2;
        }
        write_read_bytes(a, __ballot(v && !ok), my_off, my_len);
    }
}

// classify (exact copies, sort keys), then the deferred certificates (launch_band_sort: the sort follows)
void launch_band_classify(const KernelArgs& a, hipStream_t s) {
    if (a.pk_words) {   // one block per call block of 256 reads the chunk touches
        const int64_t g0 = a.pk_call_lo / 256, g1 = (a.pk_call_lo + a.n - 1) / 256;
        const size_t lds = (size_t)(8 * ((a.La + 3) / 4)) +
                           (a.amp2 ? (size_t)(4 * ((a.La + 15) / 16 + 2) + 6 * a.n_seed + 16) : 0) +
                           (size_t)(4 * a.sub12_words);
        // (the table form: where the lane path runs -- ops output, the image holds the tables)
        if (a.sub12_table && a.sub12_words > 0 && a.ops && a.amp2 && a.amp_acgt)
            hipLaunchKernelGGL((nw_band_classify<true, true>), dim3((unsigned)(g1 - g0 + 1)), dim3(256), lds, s, a);
        else
            hipLaunchKernelGGL((nw_band_classify<true, false>), dim3((unsigned)(g1 - g0 + 1)), dim3(256), lds, s, a);
        if (a.cert_q) {   // its four wavefronts' queues per block
            const int nslots = (int)(4 * (g1 - g0 + 1));
            const dim3 grid((unsigned)((nslots + kCertSlots - 1) / kCertSlots));
            const size_t clds = (size_t)(4 * ((a.La + 15) / 16 + 2));
            if (a.indel_onepass) hipLaunchKernelGGL(nw_band_cert<true>, grid, dim3(256), clds, s, a, nslots);
            else hipLaunchKernelGGL(nw_band_cert<false>, grid, dim3(256), clds, s, a, nslots);
        }
    } else {
        hipLaunchKernelGGL(nw_band_classify<false>, dim3(std::max(1, std::min(2048, (int)((a.n + 255) / 256)))),
                           dim3(256), (size_t)(8 * ((a.La + 3) / 4)), s, a);
    }
}

}  // namespace nw
