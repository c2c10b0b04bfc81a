// nw_band_fill.hip -- nw_band_fill: a band level's sweep over its list's read pairs, the
// traceback bits and captures into each pair's region (nw_band_device.h: the band and the
// region's layout); the regions' host-side geometry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "nw_band_device.h"

namespace nw {

namespace {

__device__ __forceinline__ unsigned and_or(unsigned a, unsigned m, unsigned c) {
    unsigned d;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(m), "v"(c));
    return d;
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) { return ~wave_max_u32(~v); }

}  // namespace

// ============================================================================
// Fill
// ============================================================================
// The traceback fill: a level's band list, its traceback bits into each pair's region (the walk
// follows).  (Round 6 removed the diagonal pass, a score-only fill over the reads of the
// amplicon's length ahead of this one: with the classify certificates taking nearly all of them,
// its sweep only lengthened the chain -- resident pass 0.536 -> 0.484 ms without it)
template <int W, bool SUMM = false>   // SUMM: the traceback fill also writes the stop summary (lane walk)
#define NW_FILL_WPE 6   // 5: no spills in the traceback fill but slower
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(NW_FILL_WPE))) void nw_band_fill(const KernelArgs a) {
    using G = BandGeo<W>;
    constexpr int kBL = G::L, kBPW = G::PW, kCapBytes = G::CapBytes;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // second level skipped: its reads go to the wide level (with the seeded list: that list alone)
    if (W == kBandDiags && redo_direct_taken(a) && a.seed_l2 != 1) return;
    if (W < kBandDiags && l1_skipped(a)) return;   // first level skipped (KernelArgs::l1_skip)
    if (W >= kBandDiags && a.tail_prio) __builtin_amdgcn_s_setprio(3);
    // beside a wide-first launch (raised priority, as every wide launch): the same, or its wavefronts wait for that one's
    if (W < kBandDiags && a.wf_list && a.tail_prio) __builtin_amdgcn_s_setprio(3);
    if (W > kBandDiags && a.wf_take == 1 && blockIdx.x == 0 && threadIdx.x == 0 && wf_taken(a)) *a.wf_taken_n = *a.wf_count;
    const int La = a.La;
    const int O = a.gap_open, E = a.gap_extend;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wpb = blockDim.x >> 6;
    const int q = G::q_of(lane), grp = G::grp_of(lane);
    const unsigned NEG2 = 0u;                    // -inf in the kBias16 domain
    const unsigned OE2 = pk(O - E, O - E);

    uint32_t* tab = (uint32_t*)smem;
    uint16_t* acd = (uint16_t*)(smem + kTabBytes);
    const int PCS = band_pcs(La, W);
    unsigned char* pcd_wave = smem + kTabBytes + align16(2 * band_acd_elems(La)) + wave * kBPW * PCS;
    unsigned char* pcd = pcd_wave + grp * PCS;
    unsigned char* lut6 = smem + kTabBytes + align16(2 * band_acd_elems(La)) + wpb * kBPW * PCS;
    // a tile row's four words per lane wait here (not in VGPRs) until its dwordx4 store
    unsigned* stage = (unsigned*)(lut6 + 256) + wave * 256 + 4 * lane;
    for (int k = tid; k < kTabRows * 36; k += blockDim.x) tab[k] = a.band_tab[k];
    for (int k = tid; k < 256; k += blockDim.x) lut6[k] = a.lut6[k];
    for (int k = tid; k < band_acd_elems(La); k += blockDim.x) {
        const int i = k - kAPad;   // row i = amplicon residue i - 1
        // the amplicon's EDNAFULL code (IUPAC codes included: their row of the table), pad outside
        const int c = (i >= 1 && i <= La) ? a.lut[a.amp[i - 1]] : NCODE_PAD;
        // the score table's LDS address is folded in: a0 + j0 is the entry's LDS address
        acd[k] = (uint16_t)(c * 36 * 4 + (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)tab);
    }
    __syncthreads();

    // byte-plane masks of the sign bits (SGPRs: v_and_or_b32 takes no literal)
    unsigned mT[4], mU[4];
    asm volatile("s_mov_b32 %0, 0x01010101" : "=s"(mT[0]));
    asm volatile("s_mov_b32 %0, 0x02020202" : "=s"(mT[1]));
    asm volatile("s_mov_b32 %0, 0x04040404" : "=s"(mT[2]));
    asm volatile("s_mov_b32 %0, 0x08080808" : "=s"(mT[3]));
    asm volatile("s_mov_b32 %0, 0x10101010" : "=s"(mU[0]));
    asm volatile("s_mov_b32 %0, 0x20202020" : "=s"(mU[1]));
    asm volatile("s_mov_b32 %0, 0x40404040" : "=s"(mU[2]));
    asm volatile("s_mov_b32 %0, 0x80808080" : "=s"(mU[3]));

    // the band list: wave work items of kBPW pairs each
    const int NW = a.band_words;
    const long long nb = (long long)*a.band_count;
    const long long count = band_list_count(a);
    const long long pair_lo = a.band_pair_lo;
    const long long pair_hi = min(a.band_pair_hi, (count + 1) / 2);
    const long long npB = pair_hi - pair_lo;
    const long long nB = npB > 0 ? (npB + kBPW - 1) / kBPW : 0ll;
    auto body = [&](long long wv) __attribute__((always_inline)) {
        const long long g = pair_lo + wv * kBPW + grp;
        int dlo = 0;
        bool act = false;
        long long offA = 0, offB = 0, ra = 0, rb = 0;
        int LbA = 0, LbB = 0;
        bool seeded = false;
        if (g < pair_hi) {
            ra = band_list_read(a, 2 * g, nb);
            rb = (2 * g + 1 < count) ? band_list_read(a, 2 * g + 1, nb) : ra;
            offA = a.offsets[ra];
            offB = a.offsets[rb];
            LbA = (int)(a.offsets[ra + 1] - offA);
            LbB = (int)(a.offsets[rb + 1] - offB);
            act = LbA <= a.band_lb_cap && LbB <= a.band_lb_cap && band_geometry2(La, LbA, LbB, &dlo, W);
            // the first level (16 diagonals) leaves a pair with a read classify keyed past the band's lengths
            // -- one that needs more diagonals (a known sequence's variant: nw_band_classify) -- to the next
            // (a wide-first read on this level -- its list was not taken -- is an ordinary read of its length)
            if constexpr (W < kBandDiags) {
                const int kw = a.wf_list ? a.band_lb_cap + 3 + a.seed_keys : 0x7fffffff;
                const int ka = a.sort_key[ra], kb = a.sort_key[rb];
                act = act && (ka <= a.band_lb_cap || ka >= kw) && (kb <= a.band_lb_cap || kb >= kw);
            }
            if constexpr (W >= kBandDiags) {
                // seeded reads (both of the pair): the band centred on their hits' diagonals
                if (a.seed_info) {
                    const int32_t sa = a.seed_info[ra], sb = a.seed_info[rb];
                    const int lo = min(seed_dmin(sa), seed_dmin(sb)), hi = max(seed_dmax(sa), seed_dmax(sb));
                    const int sdlo = lo - (W - (hi - lo + 1)) / 2;
                    // the second level's LDS code pads hold columns j >= -(kJPad - 1) and rows i < La + 112
                    // (the sweep's first and last steps): narrower than the wide level's
                    const bool pads_ok = W > kBandDiags || (sdlo >= -2 * (kJPad - 3) && max(LbA, LbB) - sdlo < La + 200);
                    if (seed_valid(sa) && seed_valid(sb) && hi - lo + 1 <= W - 2 && LbA <= a.band_lb_cap &&
                        LbB <= a.band_lb_cap && sdlo <= kBK && sdlo + W - 1 >= 1 - La && pads_ok) {
                        dlo = sdlo;   // (tau = t - dlo + kBK stays >= 0)
                        act = true;
                        seeded = true;
                    }
                }
            }
        }
        if (!act) {   // neutral geometry, nothing stored
            band_geometry2(La, La, La, &dlo, W);
            LbA = LbB = 0;
        }
        const int Lmax = max(LbA, LbB);

        // pair codes of the wavefront's pairs' columns (j = 1..Lb real, the rest pad):
        // all 64 lanes stage one pair at a time, 4 columns per lane from coalesced dword
        // loads of both reads (all pairs' loads issued before any is used)
        for (int k4 = lane; k4 < kBPW * PCS / 4; k4 += 64) ((unsigned*)pcd_wave)[k4] = 0x8c8c8c8cu;   // pad pair
        const int Lw = (int)wave_max_u32((unsigned)Lmax);
        unsigned bad_mask = 0u;   // bit p: pair p has a read A / B code outside A C G T N (bits 0-15 / 16-31)
        unsigned pad_mask = 0u;   // the same for bytes EDNAFULL does not score ('-', '*', ...: the walk's gap columns)
        unsigned n_mask = 0u;     // the same for N
        constexpr int kSub = kBPW < 4 ? kBPW : 4;   // pairs staged together (loads in flight)
        for (int c0 = 0; c0 < Lw; c0 += 256)
        for (int p0 = 0; p0 < kBPW; p0 += kSub) {
            const int k4 = (c0 >> 2) + lane;
            unsigned wA[kSub], wB[kSub];
            int lenA[kSub], lenB[kSub];
#pragma unroll
            for (int pp = 0; pp < kSub; ++pp) {
                const int p = p0 + pp;
                const int src = G::src_of(p);   // lane q = 0 of pair p
                const unsigned oAl = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)offA, src);
                const unsigned oAh = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(offA >> 32), src);
                const unsigned oBl = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)offB, src);
                const unsigned oBh = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(offB >> 32), src);
                lenA[pp] = __builtin_amdgcn_readlane(LbA, src);
                lenB[pp] = __builtin_amdgcn_readlane(LbB, src);
                const long long oA = (long long)(((unsigned long long)oAh << 32) | oAl);
                const long long oB = (long long)(((unsigned long long)oBh << 32) | oBl);
                wA[pp] = wB[pp] = 0u;
                if (4 * k4 < lenA[pp]) {
                    const uint8_t* b = a.reads + (oA & ~3ll) + 4 * k4;
                    wA[pp] = __builtin_amdgcn_alignbyte(*(const unsigned*)(b + 4), *(const unsigned*)b, (int)(oA & 3));
                }
                if (4 * k4 < lenB[pp]) {
                    const uint8_t* b = a.reads + (oB & ~3ll) + 4 * k4;
                    wB[pp] = __builtin_amdgcn_alignbyte(*(const unsigned*)(b + 4), *(const unsigned*)b, (int)(oB & 3));
                }
            }
#pragma unroll
            for (int pp = 0; pp < kSub; ++pp) {
                const int p = p0 + pp;
                const int Lm = max(lenA[pp], lenB[pp]);
                bool bA = false, bB = false, zA = false, zB = false, nnA = false, nnB = false;
                if (4 * k4 < Lm) {
                    unsigned packed = 0u;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int j0 = 4 * k4 + b;   // 0-based column
                        int cA = j0 < lenA[pp] ? lut6[(wA[pp] >> (8 * b)) & 0xffu] : kPadCode;
                        int cB = j0 < lenB[pp] ? lut6[(wB[pp] >> (8 * b)) & 0xffu] : kPadCode;
                        // lut6: 5 = pad / not in EDNAFULL (scores 0, as EMBOSS does); 6 = IUPAC code
                        bA = bA || cA > kPadCode;
                        bB = bB || cB > kPadCode;
                        zA = zA || (j0 < lenA[pp] && cA == kPadCode);
                        zB = zB || (j0 < lenB[pp] && cB == kPadCode);
                        nnA = nnA || (j0 < lenA[pp] && cA == 4);   // N
                        nnB = nnB || (j0 < lenB[pp] && cB == 4);
                        cA = min(cA, kPadCode);
                        cB = min(cB, kPadCode);
                        packed |= (unsigned)((cA * 6 + cB) * 4) << (8 * b);
                    }
                    *(unsigned*)(pcd_wave + p * PCS + kJPad + 1 + 4 * k4) = packed;
                }
                // ballots with every lane active: bad_mask must be the same in all lanes
                // (pair p's header is written by its own q = 0 lane)
                if (__ballot(bA)) bad_mask |= 1u << p;
                if (__ballot(bB)) bad_mask |= 1u << (16 + p);
                if (__ballot(zA)) pad_mask |= 1u << p;
                if (__ballot(zB)) pad_mask |= 1u << (16 + p);
                if (__ballot(nnA)) n_mask |= 1u << p;
                if (__ballot(nnB)) n_mask |= 1u << (16 + p);
            }
        }
        const unsigned npm = n_mask | pad_mask;   // N, or a byte EDNAFULL does not score (the walk's plain reads have neither)
        const int flags = (((bad_mask >> grp) & 1u) ? REGION_BAD_A : 0) | (((bad_mask >> (16 + grp)) & 1u) ? REGION_BAD_B : 0) |
                          (((npm >> grp) & 1u) ? REGION_NP_A : 0) | (((npm >> (16 + grp)) & 1u) ? REGION_NP_B : 0);

        // wave-uniform tau range; per lane: boundary and capture steps
        const unsigned tlo = act ? (unsigned)(kBK - dlo) : 0xffffffffu;
        const unsigned thi = act ? (unsigned)(kBK - dlo + La + Lmax) : 0u;
        const unsigned dmax = (unsigned)(-dlo > dlo + W - 1 ? -dlo : dlo + W - 1);
        const unsigned tpro = act ? (unsigned)(kBK - dlo) + dmax + 1 : 0u;
        const int tau0 = (int)(wave_min_u32(tlo) & ~3u);
        const int tau_end = (int)wave_max_u32(thi);
        const int tau_pro = (int)wave_max_u32(tpro);
        lds_fence();
        unsigned char* region = a.band_region + (g - pair_lo) * a.band_stride;
        if (q == 0 && g < pair_hi) {
            // everything the walk needs to find the pair's reads: one 48-byte load
            int4* hp = (int4*)region;
            hp[0] = make_int4(tau0, dlo, flags | (act ? 0 : kPairInactive) | (seeded ? REGION_SEEDED : 0), 0);
            hp[1] = make_int4((int)ra, (int)rb, (int)(a.offsets[ra + 1] - offA), (int)(a.offsets[rb + 1] - offB));
            hp[2] = make_int4((int)(unsigned)offA, (int)(offA >> 32), (int)(unsigned)offB, (int)(offB >> 32));
        }
        if (tau_end == 0) return;   // no active group in this wavefront

        const int d0 = dlo + 2 * q;
        int tb[2], te[2], teB[2];
        unsigned bval[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int d = d0 + p;
            const int ad = d < 0 ? -d : d;
            tb[p] = kBK - dlo + ad;
            bval[p] = pk(E * ad + kBias16, E * ad + kBias16);
            const int ilo = 1 - d > 1 ? 1 - d : 1;
            // step at which diagonal d reaches read A's / read B's last row or column
            const int ieA = La < LbA - d ? La : LbA - d, ieB = La < LbB - d ? La : LbB - d;
            te[p] = (LbA > 0 && ieA >= ilo) ? kBK - dlo + 2 * ieA + d : -1;
            teB[p] = (LbB > 0 && ieB >= ilo) ? kBK - dlo + 2 * ieB + d : -1;
        }
        // capture window: the steps at which some lane's diagonal reaches the last row
        // or column; blocks before it skip the capture selects
        const int te_lo = (int)wave_min_u32(min(min((unsigned)te[0], (unsigned)te[1]),
                                                min((unsigned)teB[0], (unsigned)teB[1])));
        unsigned* bits = (unsigned*)(region + kHdrBytes + kCapBytes) + 4 * q;   // this lane's slot of each tile
        // the stop summary (band_summ): the OR of a 16-word block's words (accumulated in LDS at each
        // row's store, next to the row's stage), one byte per block, gathered in LDS 16 blocks at a
        // time and stored as one 16-byte line piece per lane (byte stores spread over the pass had
        // cost +0.12 GB of partial-line writes)
        constexpr bool summ_on = SUMM;
        unsigned* sum_lds = (unsigned*)(lut6 + 256) + wpb * 256 + wave * 320 + lane;   // the block's OR
        unsigned* sum_chunk = (unsigned*)(lut6 + 256) + wpb * 256 + wave * 320 + 64 + 4 * lane;   // 16 blocks' bytes
        if (summ_on) {
            *sum_lds = 0u;
            *(uint4*)sum_chunk = make_uint4(0u, 0u, 0u, 0u);
        }
        auto summ_flush = [&](int b) {   // the chunk holding block b, to the pair's summary
            unsigned char* sp = (unsigned char*)(bits - 4 * q) + (size_t)NW * (W / 2) * 4 + q * band_summ_bytes(NW);
            *(uint4*)(sp + (b & ~15)) = *(const uint4*)sum_chunk;
            *(uint4*)sum_chunk = make_uint4(0u, 0u, 0u, 0u);
        };
        auto summ_put = [&](int b, unsigned x) {   // block b's byte; the chunk goes out with its last block
            ((unsigned char*)sum_chunk)[b & 15] = (unsigned char)(((x >> 20) & 0xfu) | (((x >> 28) & 0xfu) << 4));
            if ((b & 15) == 15) summ_flush(b);
        };

        unsigned Hp0 = pk(kBias16, kBias16), Hp1 = Hp0, MoP = NEG2, XP = NEG2, YP = NEG2;
        unsigned cap0 = NEG2, cap1 = NEG2, capB0 = NEG2, capB1 = NEG2;   // read A's (low) / B's (high half)
        // LDS code cursors of the block starting at tau4: rows i0, i0 + 1; columns j0 .. j0 + 2
        auto ibase = [&](int tau4) { return (tau4 - kBK) / 2 - q; };
        const uint16_t* ap = acd + kAPad + ibase(tau0);
        const unsigned char* jp = pcd + kJPad + (ibase(tau0) + dlo + 2 * q);
        auto load_scores = [&](unsigned* s) {
            const int a0 = ap[0], a1 = ap[1];
            const int j0 = jp[0], j1 = jp[1], j2 = jp[2];
            using LdsU = const __attribute__((address_space(3))) unsigned;
            s[0] = *(LdsU*)(uintptr_t)(a0 + j0);
            s[1] = *(LdsU*)(uintptr_t)(a0 + j1);
            s[2] = *(LdsU*)(uintptr_t)(a1 + j1);
            s[3] = *(LdsU*)(uintptr_t)(a1 + j2);
            ap += 2;   // rows and columns both advance by 2 per 4 steps
            jp += 2;
        };
        unsigned sc[4], sn[4];
        load_scores(sc);

        auto step = [&](int tau, auto Uc, auto PROc, auto CAPc, const unsigned* scr, unsigned& acc) {
            constexpr int U = decltype(Uc)::value;
            constexpr int P = U & 1;
            constexpr bool PRO = decltype(PROc)::value;
            constexpr bool CAP = decltype(CAPc)::value;
            unsigned X, Y, d1 = 0u, d2 = 0u;
            if constexpr (P == 0) {
                // up = own diagonal d0 + 1 one step back; left = lane q-1's d0 - 1
                const unsigned Ml = G::shr(MoP), Xl = G::shr(XP);
                X = max2(Ml, Xl);
                d2 = sub2(Xl, Ml);     // sign: X opens (open > extend)
                Y = max2(MoP, YP);
                d1 = sub2(YP, MoP);    // sign: Y opens
            } else {
                // up = lane q+1's d0 one step back; left = own diagonal d0
                const unsigned Mu = G::shl(MoP), Yu = G::shl(YP);
                Y = max2(Mu, Yu);
                d1 = sub2(Yu, Mu);
                X = max2(MoP, XP);
                d2 = sub2(XP, MoP);
            }
            unsigned M = add2(P ? Hp1 : Hp0, scr[U]);
            const unsigned mxy = max2(X, Y);
            unsigned H = max2(M, mxy);
            if constexpr (PRO) {
                if (tau == tb[P]) {   // DP boundary cell (row 0 / column 0): M = 0, X = Y = -inf
                    M = bval[P];
                    H = M;
                    X = NEG2;
                    Y = NEG2;
                }
            }
            if constexpr (P == 0) Hp0 = H; else Hp1 = H;
            MoP = sub2(M, OE2);
            XP = X;
            YP = Y;
            if constexpr (CAP) {
                if constexpr (P == 0) {
                    cap0 = tau == te[0] ? M : cap0;
                    capB0 = tau == teB[0] ? M : capB0;
                } else {
                    cap1 = tau == te[1] ? M : cap1;
                    capB1 = tau == teB[1] ? M : capB1;
                }
            }
            const unsigned d3 = sub2(X, Y);     // sign: Y > X (X wins an X == Y tie)
            const unsigned d4 = sub2(M, mxy);   // sign: M < max(X, Y)
            const unsigned tt = __builtin_amdgcn_perm(d2, d1, 0x0B0A0908u);
            const unsigned uu = __builtin_amdgcn_perm(d4, d3, 0x0B0A0908u);
            acc = and_or(tt, mT[U], acc);
            acc = and_or(uu, mU[U], acc);
        };
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        using I2 = std::integral_constant<int, 2>;
        using I3 = std::integral_constant<int, 3>;
        // one block = 4 steps = one bit word; the next block's scores load meanwhile
        // (into the other buffer: blocks go in pairs, so no register copies)
        auto block = [&](int tau4, auto PROc, auto CAPc, const unsigned* cur, unsigned* nxt) {
            load_scores(nxt);
            unsigned acc = 0u;
            step(tau4, I0{}, PROc, CAPc, cur, acc);
            step(tau4 + 1, I1{}, PROc, CAPc, cur, acc);
            step(tau4 + 2, I2{}, PROc, CAPc, cur, acc);
            step(tau4 + 3, I3{}, PROc, CAPc, cur, acc);
            return acc;
        };
        // four blocks = one tile row: words w .. w + 3 of every lane (w % 4 == 0)
        // a block pair (8 steps) is half a tile row; its words wait in LDS and the
        // second half stores the row (the phases may split a row: the stage carries it)
        auto flush = [&](int tau4) {
            asm volatile("" ::: "memory");
            const int w = ((tau4 - tau0) >> 2) & ~3;
            const uint4 row = *(const uint4*)stage;
            if (act && w < NW) *(uint4*)(bits + w * kBL) = row;
            if (summ_on) {
                const unsigned x = *sum_lds | row.x | row.y | row.z | row.w;
                const bool last = ((w >> 2) & 3) == 3;   // the block's fourth row: its summary byte
                if (last && act && (w >> 4) <= ((NW - 1) >> 4)) summ_put(w >> 4, x);   // a block with stored words
                *sum_lds = last ? 0u : x;
            }
        };
        auto pair8 = [&](int tau4, auto PROc, auto CAPc) {
            const int h2 = ((tau4 - tau0) >> 2) & 2;
            stage[h2] = block(tau4, PROc, CAPc, sc, sn);
            stage[h2 + 1] = block(tau4 + 4, PROc, CAPc, sn, sc);
            if (h2) flush(tau4);
        };
        // phases in whole block pairs (8 steps) from tau0: prologue (boundary cells,
        // captures of short reads), bulk, capture window to tau_end (may run up to 7
        // steps past it: cells outside the matrix, bits beyond NW not stored)
        auto up8 = [&](int t) { return tau0 + ((t - tau0 + 7) & ~7); };
        const int p1 = up8(tau_pro);
        const int p2 = max(p1, tau0 + ((te_lo - tau0) & ~7));
        int tau4 = tau0;
        for (; tau4 < p1; tau4 += 8) {
            pair8(tau4, std::true_type{}, std::true_type{});
        }
        for (; tau4 < p2; tau4 += 8) {
            pair8(tau4, std::false_type{}, std::false_type{});
        }
        for (; tau4 <= tau_end; tau4 += 8) {
            pair8(tau4, std::false_type{}, std::true_type{});
        }
        if (((tau4 - tau0) >> 2) & 2) flush(tau4 - 8);   // a half row left: its other half is past tau_end
        if (summ_on) {   // the last block, unless its fourth row stored it (every block up to the last word is written)
            const int wl = ((tau4 - tau0) >> 2) - 1;
            const int bl = min(wl >> 4, (NW - 1) >> 4);   // the last block with stored words
            if (act && wl >= 0) {
                // its byte unless its fourth row put it (the block ends past the computed words), then its chunk
                const bool open = (wl >> 4) <= bl && ((wl >> 2) & 3) != 3;
                if (open) ((unsigned char*)sum_chunk)[bl & 15] =
                    (unsigned char)(((*sum_lds >> 20) & 0xfu) | (((*sum_lds >> 28) & 0xfu) << 4));
                if (open || (bl & 15) != 15) summ_flush(bl);
            }
        }
        if (act) {
            unsigned* caps = (unsigned*)(region + kHdrBytes);
            caps[2 * q] = (cap0 & 0xffffu) | (capB0 & 0xffff0000u);
            caps[2 * q + 1] = (cap1 & 0xffffu) | (capB1 & 0xffff0000u);
        }
    };
    for (long long wv = (long long)blockIdx.x * wpb + wave; wv < nB; wv += (long long)gridDim.x * wpb) body(wv);
}

// ---- host-side helpers -------------------------------------------------------
int band_fill_lds_bytes(int La, int wpb, int W) {
    const int pw = W == 16 ? BandGeo<16>::PW : W == 32 ? BandGeo<32>::PW : BandGeo<kWideDiags>::PW;
    return kTabBytes + align16(2 * band_acd_elems(La)) + wpb * pw * band_pcs(La, W) + 256 + wpb * 1024 +
           (W == 16 ? wpb * 1280 : 0);   // + the stop summary's per-lane accumulators and 16-block chunks
}
int band_region_words(int La, int Lb_max, int W) { return band_words(La, Lb_max, W > kBandDiags ? W : kBandDiags); }
int64_t band_region_bytes(int La, int Lb_max, int W) { return band_region_stride(La, Lb_max, W); }
bool band_pair_geometry(int La, int Lb, int* dlo) { return band_geometry(La, Lb, dlo); }

void launch_band_fill(int W, bool summ, const KernelArgs& a, const LaunchCfg& fill, hipStream_t s) {
    if (summ)
        hipLaunchKernelGGL((nw_band_fill<16, true>), dim3(fill.grid), dim3(64 * fill.wpb), fill.lds_bytes, s, a);
    else if (W == 16)
        hipLaunchKernelGGL((nw_band_fill<16>), dim3(fill.grid), dim3(64 * fill.wpb), fill.lds_bytes, s, a);
    else if (W == 32)
        hipLaunchKernelGGL((nw_band_fill<32>), dim3(fill.grid), dim3(64 * fill.wpb), fill.lds_bytes, s, a);
    else
        hipLaunchKernelGGL((nw_band_fill<kWideDiags>), dim3(fill.grid), dim3(64 * fill.wpb), fill.lds_bytes, s, a);
}

hipError_t band_fill_occupancy(int W, int wpb, int lds, int* blocks) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(
        blocks,
        W == 16 ? (const void*)nw_band_fill<16>
                : (W == 32 ? (const void*)nw_band_fill<32> : (const void*)nw_band_fill<kWideDiags>),
        64 * wpb, lds);
}

}  // namespace nw
