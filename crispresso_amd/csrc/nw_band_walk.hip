// nw_band_walk.hip -- nw_band_walk: a band level's reads from their filled regions -- start cell,
// certificate, traceback runs, record and strings or ops (one wavefront per read; the first
// level's lane walk: one read per lane) -- and launch_band, a level's fill then its walk.
// nw_band_device.h: the band, the certificate's proof and the region's layout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_band_device.h"

#define NW_BAND_WALK_CPL 1   // gap-run cells per lane and round (a gap run inside the band is < W <= 64 cells)

namespace nw {

// ============================================================================
// Walk + emit: one wavefront per read (sorted order), latency-bound.
// ============================================================================
// The run-based traceback (nw_common.h walk_runs_wide) specialised per run type (the state
// is wave-uniform, so each round takes one scalar branch): an M run follows one diagonal
// (its band membership is uniform, tau falls by 2 per cell); X / Y runs move along a
// row / column.  Each
// lane tests CPL cells; the round's first stop is found with one ballot.  `word(tau,
// kd)` returns the band dword of anti-diagonal step tau (relative to the stored
// range) and band diagonal kd; bit positions of read h at sub-step s: Y opens hb,
// Y > X hb + 4, X opens 16 + hb, M < max(X, Y) 20 + hb, with hb = 8 h + s.
// tot (optional): [0] M columns, [1] gap columns, [2] the paid gaps' cost (runs opened inside the
// matrix: O + (k - 1) E; the end overhangs are free) -- a plain read's record without band_emit.
template <int CPL, int W>
__device__ int band_walk_runs2(const unsigned* bits, int NW, int La, int Lb, int ei, int ej, int dlo, int tb0, int h,
                               unsigned* runs, int cap, int lane, int gO = 0, int gE = 0, int* tot = nullptr) {
    int nruns = 0, last_type = -1;
    bool full = false;
    int tm = 0, tg = 0, tp = 0;
    auto push = [&](int type, int n, bool paid = false) {
        if (n <= 0) return;
        if (type == RUN_M) tm += n; else tg += n;
        if (paid) tp += (type == last_type ? 0 : gO - gE) + n * gE;
        if (type == last_type) {
            if (lane == 0) runs[nruns - 1] += (unsigned)n;
        } else if (nruns < cap) {
            if (lane == 0) runs[nruns] = ((unsigned)type << 28) | (unsigned)n;
            ++nruns;
            last_type = type;
        } else {
            full = true;
        }
    };
    // the state machine is wave-uniform: keep its inputs in SGPRs so every branch
    // below is a scalar branch (values loaded through VGPRs are not provably uniform)
    La = __builtin_amdgcn_readfirstlane(La);
    Lb = __builtin_amdgcn_readfirstlane(Lb);
    ei = __builtin_amdgcn_readfirstlane(ei);
    ej = __builtin_amdgcn_readfirstlane(ej);
    dlo = __builtin_amdgcn_readfirstlane(dlo);
    tb0 = __builtin_amdgcn_readfirstlane(tb0);
    NW = __builtin_amdgcn_readfirstlane(NW);
    h = __builtin_amdgcn_readfirstlane(h);
    if (ei == La && ej < Lb) push(RUN_X, Lb - ej);
    else if (ej == Lb && ei < La) push(RUN_Y, La - ei);
    constexpr int WR = 64 * CPL;
    constexpr int WM = 64 * 8;   // M rounds: 8 cells per lane from one dwordx4
    int i = __builtin_amdgcn_readfirstlane(ei), j = __builtin_amdgcn_readfirstlane(ej), state = RUN_M;
    const int hb = 8 * h;
    while (i > 0 && j > 0) {
        nruns = __builtin_amdgcn_readfirstlane(nruns);   // uniform (see above)
        last_type = __builtin_amdgcn_readfirstlane(last_type);
        int k0;            // cells of the current run before the stop (the run is k0 + 1 long)
        int nb = RUN_M;    // M runs: the state the stop cell continues in
        if (state == RUN_M) {
            // cells (i-1-k, j-1-k), 1-based, all on diagonal kd = j - i - dlo: one column.
            // Lane l reads the 4 words [W0 - 4l, W0 - 4l + 3] (16 steps, 8 cells of the
            // run's parity): cell u has tau = 4 (W0 - 4l) + 14 + p - 2u, run index k_l + u.
            const int kd = j - i - dlo;
            if ((unsigned)kd >= (unsigned)W) return -1;
            const int lim = min(i, j) - 1;          // k < lim: cell inside the matrix
            const int t0 = i + j - 4 + tb0;         // tau of cell k = 0
            const int p = t0 & 1;
            const int W0 = (t0 >> 2) & ~3;
            const int tl = min(max((W0 >> 2) - lane, 0), (NW >> 2) - 1);   // lane's tile row
            const int k0l = (t0 - p - 4 * W0 - 14) >> 1;   // lane 0's k of cell u = 0, in [-7, 0]
            const int kl = k0l + 8 * lane;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);   // lanes past the matrix edge stop without a load
            if (kl < lim) v = *(const uint4*)(bits + tl * (2 * W) + 4 * (kd >> 1));
            const int se = 20 + hb + 2 + p, so = 20 + hb + p;   // "M < max" bit of even / odd u
            unsigned nm = 0u;
            nm |= ((v.w >> se) & 1u) | (((v.w >> so) & 1u) << 1);
            nm |= (((v.z >> se) & 1u) << 2) | (((v.z >> so) & 1u) << 3);
            nm |= (((v.y >> se) & 1u) << 4) | (((v.y >> so) & 1u) << 5);
            nm |= (((v.x >> se) & 1u) << 6) | (((v.x >> so) & 1u) << 7);
            const int sz = min(max(-kl, 0), 8), sl = min(max(lim - kl, 0), 8);
            const unsigned ge0 = (0xffu << sz) & 0xffu, gel = (0xffu << sl) & 0xffu;
            const unsigned stop = (nm | gel) & ge0;
            const unsigned long long m = __ballot(stop != 0u);
            if (m == 0) {   // cells k < k0l + WM tested (k0l <= 0)
                push(RUN_M, WM + k0l);
                i -= WM + k0l;
                j -= WM + k0l;
                continue;
            }
            const int L = (int)__builtin_ctzll(m);
            const unsigned sL = (unsigned)__builtin_amdgcn_readlane((int)stop, L);
            const int u0 = (int)__builtin_ctz(sL);
            k0 = k0l + 8 * L + u0;
            const int q = u0 >> 1;
            const unsigned wq = (unsigned)__builtin_amdgcn_readlane(
                (int)(q == 0 ? v.w : (q == 1 ? v.z : (q == 2 ? v.y : v.x))), L);
            nb = ((wq >> (4 + hb + ((u0 & 1) ? p : 2 + p))) & 1u) ? RUN_Y : RUN_X;
            push(RUN_M, k0 + 1);
            i -= k0 + 1;
            j -= k0 + 1;
            state = nb;
        } else {
            // X: cells (i, j-k), diagonal kd = j - k - i - dlo; Y: cells (i-k, j), kd = j - i + k - dlo
            const bool isX = state == RUN_X;
            const int lim = isX ? j : i;             // k < lim: inside the matrix
            const int kd0 = j - i - dlo;
            const int t0 = i + j - 2 + tb0;          // tau of cell k = 0
            const int bit = isX ? 16 : 0;            // "opens" bit of the run's gap type
            unsigned stop = 0u, oob = 0u;
#pragma unroll
            for (int u = 0; u < CPL; ++u) {
                const int kk = lane * CPL + u;
                const int kd = isX ? kd0 - kk : kd0 + kk;
                const int tau = t0 - kk;
                const bool out = (unsigned)kd >= (unsigned)W;
                const int wd = min(max(tau, 0) >> 2, NW - 1);
                const unsigned w = (kk < lim && !out) ? bits[(wd >> 2) * (2 * W) + 4 * ((kd & (W - 1)) >> 1) + (wd & 3)]
                                                      : 0u;   // cells that stop anyway: no load
                const bool opens = ((w >> (bit + hb + (tau & 3))) & 1u) != 0u;
                const bool valid = kk < lim;
                stop |= (unsigned)(!valid || out || opens) << u;
                oob |= (unsigned)(valid && out) << u;
            }
            const unsigned long long m = __ballot(stop != 0u);
            if (m == 0) {
                push(state, WR, true);
                if (isX) j -= WR; else i -= WR;
                continue;
            }
            const int L = (int)__builtin_ctzll(m);
            const unsigned sL = (unsigned)__builtin_amdgcn_readlane((int)stop, L);
            const int u0 = (int)__builtin_ctz(sL);
            if (((unsigned)__builtin_amdgcn_readlane((int)oob, L) >> u0) & 1u) return -1;
            k0 = L * CPL + u0;
            push(state, k0 + 1, true);
            if (isX) j -= k0 + 1; else i -= k0 + 1;
            state = RUN_M;
        }
        if (full) return -1;
    }
    if (i > 0) push(RUN_Y, i);
    if (j > 0) push(RUN_X, j);
    if (tot) {
        tot[0] = tm;
        tot[1] = tg;
        tot[2] = tp;
    }
    return full ? -1 : nruns;
}

constexpr int kBandReadCap = 1280;   // >= the band length cap (La + 31, La <= 1024): every walked read fits
// lut, amplicon bytes, markup rows, the EDNAFULL score rows (17 x 16 int8: the
// single-diagonal test)
__host__ __device__ inline int band_walk_shared_bytes(int La) { return 256 + align16(La + 16) + align16(4 * La) + 17 * 16; }
constexpr int kBandRunsCap = 256;     // traceback runs per read (more: the read goes to the next level)
__host__ __device__ inline int band_walk_row(int La, int lb_max) { return (La + lb_max + 15) & ~15; }   // = stride_for()
__host__ __device__ inline int band_walk_rcap(int lb_max) { return min(kBandReadCap, (lb_max + 255) & ~255); }
// a pair's header and W captures, whole 64-dword DMA loads
__host__ __device__ constexpr int band_walk_hdr_slot(int W) { return 64 * ((kHdrBytes / 4 + W + 63) / 64); }
// per wave: runs, two read-byte buffers and two header slots (one read ahead), the three output rows
__host__ __device__ inline int band_walk_wave_bytes(int La, int lb_max, int W) {
    return kBandRunsCap * 4 + 2 * (band_walk_rcap(lb_max) + 256) + 2 * 4 * band_walk_hdr_slot(W) +
           3 * band_walk_row(La, lb_max);
}

// emit_alignment (nw_common.h) with the three rows built in LDS (byte writes) and
// written out as dwordx4 rows: 16 B per lane instead of a byte store per column.
// The rows are padded to 16 B; the host reads aln_len columns of each.
template <bool ROWS, class Score>
__device__ void band_emit(const unsigned* runs, int nruns, const unsigned char* amp, const unsigned char* raw,
                          const unsigned char* lut, const Score& sim_score, unsigned char* rows, int row,
                          unsigned char* o_ref, int64_t stride, int score, int ei, int ej, Stat* st, int lane) {
    int col = 0, ia = 0, jb = 0;
    int n_id = 0, n_sim = 0, n_gap = 0;
    for (int q = nruns - 1; q >= 0; --q) {
        const unsigned rc = (unsigned)__builtin_amdgcn_readfirstlane((int)runs[q]);
        const int type = (int)(rc >> 28);
        const int n = (int)(rc & 0x0fffffffu);
        if (type == RUN_M) {
            int same = 0;   // columns with identical bytes (not '-'): '|', identical and similar
            for (int c0 = 0; c0 < n; c0 += 64) {   // uniform trip count: scalar loop
                const int p = c0 + lane;
                if (p < n) {
                    const unsigned char ca = amp[ia + p], cb = raw[jb + p];
                    unsigned char mk = '|';
                    if (ca != cb || ca == '-') {   // rare: a mismatch, a case difference or an input '-'
                        mk = ' ';
                        if (ca == '-' || cb == '-') {   // an input '-' counts as a gap (CORE:1846)
                            ++n_gap;
                        } else {
                            const bool id = upcase(ca) == upcase(cb);
                            const bool sim = id || sim_score(ia + p, (int)lut[cb]) > 0;
                            mk = id ? '|' : (sim ? ':' : '.');
                            n_id += id;
                            n_sim += sim;
                        }
                    } else {
                        ++same;
                    }
                    if constexpr (ROWS) {
                        rows[col + p] = ca;
                        rows[row + col + p] = mk;
                        rows[2 * row + col + p] = cb;
                    }
                }
            }
            n_id += same;
            n_sim += same;
        } else if constexpr (!ROWS) {   // gap run: n gap columns
            if (lane == 0) n_gap += n;
        } else {   // gap run: every column is a gap
            const unsigned char* src = type == RUN_X ? raw + jb : amp + ia;
            unsigned char* dst = rows + (type == RUN_X ? 2 * row : 0) + col;
            unsigned char* gap = rows + (type == RUN_X ? 0 : 2 * row) + col;
            for (int c0 = 0; c0 < n; c0 += 64) {
                const int p = c0 + lane;
                if (p < n) {
                    dst[p] = src[p];
                    rows[row + col + p] = ' ';
                    gap[p] = '-';
                    ++n_gap;
                }
            }
        }
        col += n;
        if (type != RUN_X) ia += n;
        if (type != RUN_Y) jb += n;
    }
    if constexpr (ROWS) lds_fence();
    for (int c = 16 * lane; ROWS && c < col; c += 1024) {
        const uint4 r0 = *(const uint4*)(rows + c), r1 = *(const uint4*)(rows + row + c),
                    r2 = *(const uint4*)(rows + 2 * row + c);
        *(uint4*)(o_ref + c) = r0;
        *(uint4*)(o_ref + stride + c) = r1;
        *(uint4*)(o_ref + 2 * stride + c) = r2;
    }
    if (col < 1024) {
        const unsigned t = wave_sum_u32((unsigned)n_id | ((unsigned)n_sim << 10) | ((unsigned)n_gap << 20));
        n_id = (int)(t & 1023u);
        n_sim = (int)((t >> 10) & 1023u);
        n_gap = (int)(t >> 20);
    } else {
        n_id = wave_sum(n_id);
        n_sim = wave_sum(n_sim);
        n_gap = wave_sum(n_gap);
    }
    if (lane == 0) {
        Stat s;
        s.aln_len = col;
        s.n_ident = n_id;
        s.n_sim = n_sim;
        s.n_gaps = n_gap;
        s.score = score;
        s.end_i = ei;
        s.end_j = ej;
        s.flags = 0;
        *st = s;
    }
}


// True when every single-diagonal alignment outside [dlo, dhi] whose overlap could
// reach `score` (maxsub * P(d) >= score) scores below it.  A score table lookup per
// pair: amplicon / read bytes in LDS, the amplicon's EDNAFULL code (lut) and the read's
// 6-code (lut6), scores from band_tab (packed with + 2E, entry [x][y][y]).
__device__ bool band_single_diagonals_below(const KernelArgs& a, const unsigned char* amp, const unsigned char* rd,
                                            int La, int Lb, int dlo, int dhi, int score, int lane) {
    const int E2 = 2 * a.gap_extend;
    for (int side = 0; side < 2; ++side) {
        for (int k = 1;; ++k) {
            const int d = side == 0 ? dhi + k : dlo - k;
            const int P = diag_pairs(La, Lb, d);
            if (P <= 0 || a.band_maxsub * P < score) break;
            const int i0 = d >= 0 ? 0 : -d, j0 = d >= 0 ? d : 0;   // 0-based first pair
            int sum = 0;
            for (int t = lane; t < P; t += 64) {
                const int x = a.lut[amp[i0 + t]], y = a.lut6[rd[j0 + t]];
                const unsigned w = a.band_tab[x * 36 + (y < 6 ? y : 5) * 7];
                sum += (int)(short)(w & 0xffffu) - E2;
            }
            if (wave_sum(sum) >= score) return false;
        }
    }
    return true;
}

// The first level's walk, one read per lane (ops output): 64 consecutive list positions per
// wavefront, each lane its own read's header, start cell, certificate and traceback
// (band_walk_runs2's rules cell for cell, the state machine in VGPRs: the wave-per-read walk
// spends ~430 scalar instructions per read on it), its record from the runs and the score
// (plain reads), its runs into its slot.  What a lane cannot finish -- the refined certificate
// (sums over the band's neighbour diagonals), reads with codes outside A C G T, more than
// kLaneRuns runs -- goes to `defer(k)`, the wave-per-read body, one read at a time.
constexpr int kLaneRuns = 8;   // runs per lane in LDS ([kLaneRuns][64] dwords at the wave's area)
#define NW_MIS_UNROLL 8   // dword compares in flight per lane in count_mis (4: walk 0.086 ms, 8: 0.079, 16: 0.081)
constexpr int kMRows = 2;   // tile rows per M round of the lane walk (<= 4: 32 cells)
// The lane walk (with the stop summary its fill writes) pays on one long list: the kernel-resident
// pass, walk<16> 0.189 -> 0.092 ms (fill<16> +13 us for the summary).  A pipelined call runs it on
// its chunks of >= 65536 reads of one amplicon (the call's time the same, C2 1.961 vs 1.954 ms; its
// kernels faster); the pooled call's small chunks keep the wave walk (C5 17.15 vs 16.61 ms with the
// lane walk on every chunk, in-process A/Bs).  KernelArgs::band_summ selects it per launch.
// (Running it twice -- the certificates alone, then, while the next levels ran on a side stream, the
// walk of what they kept -- measured no gain: resident pass 0.700-0.703 vs 0.690-0.700 ms, C2 call
// 1.951 vs 1.956 ms; the walk and the wide level slowed each other to the serial sum)
template <int W, class Defer>
__device__ void walk_lanes(const KernelArgs& a, long long klo, long long khi, unsigned char* wb,
                           const unsigned char* amp_lds, bool amp_acgt, int sc5, const Defer& defer) {
    constexpr int kCapBytes = BandGeo<W>::CapBytes;
    const int La = a.La, E = a.gap_extend, O = a.gap_open, m = a.band_maxsub, NW = a.band_words;
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6, wave = threadIdx.x >> 6;
    const int rcap = band_walk_rcap(a.Lb_max);
    unsigned* lruns = (unsigned*)wb;   // [kLaneRuns][64]: lane's run q at lruns[64 q + lane]
    const long long ng = (khi - klo + 63) >> 6;
    for (long long g = (long long)blockIdx.x * wpb + wave; g < ng; g += (long long)gridDim.x * wpb) {
        const long long k = klo + 64 * g + lane;
        const bool live = k < khi;
        // 0: done, 1: the wave path, 2: redo list (retry), 3: fallback list
        int fate = 0;
        long long rd = 0;
        if (live) {
            const unsigned char* region = a.band_region + ((k >> 1) - a.band_pair_lo) * a.band_stride;
            const int4 hdr = *(const int4*)region, hr = *(const int4*)(region + 16), ho = *(const int4*)(region + 32);
            const int h = (int)(k & 1);
            rd = h ? hr.y : hr.x;
            const int Lb = h ? hr.w : hr.z;
            if (a.redo_flags) a.redo_flags[k] = 0;
            if (Lb <= 0) {
                Stat z = {};
                z.flags = FLAG_EMPTY;
                a.stats[rd] = z;
                a.nops[rd] = 0;
            } else if (hdr.z & kPairInactive) {
                fate = 2;
            } else if (Lb > rcap) {
                fate = 3;
            } else {
                const int dlo = hdr.y, tau0 = hdr.x;
                // start cell: the largest end key over the band's diagonals (their last cells)
                const uint4* capw = (const uint4*)(region + kHdrBytes);
                unsigned k32 = 0u;
#pragma unroll
                for (int c4 = 0; c4 < W / 4; ++c4) {
                    const uint4 q4 = capw[c4];
                    const unsigned cv[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int d = dlo + 4 * c4 + e;
                        const int iend = La < Lb - d ? La : Lb - d;
                        const int ilo = 1 - d > 1 ? 1 - d : 1;
                        if (iend >= ilo) {
                            const int v = half(cv[e], h) - kBias16 - E * (2 * iend + d);
                            const int jend = iend + d;
                            const unsigned kk = (iend == La && jend == Lb) ? end_key32(v, 3, 0)
                                                : (jend == Lb ? end_key32(v, 2, iend - 1) : end_key32(v, 1, jend - 1));
                            k32 = kk > k32 ? kk : k32;
                        }
                    }
                }
                int score, ei, ej;
                decode_end(end_key_widen(k32), La, Lb, &score, &ei, &ej);
                const int dhi = dlo + W - 1;
                int pmax = -1;
                if (dhi < Lb - 1) pmax = max(pmax, min(Lb - dhi - 1, La));
                if (dlo > 1 - La) pmax = max(pmax, min(Lb, La + dlo - 1));
                const bool certified = pmax < 0 || score > m * pmax;
                const bool bad_code = (hdr.z & (h ? REGION_BAD_B : REGION_BAD_A)) != 0;
                const bool plain = amp_acgt && !(hdr.z & (h ? (REGION_BAD_B | REGION_NP_B) : (REGION_BAD_A | REGION_NP_A)));
                const int nd = min(ei, ej);
                const long long off = h ? (long long)(((unsigned long long)(unsigned)ho.w << 32) | (unsigned)ho.z)
                                        : (long long)(((unsigned long long)(unsigned)ho.y << 32) | (unsigned)ho.x);
                // mismatches of amplicon bytes [ia, ia + n) against read bytes [jb, jb + n) (plain: A C G T,
                // case folded), dword compares, NW_MIS_UNROLL dwords' loads together.  The count stops once
                // 9 sc5 c is past `slack`: the caller asks only whether it stays within it, an unrelated
                // diagonal is past it within its first dwords, and every further batch is a dependent global
                // round trip (to the end of a 250-base diagonal: 8 of them, for each diagonal in turn)
                auto count_mis = [&](int ia, int jb, int n, int slack) -> int {
                    int c = 0;
                    const unsigned char* rp = a.reads + off + jb;
                    const int ra = (int)((uintptr_t)rp & 3), aa = ia & 3;
                    const unsigned* rw = (const unsigned*)(rp - ra);
                    const unsigned* aw = (const unsigned*)(amp_lds + (ia - aa));
                    const int nwd = (n + 3) >> 2;   // the last dword index read (the same with and without the stop)
                    unsigned rlo = rw[0], alo = aw[0];
                    for (int w0 = 0; w0 < nwd && 9 * sc5 * c <= slack; w0 += NW_MIS_UNROLL) {
                        unsigned rr[NW_MIS_UNROLL], av[NW_MIS_UNROLL];
#pragma unroll
                        for (int u = 0; u < NW_MIS_UNROLL; ++u) {
                            rr[u] = rw[min(w0 + u + 1, nwd)];
                            av[u] = aw[min(w0 + u + 1, nwd)];
                        }
#pragma unroll
                        for (int u = 0; u < NW_MIS_UNROLL; ++u) {
                            const int left = n - 4 * (w0 + u);   // bytes of this dword inside the diagonal
                            unsigned x = (__builtin_amdgcn_alignbyte(rr[u], rlo, ra) ^ __builtin_amdgcn_alignbyte(av[u], alo, aa)) &
                                         0xdfdfdfdfu;
                            x &= left >= 4 ? 0xffffffffu : (left <= 0 ? 0u : 0xffffffffu >> (8 * (4 - left)));
                            c += 4 - __builtin_popcount(zero_bytes(x));
                            rlo = rr[u];
                            alo = av[u];
                        }
                    }
                    return c;
                };
                bool cert = certified;
                if (!certified && !bad_code && score > m * pmax - O) {
                    // the refined certificate (band_single_diagonals_below): every single diagonal beyond the
                    // band whose overlap could reach the score sums below it -- a plain read's diagonal d
                    // sums to m P - 9 sc5 mis_d; other reads: the wave path
                    if (!plain) {
                        fate = 1;
                    } else {
                        cert = true;
                        for (int side = 0; side < 2 && cert; ++side) {
                            for (int kq = 1;; ++kq) {
                                const int d = side == 0 ? dhi + kq : dlo - kq;
                                const int P = diag_pairs(La, Lb, d);
                                if (P <= 0 || m * P < score) break;
                                const int i0 = d >= 0 ? 0 : -d, j0 = d >= 0 ? d : 0;
                                // m P - 9 sc5 mis_d >= score: the diagonal reaches the score
                                if (9 * sc5 * count_mis(i0, j0, P, m * P - score) <= m * P - score) {
                                    cert = false;
                                    break;
                                }
                            }
                        }
                    }
                }
                if (fate != 0) {
                } else if (bad_code || !cert) {
                    fate = bad_code ? 3 : 2;
                } else if (!plain || nd >= 1024) {
                    fate = 1;
                } else {
                    // (no single-diagonal fast path here: when the start cell's diagonal sums to the score the
                    // walk's M rounds follow that diagonal to the edge -- M wins every tie on it -- and the record
                    // from the runs equals the diagonal's; a compare of every pair would cost as many rounds)
                    int nr = 0, tm = 0, tg = 0, tp = 0, last = -1;
                    bool over = false;
                    auto push = [&](int type, int n, bool paid) {
                        if (n <= 0) return;
                        if (type == RUN_M) tm += n; else tg += n;
                        if (paid) tp += (type == last ? 0 : O - E) + n * E;
                        if (type == last) {
                            lruns[64 * (nr - 1) + lane] += (unsigned)n;
                        } else if (nr < kLaneRuns) {
                            lruns[64 * nr + lane] = ((unsigned)type << 28) | (unsigned)n;
                            ++nr;
                            last = type;
                        } else {
                            over = true;
                        }
                    };
                    if (ei == La && ej < Lb) push(RUN_X, Lb - ej, false);
                    else if (ej == Lb && ei < La) push(RUN_Y, La - ei, false);
                    Stat r;
                    r.score = score;
                    r.end_i = ei;
                    r.end_j = ej;
                    r.flags = 0;
                    {
                        // band_walk_runs2, one lane: M runs scan kMRows tile rows (8 cells of their diagonal
                        // each) per round, X / Y runs 8 cells per round; the same stop rules
                        const unsigned* bits = (const unsigned*)(region + kHdrBytes + kCapBytes);
                        const int tb0 = kBK - dlo + 2 - tau0, hb = 8 * h;
                        int i = ei, j = ej, state = RUN_M, kc = 0;   // kc: cells of the current run so far
                        bool fail = false;
                        // the stop summary (band_summ_bytes): 16 blocks' bytes of one diagonal pair per load,
                        // kept while the M runs stay on that pair and chunk
                        const unsigned char* summ = (const unsigned char*)bits + (size_t)NW * (W / 2) * 4;
                        const int NBp = band_summ_bytes(NW);
                        int skey = -1;
                        uint4 sv = make_uint4(0u, 0u, 0u, 0u);
                        for (int guard = 0; i > 0 && j > 0 && !over && !fail; ++guard) {
                            if (guard > 4 * (La + Lb + 64)) {
                                fate = 1;
                                break;
                            }
                            if (state == RUN_M) {
                                const int kd = j - i - dlo;
                                if ((unsigned)kd >= (unsigned)W) {
                                    fail = true;
                                    break;
                                }
                                const int lim = min(i, j) - 1;
                                const int tc = i + j - 4 + tb0 - 2 * kc;   // tau of the next cell to test
                                const int r0 = tc >> 4, NR = NW >> 2;
                                if (tc >= 0 && r0 < NR) {
                                    // the first block at or below tc's with an "M < max" bit of this read on this
                                    // diagonal (tau parity p: sub-steps p, p + 2); the cells above it are clear
                                    const int b = tc >> 6, pq = kd >> 1;
                                    const unsigned shb = 4 * h + (tc & 1);
                                    int bf = -1;
                                    for (int ch = b >> 4; ch >= 0 && bf < 0; --ch) {
                                        if (skey != pq * 64 + ch) {
                                            sv = *(const uint4*)(summ + pq * NBp + 16 * ch);
                                            skey = pq * 64 + ch;
                                        }
                                        const unsigned sw[4] = {sv.x, sv.y, sv.z, sv.w};
                                        unsigned m16 = 0u;
#pragma unroll
                                        for (int e = 0; e < 4; ++e) {
                                            const unsigned t = (sw[e] >> shb) & 0x05050505u;
                                            const unsigned nz = (t + 0x7f7f7f7fu) & 0x80808080u;   // bytes with a bit
                                            m16 |= (((nz >> 7) & 1u) | ((nz >> 14) & 2u) | ((nz >> 21) & 4u) | ((nz >> 28) & 8u))
                                                   << (4 * e);
                                        }
                                        const int top = ch == (b >> 4) ? (b & 15) : 15;
                                        const unsigned cand = m16 & ((2u << top) - 1u);
                                        if (cand) bf = 16 * ch + 31 - __builtin_clz(cand);
                                    }
                                    if (bf < b) {   // skip the clear blocks (to the matrix edge when none is flagged)
                                        const int tstop = bf < 0 ? -1 : 64 * bf + 63;
                                        const int cnt = (tc - tstop + 1) >> 1;   // cells with tau > tstop
                                        const int L = lim - kc;
                                        if (cnt > L) {   // the run reaches the matrix edge first
                                            const int run = kc + max(L, 0) + 1;
                                            push(RUN_M, run, false);
                                            i -= run;
                                            j -= run;
                                            kc = 0;
                                        } else {
                                            kc += cnt;
                                        }
                                        continue;
                                    }
                                }
                                // kMRows tile rows per round (8 cells of the diagonal each), their loads together
                                uint4 v[kMRows];
#pragma unroll
                                for (int q = 0; q < kMRows; ++q)
                                    v[q] = r0 - q >= 0 && r0 - q < NR ? *(const uint4*)(bits + (r0 - q) * (2 * W) + 4 * (kd >> 1))
                                                                      : make_uint4(0u, 0u, 0u, 0u);
                                // the rows' cells of this diagonal in decreasing tau, from the "M < max" bits of its
                                // parity (s = p: bit sh, s = p + 2: bit sh + 2 of each word)
                                const int p = tc & 1;
                                const unsigned sh = 20 + hb + p;
                                unsigned long long all = 0ull, oddr = 0ull;
#pragma unroll
                                for (int q = 0; q < kMRows; ++q) {
                                    const unsigned w[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
                                    unsigned mm = 0u;
#pragma unroll
                                    for (int e = 0; e < 4; ++e) {
                                        const unsigned t = w[e] >> sh;
                                        mm |= (((t >> 2) & 1u) | ((t & 1u) << 1)) << (2 * (3 - e));
                                    }
                                    all |= (unsigned long long)mm << (8 * q);
                                    // a cell of the matrix outside the stored steps: the wave path's clamps decide
                                    if (r0 - q < 0 || r0 - q >= NR) oddr |= 0xffull << (8 * q);
                                }
                                constexpr int kCells = 8 * kMRows;
                                const int c0 = (16 * r0 + 14 + p - tc) >> 1;   // cell tc's place in row r0 (0 .. 7)
                                const int ncell = kCells - c0;
                                const unsigned cells = (unsigned)((1ull << ncell) - 1ull);
                                const unsigned nm = (unsigned)(all >> c0) & cells;
                                const int L = lim - kc;   // cells u < L are inside the matrix
                                const unsigned inm = L <= 0 ? 0u : (L >= ncell ? cells : (1u << L) - 1u);
                                const unsigned stop = nm | (cells & ~inm);
                                const unsigned odd = (unsigned)(oddr >> c0) & inm;
                                const unsigned upto = stop ? (unsigned)((2ull << __builtin_ctz(stop)) - 1ull) : 0xffffffffu;
                                if (odd & upto) {
                                    fate = 1;
                                    break;
                                }
                                if (stop) {
                                    const int u0 = __builtin_ctz(stop);
                                    const int run = kc + u0 + 1;
                                    push(RUN_M, run, false);
                                    i -= run;
                                    j -= run;
                                    const int ts = tc - 2 * u0;   // the stop cell: "Y > X" picks the gap it continues in
                                    uint4 vs = v[0];
#pragma unroll
                                    for (int q = 1; q < kMRows; ++q) vs = (ts >> 4) == r0 - q ? v[q] : vs;
                                    const int qs = (ts >> 2) & 3;
                                    const unsigned ws = qs == 0 ? vs.x : (qs == 1 ? vs.y : (qs == 2 ? vs.z : vs.w));
                                    state = ((ws >> (4 + hb + (ts & 3))) & 1u) ? RUN_Y : RUN_X;
                                    kc = 0;
                                } else {
                                    kc += ncell;
                                }
                            } else {
                                const bool isX = state == RUN_X;
                                const int lim = isX ? j : i;
                                const int kd0 = j - i - dlo;
                                const int t0 = i + j - 2 + tb0;
                                const int bit = isX ? 16 : 0;
                                unsigned stop = 0u, oob = 0u;
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    const int kk = kc + u;
                                    const int kd = isX ? kd0 - kk : kd0 + kk;
                                    const int tau = t0 - kk;
                                    const bool out = (unsigned)kd >= (unsigned)W;
                                    const int wd = min(max(tau, 0) >> 2, NW - 1);
                                    const bool valid = kk < lim;
                                    const unsigned w = (valid && !out)
                                                           ? bits[(wd >> 2) * (2 * W) + 4 * ((kd & (W - 1)) >> 1) + (wd & 3)]
                                                           : 0u;
                                    const bool opens = ((w >> (bit + hb + (tau & 3))) & 1u) != 0u;
                                    stop |= (unsigned)(!valid || out || opens) << u;
                                    oob |= (unsigned)(valid && out) << u;
                                }
                                if (stop) {
                                    const int u0 = __builtin_ctz(stop);
                                    if ((oob >> u0) & 1u) {
                                        fail = true;
                                        break;
                                    }
                                    const int run = kc + u0 + 1;
                                    push(state, run, true);
                                    if (isX) j -= run; else i -= run;
                                    state = RUN_M;
                                    kc = 0;
                                } else {
                                    kc += 8;
                                }
                            }
                        }
                        if (fate == 0) {
                            if (fail) {
                                fate = 2;
                            } else {
                                if (i > 0) push(RUN_Y, i, false);
                                if (j > 0) push(RUN_X, j, false);
                                // a plain read's record from its runs and score: m id - x (M - id) - paid gaps
                                const int idn = score + tp + 4 * sc5 * tm;
                                if (over || idn < 0 || idn % (9 * sc5) != 0) {
                                    fate = 1;
                                } else {
                                    r.aln_len = tm + tg;
                                    r.n_ident = idn / (9 * sc5);
                                    r.n_sim = r.n_ident;
                                    r.n_gaps = tg;
                                }
                            }
                        }
                    }
                    if (fate == 0 && over) fate = 1;
                    if (fate == 0) {
                        // store_ops for one lane: its runs start -> end into its slot (or the spill area)
                        uint32_t* dst = a.ops + a.ops_stride * a.ops_slot + rd * a.ops_slot;
                        int32_t flag = kNopsRows;
                        bool lost = false;
                        if (nr > a.ops_slot) {
                            flag = 0;
                            const int pos = atomicAdd(a.ops_ctl, nr);
                            if ((long long)pos + nr > a.spill_cap) {
                                atomicOr(a.ops_ctl + kSpillFull, 1);
                                a.nops[rd] = 0;
                                lost = true;
                            } else {
                                a.ops[rd] = (uint32_t)pos;
                                dst = a.spill + pos;
                            }
                        }
                        if (!lost) {
                            a.nops[rd] = nr | flag;
                            for (int q = 0; q < nr; ++q) dst[q] = lruns[64 * (nr - 1 - q) + lane];
                        }
                        a.stats[rd] = r;
                    }
                }
            }
        }
        // the lists: one atomic per list and wavefront (redo flags instead when the level keeps them)
        const unsigned long long to_redo = __ballot(fate == 2 && !a.redo_flags), to_fb = __ballot(fate == 3);
        if (fate == 2 && a.redo_flags) a.redo_flags[k] = 1;
        if (to_redo) {
            int base = 0;
            if (lane == 0) base = atomicAdd(a.redo_count, (int)__builtin_popcountll(to_redo));
            base = __builtin_amdgcn_readfirstlane(base);
            if ((to_redo >> lane) & 1ull) a.redo_list[base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(to_redo >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)to_redo, 0u))] = (int)rd;
        }
        if (to_fb) {
            int base = 0;
            if (lane == 0) base = atomicAdd(a.fallback_count, (int)__builtin_popcountll(to_fb));
            base = __builtin_amdgcn_readfirstlane(base);
            if ((to_fb >> lane) & 1ull) a.fallback_list[base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(to_fb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)to_fb, 0u))] = rd;
        }
        // the wave path for the rest, one read at a time (its LDS buffers overlay lruns: read above)
        lds_fence();
        for (unsigned long long dq = __ballot(fate == 1); dq; dq &= dq - 1) {
            const int u = (int)__builtin_ctzll(dq);
            const long long ku = klo + 64 * g + u;
            defer(ku);
            lds_fence();
        }
    }
}

// W < kBandDiags: a first level; reads it cannot certify go to the redo list of the
// next (wider) level.  W >= kBandDiags: they go to the fallback list (W = kBandDiags: the
// wide level's input; the wide level: the exact int32 kernel's).
template <int W, bool LN = false>   // LN: the lane walk (walk_lanes) first, W < kBandDiags, ops output
#define NW_WALK_WPE 6
#define NW_WALK_LANE_WPE 4   // the lane walk: 116 VGPRs, no spills (5: 96 with 11 spilled, walk 0.091 vs 0.085 ms); a resident pass runs ~9 of its wavefronts per CU
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(LN ? NW_WALK_LANE_WPE : NW_WALK_WPE))) void nw_band_walk(const KernelArgs a) {
    using G = BandGeo<W>;
    constexpr int kCapBytes = G::CapBytes;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // second level skipped: its reads go to the wide level (with the seeded list: that list alone)
    if (W == kBandDiags && redo_direct_taken(a) && a.seed_l2 != 1) return;
    if (W < kBandDiags && l1_skipped(a)) return;   // first level skipped (KernelArgs::l1_skip)
    if (W >= kBandDiags && a.tail_prio) __builtin_amdgcn_s_setprio(3);
    // beside a wide-first launch (raised priority, as every wide launch): the same, or its wavefronts wait for that one's
    if (W < kBandDiags && a.wf_list && a.tail_prio) __builtin_amdgcn_s_setprio(3);
    constexpr int CW = W > 64 ? W / 64 : 1;   // captures (band diagonals) per lane
    const int La = a.La, E = a.gap_extend;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wpb = blockDim.x >> 6;
    // Reads handed on (next level's redo list, or the exact kernel's list) wait in a
    // lane of the wavefront (entry p in lane p) and go out 64 at a time: one atomic
    // per 64 reads and one coalesced store (a per-read atomic on one counter serialises
    // when most reads are handed on, e.g. the HDR pass).  Called wave-uniformly.
    int redo_n = 0, fb_n = 0;
    int redo_v = 0;
    long long fb_v = 0;
    auto flush_redo = [&]() {
        int base = 0;
        if (lane == 0) base = atomicAdd(a.redo_count, redo_n);
        base = __builtin_amdgcn_readfirstlane(base);
        if (lane < redo_n) a.redo_list[base + lane] = redo_v;
        redo_n = 0;
    };
    auto flush_fb = [&]() {
        int base = 0;
        if (lane == 0) base = atomicAdd(a.fallback_count, fb_n);
        base = __builtin_amdgcn_readfirstlane(base);
        if (lane < fb_n) a.fallback_list[base + lane] = fb_v;
        fb_n = 0;
    };
    // the second level over the seeded list (seed_l2 == 1): positions from l2_s0 on are seeded reads
    const bool l2s = W == kBandDiags && a.seed_l2 == 1;
    const long long l2_nr = l2s ? l2_redo_n(a) : 0ll;
    const long long l2_s0 = l2s ? (l2_nr + 1) & ~1ll : (1ll << 62);
    auto seed_done = [&](long long k) {   // a seeded read's record and runs are out
        if (k >= l2_s0 && lane == 0) a.seed_flags[k - l2_s0] = 0;
    };
    auto give_up = [&](long long k, long long rd, bool retry) {
        if (k >= l2_s0) {   // a seeded read: to the wide level, in the seeded list's order (compaction)
            if (lane == 0) a.seed_flags[k - l2_s0] = 1;
            return;
        }
        if (W < kBandDiags && retry && a.redo_flags) {
            // the next level's list keeps the sorted order (nw_band_redo_* compaction):
            // its pairs are reads of similar length, as on this level
            if (lane == 0) a.redo_flags[k] = 1;
        } else if (W < kBandDiags && retry) {
            if (lane == redo_n) redo_v = (int)rd;
            if (++redo_n == 64) flush_redo();
        } else {
            if (lane == fb_n) fb_v = rd;
            if (++fb_n == 64) flush_fb();
        }
    };
    unsigned char* lut_lds = smem;
    unsigned char* amp_lds = smem + 256;
    unsigned* rowpos = (unsigned*)(smem + 256 + align16(La + 16));
    unsigned* sub_lds = rowpos + align16(4 * La) / 4;   // [17][4]: EDNAFULL(a, b) * scale, int8, b = 0..15
    for (int k = tid; k < 256; k += blockDim.x) lut_lds[k] = a.lut[k];
    for (int k = tid; k < La; k += blockDim.x) {
        amp_lds[k] = a.amp[k];
        rowpos[k] = a.rowpos[k];
    }
    for (int k = tid; k < 17 * 4; k += blockDim.x) sub_lds[k] = a.sub16[k];
    int acgt = 1;
    for (int k = tid; k < La; k += blockDim.x) {
        const unsigned char c = upcase(a.amp[k]);
        acgt &= c == 'A' || c == 'C' || c == 'G' || c == 'T';
    }
    // a plain read (A C G T against an A C G T amplicon, EDNAFULL): every pair scores +m or -x
    // (x = 4 m / 5), so a diagonal's sum, and an alignment's identities, follow from its score
    const int sc5 = a.band_maxsub / 5;
    const bool amp_acgt = __syncthreads_and(acgt) && a.band_maxsub == 5 * sc5;
    // substitution score of amplicon byte x against read byte y (0 for codes outside EDNAFULL)
    auto sub_of = [&](unsigned char x, unsigned char y) {
        const int cx = lut_lds[x], cy = lut_lds[y];
        return cy < 16 ? (int)(signed char)(sub_lds[cx * 4 + (cy >> 2)] >> (8 * (cy & 3))) : 0;
    };
    const int row = band_walk_row(La, a.Lb_max);   // columns <= La + Lb
    const int rcap = band_walk_rcap(a.Lb_max);
    constexpr int kSlot = band_walk_hdr_slot(W);   // dwords of a pair header + captures slot
    unsigned char* wb = smem + band_walk_shared_bytes(La) + wave * band_walk_wave_bytes(La, a.Lb_max, W);
    unsigned* runs = (unsigned*)wb;
    unsigned char* rbufs = wb + kBandRunsCap * 4;               // [2][rcap + 256]: read bytes (DMA)
    unsigned* hbufs = (unsigned*)(rbufs + 2 * (rcap + 256));    // [2][kSlot]: pair header + captures (DMA)
    unsigned char* rows = (unsigned char*)(hbufs + 2 * kSlot);

    const long long count = band_list_count(a);
    const long long klo = 2 * a.band_pair_lo;
    const long long khi = 2 * a.band_pair_hi < count ? 2 * a.band_pair_hi : count;
    // Per read, everything it needs from memory before its walk -- the pair header (reads,
    // lengths, offsets, geometry), the W captures and the read's bytes -- lands in LDS by DMA
    // ahead of it: read k's bytes (and read k + kstep's header) go out right after read
    // k - kstep's wait, so they travel during that read's walk; read k's own wait (vmcnt 0)
    // then finds them landed, and only the walk's rounds wait on memory.
    const long long kstep = (long long)gridDim.x * wpb;
    auto region_of = [&](long long k) { return a.band_region + ((k >> 1) - a.band_pair_lo) * a.band_stride; };
    auto load_hdr = [&](long long kk, unsigned* dst) {   // header and captures: the region's first kSlot dwords
        const unsigned char* rg = region_of(kk);
#pragma unroll
        for (int m = 0; m < kSlot; m += 64)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(rg + 4 * (m + lane)),
                                             (__attribute__((address_space(3))) void*)(dst + m), 4, 0, 0);
    };
    auto uni = [](int4 v) {   // the header is wave-uniform: SGPRs, scalar branches
        return make_int4(__builtin_amdgcn_readfirstlane(v.x), __builtin_amdgcn_readfirstlane(v.y),
                         __builtin_amdgcn_readfirstlane(v.z), __builtin_amdgcn_readfirstlane(v.w));
    };
    // read kk's length and byte offset from its header slot (kk & 1: read B of the pair)
    auto read_of = [&](const unsigned* hb, long long kk, int* Lb, long long* off) {
        const int4 hr = uni(*(const int4*)(hb + 4)), ho = uni(*(const int4*)(hb + 8));
        const bool hB = (kk & 1) != 0;
        *Lb = hB ? hr.w : hr.z;
        *off = hB ? (long long)(((unsigned long long)(unsigned)ho.w << 32) | (unsigned)ho.z)
                  : (long long)(((unsigned long long)(unsigned)ho.y << 32) | (unsigned)ho.x);
    };
    auto load_bytes = [&](long long off, int Lb, unsigned char* dst) {   // Lb <= rcap
        const unsigned char* raw = a.reads + off;
        const int ms = (int)((uintptr_t)raw & 3);
        for (int m = 0; m < Lb + ms; m += 256)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(raw - ms + m + 4 * lane),
                                             (__attribute__((address_space(3))) void*)(dst + m), 4, 0, 0);
    };
    // read k once its header (hb: pair header + captures) and bytes (rbuf) are in LDS and have landed
    auto process = [&](long long k, const int4 hdr, const int4 hr, const unsigned* cw, int h, long long rd, int Lb,
                       long long off, unsigned char* rbuf) {
        if (W < kBandDiags && a.redo_flags && lane == 0) a.redo_flags[k] = 0;   // give_up may set it
        // a pair of one read (the seeded list's padding, the 32-diagonal level's hole): its first position
        if (W >= kBandDiags && (k & 1) && hr.x == hr.y) {
            seed_done(k);   // (its flag: the pair's first position decides)
            return;
        }
        if (Lb <= 0) {
            if (lane == 0) {
                Stat z = {};
                z.flags = FLAG_EMPTY;
                a.stats[rd] = z;
                if (a.ops) a.nops[rd] = 0;
            }
            return;
        }
        if (hdr.z & kPairInactive) {   // too long, or the pair's lengths do not fit the band
            give_up(k, rd, true);
            return;
        }
        const int dlo = hdr.y;
        const unsigned char* region = region_of(k);
        if (Lb > rcap) {   // not reached: rcap covers the band length cap
            give_up(k, rd, false);
            return;
        }
        const int mis = (int)((uintptr_t)(a.reads + off) & 3);
        const int tau0 = hdr.x;
        // start cell: the last cell of each band diagonal is on the last row or column
        unsigned k32 = 0u;
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            if (lane + 64 * c >= W) continue;
            const int d = dlo + lane + 64 * c;
            const int iend = La < Lb - d ? La : Lb - d;
            const int ilo = 1 - d > 1 ? 1 - d : 1;
            if (iend >= ilo) {
                const int v = half(cw[c], h) - kBias16 - E * (2 * iend + d);
                const int jend = iend + d;
                const unsigned kk = (iend == La && jend == Lb) ? end_key32(v, 3, 0)
                                    : (jend == Lb ? end_key32(v, 2, iend - 1) : end_key32(v, 1, jend - 1));
                k32 = kk > k32 ? kk : k32;
            }
        }
        int score, ei, ej;
        decode_end(end_key_widen(wave_max_u32(k32)), La, Lb, &score, &ei, &ej);
        score = __builtin_amdgcn_readfirstlane(score);
        ei = __builtin_amdgcn_readfirstlane(ei);
        ej = __builtin_amdgcn_readfirstlane(ej);
        // certificate: every alignment leaving the band scores <= UB < score
        const int dhi = dlo + W - 1;
        int pmax = -1;
        if (dhi < Lb - 1) pmax = max(pmax, min(Lb - dhi - 1, La));
        if (dlo > 1 - La) pmax = max(pmax, min(Lb, La + dlo - 1));
        bool certified = pmax < 0 || score > a.band_maxsub * pmax;
        const bool bad_code = (hdr.z & (h ? REGION_BAD_B : REGION_BAD_A)) != 0;
        if (W >= kBandDiags && (hdr.z & REGION_SEEDED) && !certified) {
            // Seeded band: every exact hit of the read's nb disjoint 16-base blocks
            // lies on diagonals [smin, smax] inside the band.  An alignment with a cell outside the
            // band either has a block paired as an exact match -- on one of those diagonals, so its
            // gaps shift it by >= dexit diagonals: it scores <= m Lb - O - (dexit - 1) E -- or has
            // none: each block then loses >= m (an unpaired base, a mismatch, or a gap opened
            // inside it, O >= m), <= m (Lb - nb).  Plain reads and amplicon, EDNAFULL 5 / -4.
            const int32_t si = a.seed_info[rd];
            const int smin = seed_dmin(si), smax = seed_dmax(si), nb = seed_blocks(si);
            const int dexit = min(smin - dlo + 1, dhi - smax + 1);
            const int m = a.band_maxsub;
            const bool plainr = amp_acgt && !(hdr.z & (h ? (REGION_BAD_B | REGION_NP_B) : (REGION_BAD_A | REGION_NP_A)));
            const bool pen_ok = a.gap_open >= m && a.gap_open >= a.gap_extend && a.gap_extend >= 0;
            certified = plainr && seed_valid(si) && dexit >= 1 && pen_ok && score > m * (Lb - nb) &&
                        score > m * Lb - a.gap_open - (dexit - 1) * a.gap_extend;
            const int32_t si2 = a.seed_info2 ? a.seed_info2[rd] : 0;
            if (!certified && plainr && seed_valid(si) && seed2_valid(si2) && dexit >= 1 && pen_ok) {
                // Refined (round 5): a block not paired as an exact match loses >= m when it can sit
                // in a free end gap (the first and the last block), else >= w = min(m + x, O, m + O / 2)
                // -- a mismatch, a deletion opened inside it, or unpaired bases in an insertion whose
                // open it shares with at most one neighbouring block.  An alignment with a cell outside
                // the band pairs (a) no block exactly: every block loses; (b) blocks on one diagonal only:
                // the others lose and it moves >= d_exit diagonals; (c) blocks on two diagonals: it also
                // pays the cheapest move between them (seed_info2).  S above all three bounds.
                const int x = 4 * (m / 5), O = a.gap_open;
                const int w = min(min(m + x, O), m + O / 2);
                auto lose = [&](int k) { return w * max(0, k - 2) + m * min(k, 2); };
                const int ex = O + (dexit - 1) * a.gap_extend;
                const int ba = lose(nb);
                const int bb = ex + lose(max(0, nb - seed2_cmax(si2)));
                const int bc = seed2_shift(si2) >= 0xffff ? (1 << 30) : ex + seed2_shift(si2) + lose(seed2_n0(si2));
                const int loss = m * Lb - score;
                certified = loss < ba && loss < bb && loss < bc;
            }
        }
        if (!certified && !bad_code && score > a.band_maxsub * pmax - a.gap_open) {
            // Refined bound: an alignment leaving the band with an internal gap pays at
            // least the gap open, so it scores <= maxsub * pmax - O < score; one without
            // internal gaps is a single diagonal d (free end gaps), paired over its whole
            // overlap P(d): its score S_d is computed exactly, for the few diagonals beyond
            // the band with maxsub * P(d) >= score (P falls by one per diagonal: at most
            // about two per side, as score > maxsub * (pmax - 2)).
            certified = band_single_diagonals_below(a, amp_lds, rbuf + mis, La, Lb, dlo, dhi, score, lane);
        }
        if (bad_code || !certified) {
            give_up(k, rd, !bad_code);   // IUPAC codes: no band helps
            return;
        }
        // Single-diagonal fast path: when the start cell's score equals the plain sum of
        // substitution scores down its diagonal to the matrix edge, D(ei, ej), the
        // traceback is that diagonal (M(i, j) >= D(i, j) everywhere, so H = M = D on
        // each of its cells, and M wins ties), with the end gaps around it: no band bits
        // are read.  Reads with substitutions only (most non-identical reads) take it.
        int nruns;
        const int nd = min(ei, ej);
        const bool plain = amp_acgt && !(hdr.z & (h ? (REGION_BAD_B | REGION_NP_B) : (REGION_BAD_A | REGION_NP_A)));
        // a plain read's diagonal sums to m nd - (m + x) k for its k mismatches: a score not of that
        // form cannot be the diagonal's (reads with an indel: the test's loop is skipped)
        const int dres = a.band_maxsub * nd - score;
        const bool maybe_diag = !plain || (dres >= 0 && dres % (9 * sc5) == 0);
        int dsum = 0;
        unsigned cnt = 0u;   // identical | similar << 10 | gap columns << 20 of the diagonal (band_emit's counts)
        for (int t = lane; maybe_diag && t < nd; t += 64) {
            const unsigned char ca = amp_lds[ei - 1 - t], cb = rbuf[mis + ej - 1 - t];
            const int sc = sub_of(ca, cb);
            dsum += sc;
            const bool gapc = ca == '-' || cb == '-';   // an input '-' prints as a gap (CORE:1846)
            const bool id = !gapc && upcase(ca) == upcase(cb);
            const bool sim = !gapc && (id || sc > 0);
            cnt += (unsigned)id | ((unsigned)sim << 10) | ((unsigned)gapc << 20);
        }
        const bool diag = maybe_diag && wave_sum(dsum) == score;
        if (diag) {
            const bool endg = (ei == La && ej < Lb) || (ej == Lb && ei < La);
            const int lead = max(ei, ej) - nd;   // leading gap run (Y when ei > nd, X when ej > nd)
            if (lane == 0) {
                int q = 0;
                if (ei == La && ej < Lb) runs[q++] = ((unsigned)RUN_X << 28) | (unsigned)(Lb - ej);
                else if (ej == Lb && ei < La) runs[q++] = ((unsigned)RUN_Y << 28) | (unsigned)(La - ei);
                runs[q++] = ((unsigned)RUN_M << 28) | (unsigned)nd;
                if (ei > nd) runs[q++] = ((unsigned)RUN_Y << 28) | (unsigned)(ei - nd);
                else if (ej > nd) runs[q++] = ((unsigned)RUN_X << 28) | (unsigned)(ej - nd);
            }
            nruns = 1 + (int)endg + (lead > 0);
            if (a.ops && nd < 1024) {
                // ops output: the record comes from the diagonal's counts; no emit pass
                lds_fence();
                store_ops(a, rd, runs, nruns, lane);
                const unsigned t = wave_sum_u32(cnt);
                if (lane == 0) {
                    const int endlen = endg ? (ei == La ? Lb - ej : La - ei) : 0;
                    Stat r;
                    r.aln_len = nd + endlen + lead;
                    r.n_ident = (int)(t & 1023u);
                    r.n_sim = (int)((t >> 10) & 1023u);
                    r.n_gaps = (int)(t >> 20) + endlen + lead;
                    r.score = score;
                    r.end_i = ei;
                    r.end_j = ej;
                    r.flags = 0;
                    a.stats[rd] = r;
                }
                lds_fence();
                seed_done(k);
                return;
            }
        } else {
            const unsigned* bits = (const unsigned*)(region + kHdrBytes + kCapBytes);
            const int tb0 = kBK - dlo + 2 - tau0;
            int tot[3];
            nruns = band_walk_runs2<NW_BAND_WALK_CPL, W>(bits, a.band_words, La, Lb, ei, ej, dlo, tb0, h, runs,
                                                         kBandRunsCap, lane, a.gap_open, a.gap_extend, tot);
            // ops output, plain read: the record from the runs and the score (score = m id - x (M - id) -
            // paid gaps), no emit pass; similar pairs are the identical ones
            const int idn = score + tot[2] + 4 * sc5 * tot[0];
            if (a.ops && plain && nruns >= 0 && idn >= 0 && idn % (9 * sc5) == 0) {
                lds_fence();
                store_ops(a, rd, runs, nruns, lane);
                if (lane == 0) {
                    Stat r;
                    r.aln_len = tot[0] + tot[1];
                    r.n_ident = idn / (9 * sc5);
                    r.n_sim = r.n_ident;
                    r.n_gaps = tot[1];
                    r.score = score;
                    r.end_i = ei;
                    r.end_j = ej;
                    r.flags = 0;
                    a.stats[rd] = r;
                }
                lds_fence();
                seed_done(k);
                return;
            }
        }
        if (nruns < 0) {
            give_up(k, rd, true);
            return;
        }
        lds_fence();
        auto sim = [&](int ai, int code) { return (int)((rowpos[ai] >> code) & 1u); };
        if (a.ops) {
            store_ops(a, rd, runs, nruns, lane);
            band_emit<false>(runs, nruns, amp_lds, rbuf + mis, lut_lds, sim, rows, row, nullptr, 0, score, ei, ej,
                             a.stats + rd, lane);
        } else {
            band_emit<true>(runs, nruns, amp_lds, rbuf + mis, lut_lds, sim, rows, row, a.out + rd * 3 * a.stride, a.stride,
                            score, ei, ej, a.stats + rd, lane);
        }
        lds_fence();
        seed_done(k);
    };
    if constexpr (LN && W < kBandDiags) {
        if (a.ops) {
            walk_lanes<W>(a, klo, khi, wb, amp_lds, amp_acgt, sc5, [&](long long kq) {
                // a read the lane walk leaves to the wave path: its header, captures and bytes into
                // LDS, then the per-read body
                load_hdr(kq, hbufs);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const int4 hdr = uni(*(const int4*)hbufs), hr = uni(*(const int4*)(hbufs + 4));
                unsigned cw[CW];
#pragma unroll
                for (int c = 0; c < CW; ++c) cw[c] = lane + 64 * c < W ? hbufs[kHdrBytes / 4 + lane + 64 * c] : 0u;
                const int h = (int)(kq & 1);
                const long long rd = h ? hr.y : hr.x;
                int Lb;
                long long off;
                read_of(hbufs, kq, &Lb, &off);
                if (Lb > 0 && Lb <= rcap) load_bytes(off, Lb, rbufs);
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                process(kq, hdr, hr, cw, h, rd, Lb, off, rbufs);
            });
            if (redo_n) flush_redo();
            if (fb_n) flush_fb();
            return;
        }
    }
    long long k = klo + (long long)blockIdx.x * wpb + wave;
    int it = 0;   // parity of the slots holding read k's header and bytes
    if (k < khi) {   // the pipeline's start: read k's header, then its bytes and the next header
        load_hdr(k, hbufs);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int Lb0;
        long long off0;
        read_of(hbufs, k, &Lb0, &off0);
        if (Lb0 > 0 && Lb0 <= rcap) load_bytes(off0, Lb0, rbufs);
        if (k + kstep < khi) load_hdr(k + kstep, hbufs + kSlot);
    }
    for (; k < khi; k += kstep, it ^= 1) {
        const unsigned* hb = hbufs + it * kSlot;   // landed: the previous read's wait
        unsigned char* rbuf = rbufs + it * (rcap + 256);
        const int4 hdr = uni(*(const int4*)hb), hr = uni(*(const int4*)(hb + 4));
        unsigned cw[CW];
#pragma unroll
        for (int c = 0; c < CW; ++c) cw[c] = lane + 64 * c < W ? hb[kHdrBytes / 4 + lane + 64 * c] : 0u;
        const int h = (int)(k & 1);
        const long long rd = h ? hr.y : hr.x;
        int Lb;
        long long off;
        read_of(hb, k, &Lb, &off);
        // every load issued for this read has landed (its bytes, the next read's header), and the
        // header reads above are done (lgkmcnt); the next read's bytes and the header after it go
        // out now, into the slots the previous read used and this read's header slot
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        if (k + kstep < khi) {
            unsigned* hn = hbufs + (it ^ 1) * kSlot;
            int Lbn;
            long long offn;
            read_of(hn, k + kstep, &Lbn, &offn);
            if (Lbn > 0 && Lbn <= rcap) load_bytes(offn, Lbn, rbufs + (it ^ 1) * (rcap + 256));
            if (k + 2 * kstep < khi) load_hdr(k + 2 * kstep, hbufs + it * kSlot);   // this read's header is in registers
        }
        process(k, hdr, hr, cw, h, rd, Lb, off, rbuf);
    }
    if constexpr (W > kBandDiags) {
        // the wide level's list entries past its region's capacity: straight to the exact kernel
        const long long nb = (long long)*a.band_count;
        for (long long k2 = khi + (long long)blockIdx.x * wpb + wave; k2 < count; k2 += kstep)
            if (!((k2 & 1) && band_list_read(a, k2 - 1, nb) == band_list_read(a, k2, nb))) give_up(k2, band_list_read(a, k2, nb), false);
    }
    if (redo_n) flush_redo();
    if (fb_n) flush_fb();
}

// ---- host-side helpers -------------------------------------------------------
int band_walk_lds_bytes(int La, int wpb, int lb_max, int W) {
    return band_walk_shared_bytes(La) + wpb * band_walk_wave_bytes(La, lb_max, W);
}

static void launch_band_walk(int W, bool lanes, const KernelArgs& a, const LaunchCfg& walk, hipStream_t s) {
    if (lanes)
        hipLaunchKernelGGL((nw_band_walk<16, true>), dim3(walk.grid), dim3(64 * walk.wpb), walk.lds_bytes, s, a);
    else if (W == 16)
        hipLaunchKernelGGL(nw_band_walk<16>, dim3(walk.grid), dim3(64 * walk.wpb), walk.lds_bytes, s, a);
    else if (W == 32)
        hipLaunchKernelGGL(nw_band_walk<32>, dim3(walk.grid), dim3(64 * walk.wpb), walk.lds_bytes, s, a);
    else
        hipLaunchKernelGGL(nw_band_walk<kWideDiags>, dim3(walk.grid), dim3(64 * walk.wpb), walk.lds_bytes, s, a);
}

static hipError_t band_walk_occupancy(int W, int wpb, int lds, int* blocks) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(
        blocks,
        W == 16 ? (const void*)nw_band_walk<16> : (W == 32 ? (const void*)nw_band_walk<32> : (const void*)nw_band_walk<kWideDiags>),
        64 * wpb, lds);
}

hipError_t band_occupancy(int W, int fill_wpb, int walk_wpb, int fill_lds, int walk_lds, int* fill_blocks,
                          int* walk_blocks) {
    hipError_t e = band_fill_occupancy(W, fill_wpb, fill_lds, fill_blocks);
    return e != hipSuccess ? e : band_walk_occupancy(W, walk_wpb, walk_lds, walk_blocks);
}

hipError_t launch_band(int W, const KernelArgs& a, const LaunchCfg& fill, const LaunchCfg& walk, hipStream_t s,
                       hipEvent_t after_fill) {
    // the lane walk (and the stop summary its fill writes for it) when the context asked for it
    KernelArgs al = a;
    al.band_summ = W == 16 && a.ops && a.band_summ;
    launch_band_fill(W, al.band_summ, al.band_summ ? al : a, fill, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (after_fill && (e = hipEventRecord(after_fill, s)) != hipSuccess) return e;
    launch_band_walk(W, al.band_summ, al.band_summ ? al : a, walk, s);
    return hipGetLastError();
}

}  // namespace nw
