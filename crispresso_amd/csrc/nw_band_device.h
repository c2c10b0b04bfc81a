// nw_band_device.h -- certified diagonal-band DP: the default aligner path.
//
// The exact kernel (nw_kernel.hip) fills every cell of the La x Lb matrix.  A
// CRISPResso read is a near-copy of its amplicon, so its optimal alignments stay
// within a few diagonals of the main one.  These kernels fill only a band of
// kBD = 32 diagonals [dlo, dlo + 31] around [min(0, Lb - La), max(0, Lb - La)]
// and then PROVE that the result is the full DP's result:
//
//   A path that visits a cell on diagonal d = j - i has left |d| residues of one
//   sequence unpaired on the way there, so it pairs at most
//       min(Lb - d, La)  (d > 0)   or   min(Lb, La + d)  (d < 0)
//   residues, and every pair scores at most the matrix maximum (EDNAFULL: 5) while
//   gaps cost >= 0.  Hence every alignment touching a diagonal outside the band
//   scores at most UB = maxsub * max(min(Lb - dhi - 1, La), min(Lb, La + dlo - 1)).
//   If the best in-band score S > UB, every optimal alignment -- and every
//   alignment tied with one -- lies inside the band.  All values the traceback
//   compares (the predecessor states of an optimal path, the start cells of the
//   last row/column with score S, the open/extend choices along the path) are
//   then values of in-band paths, which the banded DP computes exactly; values it
//   under-estimates are strictly below S and below the compared optimum.  So the
//   banded traceback, with the same tie rules, is the full DP's
//   traceback, bit for bit.
//
// Reads that fail the certificate (S <= UB: chimeras, off-target, large indels),
// whose pair's lengths span more than the band, or that hold IUPAC codes other
// than N go to the exact int32 kernel's fallback list.
//
// Layout / schedule:
//   * reads are sorted by length on the device (nw_band_segsort: 4096-read segments
//     sorted in LDS, placed by look-back); DP-list positions (2g, 2g+1) form pair g,
//     packed in int16x2
//     (read A low, B high) on one band that holds both reads' start and end
//     diagonals; the sort keeps the wavefront's pairs at similar lengths;
//   * one read pair per 16-lane DPP row, 4 pairs per wavefront; lane q owns
//     diagonals d0 = dlo + 2q and d0 + 1; the wave sweeps anti-diagonals t = i + j
//     and at each step every lane computes one cell (the diagonal whose parity
//     matches t).  Predecessors: diag = own lane two steps back, up / left = own
//     lane or its row neighbour one step back (DPP row_shr:1 / row_shl:1; the row
//     edge reads -inf = outside the band).  Groups run at tau = t - dlo + kBK, so
//     the step parity is wave-uniform;
//   * biased recurrence: values carry + t * E (t = anti-diagonal step), so X = max(Mo,
//     X_left), Y = max(Mo, Y_up) with no "- extend"; the diagonal's + 2E is in
//     the score table; Mo = M - (O - E);
//   * 4 traceback bits per cell and read, 4 steps per dword (byte planes of the
//     sign bits); per pair region: header, the M of each
//     diagonal's last cell (= the last row / last column cells), bits in tiles
//     [words / 4][lanes][4 words]: the fill writes 16 steps of a pair's lanes as one
//     contiguous dwordx4 row, an M run of the walk reads 16 steps of its diagonal
//     pair with one dwordx4 per lane;
//   * nw_band_walk: one wavefront per read: start cell from the W captures,
//     certificate, the run-based walk of nw_common.h over the band, strings.
//
// This header: what more than one band stage uses (nw_band.hip: classify; nw_band_sort.hip,
// nw_band_fill.hip, nw_band_walk.hip) -- the packed-halfword and DPP helpers, the band's
// geometry and region layout, the band lists -- and the stages' launchers for each other.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_common.h"

namespace nw {

namespace {

typedef short s16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ s16x2 as_v(unsigned u) { return __builtin_bit_cast(s16x2, u); }
__device__ __forceinline__ unsigned as_u(s16x2 v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ unsigned pk(int lo, int hi) { return ((unsigned)lo & 0xffffu) | ((unsigned)hi << 16); }
__device__ __forceinline__ int half(unsigned w, int h) { return (int)(short)(w >> (16 * h)); }
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
// The fill keeps every value + kBias16 (unsigned, -inf = 0): max is v_pk_max_u16 and
// a DPP lane without a source reads 0 (bound_ctrl) -- no "old" operand to set up.
// Sums and differences are the same bits as in the signed domain.
constexpr int kBias16 = 16384;
__device__ __forceinline__ unsigned max2(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a),
                                                                  __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ unsigned add2(unsigned a, unsigned b) { return as_u(as_v(a) + as_v(b)); }
__device__ __forceinline__ unsigned sub2(unsigned a, unsigned b) { return as_u(as_v(a) - as_v(b)); }
// DPP within 16-lane rows by S lanes; a lane without a source reads 0 (= -inf:
// outside the band).  S = 2 when two read pairs share a row (interleaved lanes).
template <int S>
__device__ __forceinline__ unsigned row_shr(unsigned v) {
    return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x110 + S, 0xf, 0xf, true);
}
template <int S>
__device__ __forceinline__ unsigned row_shl(unsigned v) {
    return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x100 + S, 0xf, 0xf, true);
}

}  // namespace

// ---- geometry shared by fill, walk and host --------------------------------------
// Band of a read pair: it must hold both reads' start (diagonal 0's neighbourhood)
// and end diagonals (Lb - La); the spare diagonals are split evenly.  An empty
// read imposes nothing.  False when the band cannot hold them or both are empty.
__host__ __device__ inline bool band_geometry2(int La, int LbA, int LbB, int* dlo, int W = kBandDiags) {
    int lo0 = 0, hi0 = 0;
    if (LbA > 0) { lo0 = min(lo0, LbA - La); hi0 = max(hi0, LbA - La); }
    if (LbB > 0) { lo0 = min(lo0, LbB - La); hi0 = max(hi0, LbB - La); }
    const int extra = W - (hi0 - lo0 + 1);
    *dlo = 0;
    if ((LbA <= 0 && LbB <= 0) || extra < 0) return false;
    *dlo = lo0 - extra / 2;
    return true;
}
__host__ __device__ inline bool band_geometry(int La, int Lb, int* dlo) { return band_geometry2(La, Lb, Lb, dlo); }

namespace {

// band of W diagonals: L = W / 2 lanes per read pair, PR pairs per 16-lane DPP row
// (interleaved: pair = lane % PR, q = lane / PR within the row), PW pairs per wavefront.
// W = kWideDiags (the wide level): one pair per wavefront, lane q = the lane, neighbours
// through the wave-wide DPP shifts (wave_shr:1 / wave_shl:1; lane 0 / 63 read -inf).
template <int W> struct BandGeo {
    static constexpr bool Wide = W > 32;
    static constexpr int L = W / 2;
    static constexpr int PR = Wide ? 1 : 16 / L;
    static constexpr int PW = Wide ? 1 : 4 * PR;
    static constexpr int CapBytes = W * 4;
    __device__ static int q_of(int lane) { return Wide ? lane : (lane & 15) / PR; }
    __device__ static int grp_of(int lane) { return Wide ? 0 : (lane >> 4) * PR + (lane & 15) % PR; }
    __device__ static int src_of(int p) { return Wide ? 0 : (p / PR) * 16 + p % PR; }   // lane q = 0 of pair p
    // the left / upper neighbour's value one step back (0 = -inf past the band's edge)
    __device__ static unsigned shr(unsigned v) {
        if constexpr (Wide) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x138, 0xf, 0xf, true);   // wave_shr:1
        else return row_shr<PR>(v);
    }
    __device__ static unsigned shl(unsigned v) {
        if constexpr (Wide) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x130, 0xf, 0xf, true);   // wave_shl:1
        else return row_shl<PR>(v);
    }
};
constexpr int kBK = 64;               // tau = t - dlo + kBK: >= 0 and even
constexpr int kAPad = 80;             // amplicon codes: index i + kAPad, i in [-17, La + 48] (wide level: [-66, La + 102])
constexpr int kJPad = 95;             // pair codes: index j + kJPad, j in [-48, La + 80] (wide: [-66, La + 196]); j = 1 is 4-aligned
constexpr int kPadCode = 5;           // lut6: A T G C N pad
constexpr int kTabRows = NCODE;       // amplicon rows: every EDNAFULL code (IUPAC too) + pad/unknown
constexpr int kTabBytes = 2448;       // [17][36] packed scores
constexpr int kHdrBytes = 48;         // {tau0, dlo, flags, -}, {ra, rb, LbA, LbB}, {offA, offB}
constexpr int kPairInactive = 4;      // header flag: the pair was not filled (walk: empty / fallback)

__host__ __device__ inline int band_acd_elems(int La) { return La + kAPad + 112; }
__host__ __device__ inline int band_pcs(int La, int W) { return align16(La + kJPad + (W > 32 ? 208 : 96)); }

}  // namespace

// reads longer than La + W - 1 never enter a level of W diagonals (KernelArgs::band_lb_cap)
__host__ __device__ inline int band_words(int La, int Lb_max, int W = kBandDiags) {
    const int Lbm = Lb_max < La + W - 1 ? Lb_max : La + W - 1;
    return (((La + Lbm + 80) / 4 + 2) + 3) & ~3;   // column length: whole dwordx4 of the walk
}
// Stop summary (the first level, KernelArgs::band_summ): after a pair's tiles, per lane (diagonal
// pair q) one byte per 16 words (64 steps, four tile rows) -- the OR of the block's "M < max"
// bits, read A's four sub-steps in the low nibble, read B's in the high -- padded to 16 bytes
// per lane.  A lane walk's M run skips the blocks whose bits for its read and diagonal are clear.
__host__ __device__ inline int band_summ_bytes(int NW) { return ((((NW + 15) >> 4) + 15) & ~15); }

__host__ __device__ inline int64_t band_region_stride(int La, int Lb_max, int W) {
    const int NW = band_words(La, Lb_max, W > kBandDiags ? W : kBandDiags);
    return ((int64_t)kHdrBytes + 4 * W + (int64_t)NW * (W / 2) * 4 + (int64_t)(W / 2) * band_summ_bytes(NW) + 255) &
           ~(int64_t)255;
}

// ---- device helpers of more than one stage, the band lists ------------------------
// (classify's byte compares, the lane walk's count_mis)
__device__ __forceinline__ unsigned zero_bytes(unsigned x) {   // 0x80 in each zero byte of x
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

// Overlap of diagonal d = j - i (pairs of the alignment that stays on it).
__device__ __forceinline__ int diag_pairs(int La, int Lb, int d) { return d >= 0 ? min(La, Lb - d) : min(Lb, La + d); }

// DP list of the traceback pass: band_order[0, *band_count).
// The wide level (a.band_from_work) reads the exact kernel's work list instead: the reads the
// narrower levels gave up on, then (direct hand-off) the first level's redo list; there
// a.band_count = a.work_count.
// The wide level's list ends with the seeded reads (the segment sort's seeded list, sorted by
// their hits' diagonals, so a pair's two reads share a band).
// The 32-diagonal level with the seeded list (KernelArgs::seed_l2 == 1): its own list (the redo
// list, none when the direct hand-off gave it to the wide level; as the only level, the sorted DP
// list), then, from the next even position, the seeded list -- an
// odd count before it leaves one hole (read by no walk), so no pair mixes a seeded read with another.
__device__ __forceinline__ long long l2_redo_n(const KernelArgs& a) {
    return redo_direct_taken(a) ? 0ll : (long long)*a.band_count;
}
__device__ __forceinline__ long long l2_seed0(const KernelArgs& a) { return (l2_redo_n(a) + 1) & ~1ll; }
// Wide first (KernelArgs::wf_list): the launch with wf_take = 1 reads that list when the chunk takes it
// (wf_taken), nothing otherwise; a launch over the sorted DP list (a.wf_list set: the first level, the
// redo compaction) reads band_order[0, *band_count - *wf_count) and, unless that launch took it, the
// wide-first list after it.
__device__ __forceinline__ long long band_list_count(const KernelArgs& a) {
    if (a.wf_take == 1) return wf_taken(a) ? (long long)*a.wf_count : 0ll;
    if (a.band_from_work) return exact_work_count(a) + (a.seed_list ? (long long)*a.seed_count : 0ll);
    if (a.seed_l2 == 1) return l2_seed0(a) + (long long)*a.seed_count;
    return (long long)*a.band_count - (wf_taken(a) ? (long long)*a.wf_count : 0ll);
}
__device__ __forceinline__ long long band_list_read(const KernelArgs& a, long long k, long long nb) {
    if (a.wf_take == 1) return (long long)a.wf_list[k];
    if (a.band_from_work) {
        if (k < nb) return a.work_list[k];
        const long long nr = redo_direct_taken(a) ? (long long)*a.redo_count : 0ll;
        return k < nb + nr ? (long long)a.redo_list[k - nb] : (long long)a.seed_list[k - nb - nr];
    }
    if (a.seed_l2 == 1) {
        const long long nr = l2_redo_n(a), s0 = (nr + 1) & ~1ll;
        if (k >= s0) return (long long)a.seed_list[k - s0];
        if (k >= nr) --k;   // the hole: its pair's read A again (the pair holds one read)
    }
    if (a.wf_list) {
        const long long nbo = nb - (long long)*a.wf_count;
        if (k >= nbo) return (long long)a.wf_list[k - nbo];
    }
    return (long long)a.band_order[k];
}

// ---- the stages' launchers for each other (host) ----------------------------------
// launch_band_sort (nw_band_sort.hip): classify and the deferred certificates (nw_band.hip) ahead of the sort
void launch_band_classify(const KernelArgs& a, hipStream_t s);
// launch_band / band_occupancy (nw_band_walk.hip): the fill ahead of the walk; summ: nw_band_fill<16, true>
void launch_band_fill(int W, bool summ, const KernelArgs& a, const LaunchCfg& fill, hipStream_t s);
hipError_t band_fill_occupancy(int W, int wpb, int lds, int* blocks);

}  // namespace nw
