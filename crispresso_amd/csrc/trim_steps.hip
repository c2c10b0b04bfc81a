// Trimmomatic 0.33's quality and crop steps on gfx950 (include/crispr_trim.h: nwt_step,
// nwt_trim_program): LEADING, TRAILING, SLIDINGWINDOW, CROP, HEADCROP, AVGQUAL, MINLEN, in the
// order given, on the device buffers the clip kernel has just read.  tests/trim_steps_model.py
// restates the steps.
//
// One wavefront per read (the two mates of a pair are independent reads).  The read's qualities
// minus 33, zero where the base is 'N', are staged once in LDS as bytes: lane l takes dwords
// l, l + 64, ... of the quality and the sequence line (aligned loads shifted to the read's first
// byte, 256 B a step, coalesced).  The record is a window (start, len, alive) of the staged read,
// the same in every lane, so every step is a uniform branch and the program (kernel arguments,
// scalar loads) is walked once per read.
//   * LEADING / TRAILING: strips of 64 aligned LDS dwords (256 bases) from the window's end in
//     question; a lane turns its dword into a 4-bit mask of bases inside the window that reach the
//     threshold, one ballot finds the lane, ffs / clz the base.  The first strip usually decides.
//   * AVGQUAL: masked byte sums per lane, a wave reduction.
//   * SLIDINGWINDOW: prefix sums of the staged qualities (from the read's first base, so they do
//     not depend on the window) are extended 256 bases at a time -- a lane's four partial sums, a
//     wave inclusive scan of the lane totals, the running base carried to the next strip -- and
//     kept in LDS, shared by every SLIDINGWINDOW step of the program.  A window's total is the
//     difference of two of them; 64 windows a ballot, the first failing one ends the search and
//     no further prefix is formed.  The walk back over low-quality bases is TRAILING's scan with
//     a float predicate.
// Totals stay below 2^24 (4096 bases of at most 93), so their float32 images are exact.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trim_device.h"

namespace nwt {
namespace {

__device__ __forceinline__ void wsync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// Dword k of the nb bytes at p (4k < nb): bytes 4k .. 4k + 3; those at or past nb are undefined.
// Aligned loads only, and only of words that hold one of the nb bytes.
__device__ __forceinline__ uint32_t load_dword(const uint8_t* p, int k, int nb) {
    const uintptr_t a = (uintptr_t)p + 4 * (uintptr_t)k;
    const unsigned m = (unsigned)(a & 3);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(a - m);
    const int left = nb - 4 * k;
    uint32_t v = w[0] >> (8 * m);
    if (m && left > 4 - (int)m) v |= w[1] << (32 - 8 * m);
    return v;
}

__device__ __forceinline__ int clamp04(int x) { return x < 0 ? 0 : x > 4 ? 4 : x; }
// bit k set: position pos0 + k lies in [lo, hi)
__device__ __forceinline__ unsigned range4(int pos0, int lo, int hi) {
    return ((1u << clamp04(hi - pos0)) - 1u) & ~((1u << clamp04(lo - pos0)) - 1u);
}

struct AtLeast {   // q >= t
    int t;
    __device__ __forceinline__ unsigned operator()(uint32_t w) const {
        return (unsigned)((int)(w & 255u) >= t) | (unsigned)((int)((w >> 8) & 255u) >= t) << 1 |
               (unsigned)((int)((w >> 16) & 255u) >= t) << 2 | (unsigned)((int)(w >> 24) >= t) << 3;
    }
};
struct NotBelow {   // !((float)q < r)
    float r;
    __device__ __forceinline__ unsigned operator()(uint32_t w) const {
        return (unsigned)!((float)(w & 255u) < r) | (unsigned)!((float)((w >> 8) & 255u) < r) << 1 |
               (unsigned)!((float)((w >> 16) & 255u) < r) << 2 | (unsigned)!((float)(w >> 24) < r) << 3;
    }
};

// The first position in [lo, hi) of the staged read whose quality satisfies pred, or -1.
template <class P>
__device__ int scan_first(const uint32_t* zq, int lo, int hi, int lane, P pred) {
    for (int d0 = lo >> 2; 4 * d0 < hi; d0 += 64) {
        const int d = d0 + lane;
        unsigned m = 0;
        if (4 * d < hi) m = pred(zq[d]) & range4(4 * d, lo, hi);
        const uint64_t b = __ballot(m != 0);
        if (b) {
            const int fl = (int)__builtin_ctzll(b);
            const unsigned mm = (unsigned)__shfl((int)m, fl);
            return __builtin_amdgcn_readfirstlane(4 * (d0 + fl) + (int)__builtin_ctz(mm));
        }
    }
    return -1;
}

// The last position in [lo, hi), or -1.
template <class P>
__device__ int scan_last(const uint32_t* zq, int lo, int hi, int lane, P pred) {
    if (hi <= lo) return -1;
    for (int dt = (hi - 1) >> 2; 4 * dt + 3 >= lo; dt -= 64) {
        const int d = dt - 63 + lane;
        unsigned m = 0;
        if (d >= 0 && 4 * d + 3 >= lo) m = pred(zq[d]) & range4(4 * d, lo, hi);
        const uint64_t b = __ballot(m != 0);
        if (b) {
            const int fl = 63 - (int)__builtin_clzll(b);
            const unsigned mm = (unsigned)__shfl((int)m, fl);
            return __builtin_amdgcn_readfirstlane(4 * (dt - 63 + fl) + 31 - (int)__builtin_clz(mm));
        }
    }
    return -1;
}

// The sum of the qualities at [lo, hi).
__device__ int sum_range(const uint32_t* zq, int lo, int hi, int lane) {
    int s = 0;
    for (int d = (lo >> 2) + lane; 4 * d < hi; d += 64) {
        const unsigned r = range4(4 * d, lo, hi);
        const uint32_t w = zq[d];
        s += (int)((r & 1u ? w & 255u : 0u) + (r & 2u ? (w >> 8) & 255u : 0u) + (r & 4u ? (w >> 16) & 255u : 0u) +
                   (r & 8u ? w >> 24 : 0u));
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return __builtin_amdgcn_readfirstlane(s);
}

__global__ __launch_bounds__(64 * kWpb) void nwt_steps_kernel(const StepsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned char* base = smem + (size_t)wave * ((size_t)5 * a.lb + 16);
    int32_t* E = (int32_t*)(base + 16);              // E[k] = q[0] + ... + q[k] of the staged read; E[-1] = 0
    uint32_t* zq = (uint32_t*)(base + 16 + (size_t)4 * a.lb);   // the staged qualities, 4 to a dword
    if (lane == 0) E[-1] = 0;
    const int64_t reads = a.paired ? 2 * a.n : a.n;
    for (int64_t r = (int64_t)blockIdx.x * a.wpb + wave; r < reads; r += (int64_t)gridDim.x * a.wpb) {
        const int mate = r >= a.n ? 1 : 0;
        const int64_t i = r - (mate ? a.n : 0);
        const int64_t* off = a.off[mate];
        const int64_t o = off[i];
        const int L = __builtin_amdgcn_readfirstlane((int)(off[i + 1] - o));
        int start = 0, len = L;
        bool alive = true;
        const int32_t* keep_in = a.keep_in[mate];
        if (keep_in) {
            len = __builtin_amdgcn_readfirstlane(keep_in[i]);
            alive = len > 0 || L == 0;
        }
        const int ns = alive ? len : 0;   // the window only shrinks: these bases are all a step can see
        wsync();                          // the previous read's readers are done
        {
            const uint8_t* qp = a.qual[mate] + o;
            const uint8_t* sp = a.seq[mate] + o;
            for (int k = lane; 4 * k < ns; k += 64) {
                const uint32_t qw = load_dword(qp, k, ns), sw = load_dword(sp, k, ns);
                uint32_t z = qw - 0x21212121u;   // every byte of the read is >= 33: no borrow into it
                const uint32_t x = sw ^ 0x4e4e4e4eu;   // a zero byte: 'N'
                const uint32_t isn = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);   // 0x80 there
                z &= ~((isn >> 7) * 255u);
                const int left = ns - 4 * k;
                if (left < 4) z &= (1u << (8 * left)) - 1u;
                zq[k] = z;
            }
        }
        wsync();
        int pdone = 0, carry = 0;   // prefix sums exist for dwords [0, pdone); carry = E[4 * pdone - 1]
        for (int s = 0; s < a.n_steps && alive; ++s) {
            const nwt_step st = a.steps[s];
            const int arg = st.arg;
            switch (st.op) {
            case NWT_OP_LEADING: {
                const int p = scan_first(zq, start, start + len, lane, AtLeast{arg});
                if (p < 0) {
                    alive = false;
                } else {
                    len -= p - start;
                    start = p;
                }
                break;
            }
            case NWT_OP_TRAILING: {
                const int p = scan_last(zq, start + 1, start + len, lane, AtLeast{arg});
                if (p < 0)
                    alive = false;
                else
                    len = p - start + 1;
                break;
            }
            case NWT_OP_SLIDINGWINDOW: {
                if (len < arg) {
                    alive = false;
                    break;
                }
                const int nwin = len - arg + 1;
                int found = -1;
                for (int jb = 0; jb < nwin; jb += 64) {
                    const int need = min(start + jb + 63 + arg, start + len);   // bases the 64 windows cover
                    while (4 * pdone < need) {
                        const int d = pdone + lane;
                        const bool in = 4 * d < ns;
                        const uint32_t w = in ? zq[d] : 0u;
                        const int s1 = (int)(w & 255u), s2 = s1 + (int)((w >> 8) & 255u),
                                  s3 = s2 + (int)((w >> 16) & 255u), s4 = s3 + (int)(w >> 24);
                        int x = s4;
                        for (int sh = 1; sh < 64; sh <<= 1) {
                            const int y = __shfl_up(x, sh);
                            if (lane >= sh) x += y;
                        }
                        const int ex = x - s4 + carry;
                        if (in) *(int4*)(E + 4 * d) = make_int4(ex + s1, ex + s2, ex + s3, ex + s4);
                        carry = __builtin_amdgcn_readfirstlane(__shfl(x, 63)) + carry;
                        pdone += 64;
                    }
                    wsync();
                    const int j = jb + lane;
                    bool bad = false;
                    if (j < nwin) bad = (float)(E[start + j + arg - 1] - E[start + j - 1]) < st.R;
                    const uint64_t b = __ballot(bad);
                    if (b) {
                        found = jb + (int)__builtin_ctzll(b);
                        break;
                    }
                }
                if (found == 0) {
                    alive = false;
                    break;
                }
                const int keep = found > 0 ? found + arg - 1 : len;
                const int p = scan_last(zq, start + 1, start + keep, lane, NotBelow{st.r});
                len = p < 0 ? 1 : p - start + 1;
                break;
            }
            case NWT_OP_CROP:
                if (len >= arg) len = arg;
                break;
            case NWT_OP_HEADCROP:
                if (len <= arg) {
                    alive = false;
                } else {
                    start += arg;
                    len -= arg;
                }
                break;
            case NWT_OP_AVGQUAL:
                if (sum_range(zq, start, start + len, lane) < arg * len) alive = false;
                break;
            case NWT_OP_MINLEN:
                if (len < arg) alive = false;
                break;
            default:
                break;
            }
        }
        if (lane == 0) {
            a.start[mate][i] = alive ? start : 0;
            a.keep[mate][i] = alive ? len : -1;
        }
    }
}

}  // namespace

size_t steps_lds_per_wave(int lmax, int32_t* lb) {
    *lb = (lmax + 4 + 15) & ~15;
    return (size_t)5 * *lb + 16;
}

void launch_steps(const StepsArgs& a, unsigned grid, size_t lds) {
    hipLaunchKernelGGL(nwt_steps_kernel, dim3(grid), dim3(64 * a.wpb), lds, nullptr, a);
}

}  // namespace nwt
