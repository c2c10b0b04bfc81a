// group_device.h -- what the stages that group keys in an open-addressing table share
// (nw_alleles.hip, nw_count.hip, nw_regions.hip): the hash's constants and finaliser, the 64-bit
// shuffles, the wavefront election of equal keys, the single-word slot claim, the
// one-atomic-per-wavefront list append, the unaligned-dword load, and the table's geometry on
// the host.  Each stage keeps its own finish_hash / key_hash and its own policy on a full table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

namespace grp {

constexpr uint64_t kPoly = 0x9E3779B97F4A7C15ull;     // odd: a one-dword difference never cancels
constexpr uint64_t kLenMul = 0xC2B2AE3D27D4EB4Full;
constexpr uint64_t kNoSlot = ~0ull;                    // claim_slot: the probe bound was reached

__host__ __device__ inline uint64_t fmix64(uint64_t h) {
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return h;
}

__device__ inline uint64_t shfl64(uint64_t v, int src) {
    const int lo = __shfl((int)(uint32_t)v, src, 64);
    const int hi = __shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

__device__ inline uint64_t shfl_xor64(uint64_t v, int mask) {
    const int lo = __shfl_xor((int)(uint32_t)v, mask, 64);
    const int hi = __shfl_xor((int)(uint32_t)(v >> 32), mask, 64);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

// Dword k of the L bytes at p (4k < L): bytes 4k .. 4k + 3, those at or past L as zero.
// Aligned loads only, and only of words that hold one of the L bytes.
__device__ inline uint32_t load_dword(const uint8_t* p, int64_t k, int64_t L) {
    const uintptr_t a = (uintptr_t)p + 4 * (uintptr_t)k;
    const unsigned m = (unsigned)(a & 3);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(a - m);
    const int64_t left = L - 4 * k;
    const int nb = left < 4 ? (int)left : 4;
    uint32_t v = w[0] >> (8 * m);
    if (m && nb > 4 - (int)m) v |= w[1] << (32 - 8 * m);
    if (nb < 4) v &= (1u << (8 * nb)) - 1u;
    return v;
}

// Among the active lanes of the wavefront, those with equal `key` elect the lowest of them:
// *lead = that lane (the lane itself when inactive); returns the group's size in the elected
// lane and 0 in every other.  At most 64 rounds, one per distinct key.
__device__ inline uint32_t wave_elect(uint64_t key, bool active, int* lead) {
    const int lane = threadIdx.x & 63;
    bool done = !active;
    uint32_t cnt = 0;
    *lead = lane;
    for (int it = 0; it < 64; ++it) {
        const unsigned long long act = __ballot(!done);
        if (!act) break;
        const int l0 = __ffsll((long long)act) - 1;
        const uint64_t k0 = shfl64(key, l0);
        const bool mine = !done && key == k0;
        const unsigned long long same = __ballot(mine);
        if (mine) {
            done = true;
            *lead = l0;
            if (lane == l0) cnt = (uint32_t)__popcll(same);
        }
    }
    return cnt;
}

// Claims the slot of hash h (nonzero) in a table of one 64-bit word a slot, 0 = empty: a relaxed
// load, a 64-bit CAS on an empty slot, linear probing bounded by the table size.  The slot's
// first = min(first, r), its count += cnt: its content is independent of the order of arrival.
// Returns the slot, or kNoSlot when every slot holds another hash.
__device__ inline uint64_t claim_slot(unsigned long long* keys, uint32_t* first, uint32_t* count, uint64_t h, uint32_t r,
                                      uint32_t cnt, int shift, uint64_t cap_mask) {
    uint64_t s = (h * kPoly) >> shift;
    bool ok = false;
    for (uint64_t probe = 0; probe <= cap_mask; ++probe) {      // bounded by the table size
        unsigned long long k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0) k = atomicCAS(&keys[s], 0ull, (unsigned long long)h);
        if (k == 0 || k == h) {
            atomicMin(&first[s], r);
            atomicAdd(&count[s], cnt);
            ok = true;
            break;
        }
        s = (s + 1) & cap_mask;
    }
    return ok ? s : kNoSlot;
}

// The lanes with `flag` reserve one entry each of a list counted by *counter (one atomic per
// wavefront); returns the lane's index in the list (meaningless without flag).
template <class C>
__device__ inline C wave_reserve(bool flag, C* counter) {
    const int lane = threadIdx.x & 63;
    const unsigned long long b = __ballot(flag);
    if (!b) return 0;
    const int lead = __ffsll((long long)b) - 1;
    C at = 0;
    if (lane == lead) at = atomicAdd(counter, (C)__popcll(b));
    return __shfl(at, lead, 64) + (C)__popcll(b & ((1ull << lane) - 1ull));
}

// ---- the host side --------------------------------------------------------------------------

// A table for `keys` keys: a power of two of at least twice the keys (load <= 1/2), at least
// 2^10 slots.  shift = 64 - log2 (the slot of hash h is (h * kPoly) >> shift); hash_mask cuts a
// hash to its low hash_bits bits.
struct TableGeometry {
    int log2;
    size_t slots;
    uint64_t cap_mask;
    int shift;
    uint64_t hash_mask;
};

inline TableGeometry table_geometry(int64_t keys, int hash_bits) {
    TableGeometry g;
    g.log2 = 10;
    while (((int64_t)1 << g.log2) < 2 * keys) ++g.log2;
    g.slots = (size_t)1 << g.log2;
    g.cap_mask = (uint64_t)g.slots - 1;
    g.shift = 64 - g.log2;
    g.hash_mask = hash_bits >= 64 ? ~0ull : (((uint64_t)1 << hash_bits) - 1);
    return g;
}

// The hash width of a stage's CRISPR_*_HASH_BITS switch, clamped to [0, 64]; 64 when unset.
inline int env_hash_bits(const char* name) {
    const char* e = std::getenv(name);
    return e ? std::max(0, std::min(64, std::atoi(e))) : 64;
}

}  // namespace grp
