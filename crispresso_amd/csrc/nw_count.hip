// nw_count.hip -- sgRNA counting on host reads (gfx950): CRISPRessoCount's per-read find, slice
// and tally (CRISPRessoCountCORE.py:320-347), behind the C ABI of include/crispr_count.h.
//
// A call runs its reads in chunks; every kernel is launched on the context's stream:
//   find     one wavefront per run of 64 consecutive reads.  The run's span is swept 64
//            candidate positions at a time, a lane per position: the text dword at an
//            unaligned position comes from two aligned words and a funnel shift, the pattern
//            sits as dwords in LDS, and the sweep of one step ends as soon as no lane still
//            matches.  The ballot of the survivors is then cut by every read (a lane per read)
//            to its own range [off, off + n - m], so a match that straddles two reads is none.
//            The found reads' guides go to a fixed-stride key buffer with length and hash.
//   insert   (no whitelist) one lane per read: the lanes of a wavefront that share a hash elect
//            their lowest lane, which claims the hash's slot of an open-addressing table (64-bit
//            CAS, linear probing bounded by the table size); atomicMin(first) / atomicAdd(count)
//            make the slot's content independent of the order of arrival.
//   publish  the read that is its slot's first writes its key into the slot's key store (the
//            table outlives the chunk, the chunk's keys do not).
//   verify   every other counted read compares its key with the slot's; a read that differs
//            (equal hashes, different guides) goes to the collided list, grouped on the host.
//   lookup   (whitelist) the table is built exactly by the host; the device only probes it and
//            counts on a hit of hash, length and bytes.
//   compact  after the last chunk: the occupied slots, gathered to dense arrays; the host sorts
//            them by first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/crispr_count.h"
#include "../../include/crispr_nw.h"
#include "group_device.h"
#include "host_dev.h"

namespace nwc {

using grp::fmix64;
using grp::kLenMul;
using grp::kPoly;
using grp::wave_elect;

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr int64_t kChunkBytes = (int64_t)64 << 20;     // text per chunk by default
constexpr int64_t kChunkReads = (int64_t)4 << 20;      // and no more reads than this
enum { kFound = 0, kCounted = 1, kError = 2, kCollided = 3, kGroups = 4, kCounters = 8 };

// The hash of a key from the polynomial of its zero-padded dwords (sum of dword k times
// kPoly^(k + 1)): the length mixed in, cut to the low bits of `mask`, never 0 (0 = no key).
__host__ __device__ inline uint64_t finish_hash(uint64_t poly, int32_t len, uint64_t mask) {
    uint64_t h = fmix64(poly ^ ((uint64_t)(uint32_t)len * kLenMul + 1));
    h &= mask;
    return h ? h : 1;
}

struct Args {
    const uint32_t* text;      // the chunk's words; its first byte is byte (first offset & 3) of word 0
    const int64_t* off;        // [cn + 1] the chunk's offsets; byte 0 of word 0 is offset `base`
    int64_t base;
    int64_t r0;                // global index of the chunk's first read
    int32_t cn;                // reads of the chunk
    int32_t m, L, kw;          // pattern bytes, guide length, key dwords ((L + 3) / 4)
    const uint32_t* pat;       // [32] the pattern's dwords, zero-padded
    uint32_t last_mask;        // the bytes of the pattern's last dword
    int32_t* pos;              // [cn]
    int32_t* klen;             // [cn] -1 = not found
    uint64_t* hash;            // [cn] 0 = not found
    uint32_t* keys;            // [cn * kw]
    uint32_t* slot;            // [cn] the read's table slot, kNoSlot = not counted
    unsigned long long* tkey;  // table: [cap] the slot's hash, 0 = empty
    uint32_t* tfirst;
    uint32_t* tcount;
    int32_t* tlen;
    uint32_t* tkeys;           // [cap * kw]
    uint64_t cap_mask;
    int shift;                 // 64 - log2(cap)
    uint64_t hash_mask;
    uint32_t* coll;            // [cn] the chunk's collided reads (chunk index), any order
    uint32_t* counters;
};

__global__ __launch_bounds__(256) void nwc_find_kernel(Args a) {
    __shared__ uint32_t spat[32];
    if (threadIdx.x < 32) spat[threadIdx.x] = a.pat[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t r_lo = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (r_lo >= a.cn) return;
    const int64_t r_hi = r_lo + 64 < a.cn ? r_lo + 64 : a.cn;
    const int64_t r = r_lo + lane;
    const bool have = r < r_hi;
    const int64_t run_start = a.off[r_lo] - a.base, run_end = a.off[r_hi] - a.base;
    const int64_t s0 = have ? a.off[r] - a.base : run_end;
    const int64_t s1 = have ? a.off[r + 1] - a.base : run_end;
    const int m = a.m, nd = (m + 3) >> 2;
    const int64_t last = s1 - s0 >= m ? s1 - m : -1;    // this read's last candidate position
    int64_t hit = -1;
    for (int64_t b = run_start; b + m <= run_end; b += 64) {
        const int64_t p = b + lane;
        bool alive = p + m <= run_end;
        const int64_t q = p >> 2, qe = (p + m - 1) >> 2;
        const unsigned sh = 8u * (unsigned)(p & 3);
        uint32_t lo = alive ? a.text[q] : 0u;
        for (int k = 0; k < nd; ++k) {
            if (!__ballot(alive)) break;
            const uint32_t hi = (alive && q + k + 1 <= qe) ? a.text[q + k + 1] : 0u;
            const uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
            const uint32_t mask = k == nd - 1 ? a.last_mask : 0xFFFFFFFFu;
            alive = alive && ((v ^ spat[k]) & mask) == 0;
            lo = hi;
        }
        const unsigned long long match = __ballot(alive);
        if (hit < 0 && last >= 0) {
            const int64_t from = s0 > b ? s0 : b, to = last < b + 63 ? last : b + 63;
            if (from <= to) {
                unsigned long long mm = match >> (from - b);
                const int width = (int)(to - from + 1);
                if (width < 64) mm &= (1ull << width) - 1ull;
                if (mm) hit = from + (__ffsll((long long)mm) - 1);
            }
        }
    }
    const bool found = have && hit >= 0;
    const unsigned long long fb = __ballot(found);
    if (lane == 0 && fb) atomicAdd(&a.counters[kFound], (uint32_t)__popcll(fb));
    if (!have) return;
    if (!found) {
        a.pos[r] = -1;
        a.klen[r] = -1;
        a.hash[r] = 0;
        return;
    }
    const int64_t idx = hit - s0, n = s1 - s0;
    int64_t st = idx - a.L;
    if (st < 0) st = st + n > 0 ? st + n : 0;
    const int glen = st < idx ? (int)(idx - st) : 0;
    uint64_t poly = 0, pw = kPoly;
    for (int k = 0; k < a.kw; ++k) {
        const uint32_t v = 4 * k < glen ? grp::load_dword((const uint8_t*)a.text + (s0 + st), k, glen) : 0u;
        a.keys[r * a.kw + k] = v;
        poly += (uint64_t)v * pw;
        pw *= kPoly;
    }
    a.pos[r] = (int32_t)idx;
    a.klen[r] = glen;
    a.hash[r] = finish_hash(poly, glen, a.hash_mask);
}

__global__ __launch_bounds__(256) void nwc_insert_kernel(Args a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t h = r < a.cn ? a.hash[r] : 0;
    // the lanes that share a hash elect the lowest of them (the smallest read index)
    int lead;
    const uint32_t cnt = wave_elect(h, h != 0, &lead);
    uint32_t found = kNoSlot;
    if (cnt) {
        found = (uint32_t)grp::claim_slot(a.tkey, a.tfirst, a.tcount, h, (uint32_t)(a.r0 + r), cnt, a.shift, a.cap_mask);
        if (found == kNoSlot) a.counters[kError] = 1;   // a full table: cannot happen at load <= 1/2
    }
    found = (uint32_t)__shfl((int)found, lead, 64);
    if (r < a.cn) a.slot[r] = h ? found : kNoSlot;
}

__global__ __launch_bounds__(256) void nwc_publish_kernel(Args a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.cn) return;
    const uint32_t s = a.slot[r];
    if (s == kNoSlot || a.tfirst[s] != (uint32_t)(a.r0 + r)) return;
    a.tlen[s] = a.klen[r];
    for (int k = 0; k < a.kw; ++k) a.tkeys[(int64_t)s * a.kw + k] = a.keys[r * a.kw + k];
}

__global__ __launch_bounds__(256) void nwc_verify_kernel(Args a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool diff = false;
    if (r < a.cn) {
        const uint32_t s = a.slot[r];
        if (s != kNoSlot) {
            const uint32_t f = a.tfirst[s];
            if (f > (uint32_t)(a.r0 + r)) a.counters[kError] = 1;      // (only after a failed insert)
            if (f < (uint32_t)(a.r0 + r)) {
                diff = a.tlen[s] != a.klen[r];
                for (int k = 0; k < a.kw && !diff; ++k)
                    diff = a.tkeys[(int64_t)s * a.kw + k] != a.keys[r * a.kw + k];
            }
        }
    }
    const uint32_t at = grp::wave_reserve(diff, &a.counters[kCollided]);
    if (diff) a.coll[at] = (uint32_t)r;
}

// Whitelist: tkey / tlen / tkeys hold the host's table; tcount is the count by slot.
__global__ __launch_bounds__(256) void nwc_lookup_kernel(Args a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t h = r < a.cn ? a.hash[r] : 0;
    uint32_t found = kNoSlot;
    if (h) {
        uint64_t s = (h * kPoly) >> a.shift;
        for (uint64_t probe = 0; probe <= a.cap_mask; ++probe) {      // bounded by the table size
            const unsigned long long k = a.tkey[s];
            if (k == 0) break;
            if (k == h && a.tlen[s] == a.klen[r]) {
                bool same = true;
                for (int j = 0; j < a.kw && same; ++j) same = a.tkeys[(int64_t)s * a.kw + j] == a.keys[r * a.kw + j];
                if (same) {
                    found = (uint32_t)s;
                    break;
                }
            }
            s = (s + 1) & a.cap_mask;
        }
    }
    // the lanes that hit one slot add their number once (a library's few most frequent guides
    // take most of the reads: one atomic per read would serialise on those counters)
    int lead;
    const uint32_t cnt = wave_elect(found, found != kNoSlot, &lead);
    if (cnt) atomicAdd(&a.tcount[found], cnt);
    const unsigned long long hb = __ballot(found != kNoSlot);
    if (lane == 0 && hb) atomicAdd(&a.counters[kCounted], (uint32_t)__popcll(hb));
    if (r < a.cn) a.slot[r] = found;
}

__global__ __launch_bounds__(256) void nwc_occupied_kernel(Args a, uint32_t* list) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool used = s <= a.cap_mask && a.tkey[s] != 0;
    const uint32_t at = grp::wave_reserve(used, &a.counters[kGroups]);
    if (used) list[at] = (uint32_t)s;
}

__global__ __launch_bounds__(256) void nwc_gather_kernel(Args a, const uint32_t* list, int64_t ng, uint32_t* gfirst,
                                                         uint32_t* gcount, int32_t* glen, uint32_t* gkeys) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= ng) return;
    const uint32_t s = list[g];
    gfirst[g] = a.tfirst[s];
    gcount[g] = a.tcount[s];
    glen[g] = a.tlen[s];
    for (int k = 0; k < a.kw; ++k) gkeys[g * a.kw + k] = a.tkeys[(int64_t)s * a.kw + k];
}

// The polynomial of a key's zero-padded dwords, as the find kernel computes it.
uint64_t host_hash(const uint8_t* key, int len, int kw, uint64_t mask, uint32_t* dwords) {
    uint64_t poly = 0, pw = kPoly;
    for (int k = 0; k < kw; ++k) {
        uint32_t v = 0;
        if (4 * k < len) std::memcpy(&v, key + 4 * k, (size_t)std::min(4, len - 4 * k));
        dwords[k] = v;
        poly += (uint64_t)v * pw;
        pw *= kPoly;
    }
    return finish_hash(poly, len, mask);
}

}  // namespace nwc

struct nwc_ctx : hd::DevContext {
    int hash_bits = 64;
    int64_t chunk_reads = 0;       // 0: by bytes
    int64_t collided = 0;
    float phase_ms[6] = {0, 0, 0, 0, 0, 0};
    // the last call's groups
    std::vector<int64_t> g_first, g_count, g_koff;
    std::vector<uint8_t> g_kbytes;
    hd::DevBuf<uint32_t> d_text, d_pat, d_keys, d_slot, d_tfirst, d_tcount, d_tkeys, d_coll, d_counters, d_list,
        d_gfirst, d_gcount, d_gkeys;
    hd::DevBuf<int64_t> d_off;
    hd::DevBuf<int32_t> d_pos, d_klen, d_tlen, d_glen;
    hd::DevBuf<uint64_t> d_hash;
    hd::DevBuf<unsigned long long> d_tkey;
};

namespace {

using hd::fail;

struct Collided {
    int64_t read;          // global read index
    uint32_t slot;
    std::string key;
};

// The whitelist's distinct keys in order of first line, and the key of every line.
struct Whitelist {
    std::vector<std::string> keys;
    std::vector<int64_t> slot_key;     // table slot -> key index (-1 = empty)
};

int hand_out(const nwc_ctx* c, int64_t* first, int64_t* count, int64_t* key_offsets, uint8_t* key_bytes, int64_t cap,
             int64_t key_cap) {
    const int64_t ng = (int64_t)c->g_first.size(), nb = (int64_t)c->g_kbytes.size();
    if (ng > cap || nb > key_cap) return NW_E_CAPACITY;
    if (ng > 0 && (!first || !count || !key_offsets)) return NW_E_INVALID;
    if (nb > 0 && !key_bytes) return NW_E_INVALID;
    if (ng > 0) {
        std::memcpy(first, c->g_first.data(), sizeof(int64_t) * (size_t)ng);
        std::memcpy(count, c->g_count.data(), sizeof(int64_t) * (size_t)ng);
    }
    if (key_offsets) std::memcpy(key_offsets, c->g_koff.data(), sizeof(int64_t) * (size_t)(ng + 1));
    if (nb > 0) std::memcpy(key_bytes, c->g_kbytes.data(), (size_t)nb);
    return NW_OK;
}

}  // namespace

extern "C" {

int nwc_create(int device, nwc_ctx** out) {
    const int rc = hd::create_context(device, 5, out);
    if (rc != NW_OK) return rc;
    nwc_ctx* c = *out;
    c->hash_bits = grp::env_hash_bits("CRISPR_NWC_HASH_BITS");
    if (const char* e = std::getenv("CRISPR_NWC_CHUNK"))
        c->chunk_reads = std::max<int64_t>(0, std::min<int64_t>(std::atoll(e), 0x7FFFFFFFll));
    c->g_koff.assign(1, 0);
    return NW_OK;
}

void nwc_destroy(nwc_ctx* c) { hd::destroy_context(c); }

const char* nwc_last_error(const nwc_ctx* c) { return c ? c->err.c_str() : "null context"; }

int64_t nwc_last_collided(const nwc_ctx* c) { return c ? c->collided : -1; }

int nwc_phase_times(const nwc_ctx* c, float* ms) {
    if (!c || !ms) return NW_E_INVALID;
    std::memcpy(ms, c->phase_ms, sizeof c->phase_ms);
    return NW_OK;
}

int nwc_fetch_groups(const nwc_ctx* c, int64_t* first, int64_t* count, int64_t* key_offsets, uint8_t* key_bytes,
                     int64_t cap, int64_t key_cap) {
    if (!c || cap < 0 || key_cap < 0) return NW_E_INVALID;
    return hand_out(c, first, count, key_offsets, key_bytes, cap, key_cap);
}

int nwc_count(nwc_ctx* c, const uint8_t* reads, const int64_t* offsets, int64_t n, const uint8_t* pattern,
              int32_t m, int32_t guide_length, const uint8_t* wl_bytes, const int64_t* wl_offsets, int64_t n_wl,
              int64_t* first, int64_t* count, int64_t* key_offsets, uint8_t* key_bytes, int64_t cap,
              int64_t key_cap, int32_t* pos, int32_t* group_of_read, int64_t* n_groups, int64_t* n_key_bytes,
              int64_t* n_found, int64_t* n_counted, float* kernel_ms) {
    if (!c) return NW_E_INVALID;
    if (n < 0 || n > 0x7FFFFFFFll) return fail(c, NW_E_INVALID, "read count %lld out of range", (long long)n);
    if (!n_groups || !n_key_bytes || !n_found || !n_counted || cap < 0 || key_cap < 0)
        return fail(c, NW_E_INVALID, "null output");
    if (n > 0 && (!reads || !offsets)) return fail(c, NW_E_INVALID, "null input array");
    if (!pattern || m < 1 || m > NWC_MAX_PATTERN)
        return fail(c, NW_E_UNSUPPORTED, "pattern of %d bytes: 1 to %d are supported", (int)m, NWC_MAX_PATTERN);
    if (guide_length < 0 || guide_length > NWC_MAX_GUIDE)
        return fail(c, NW_E_UNSUPPORTED, "guide length %d: 0 to %d are supported", (int)guide_length, NWC_MAX_GUIDE);
    const bool wl = n_wl >= 0;
    if (wl && n_wl > 0 && !wl_offsets) return fail(c, NW_E_INVALID, "null whitelist");
    for (int64_t k = 0; wl && k < n_wl; ++k)
        if (wl_offsets[k + 1] < wl_offsets[k]) return fail(c, NW_E_INVALID, "whitelist offsets do not ascend");
    for (int64_t r = 0; r < n; ++r) {
        const int64_t len = offsets[r + 1] - offsets[r];
        if (len < 0) return fail(c, NW_E_INVALID, "offsets do not ascend at read %lld", (long long)r);
        if (len > 0x7FFFFFFFll) return fail(c, NW_E_UNSUPPORTED, "read %lld is longer than 2^31 - 1 bytes", (long long)r);
    }
    c->collided = 0;
    std::fill(c->phase_ms, c->phase_ms + 6, 0.0f);
    c->g_first.clear();
    c->g_count.clear();
    c->g_kbytes.clear();
    c->g_koff.assign(1, 0);
    if (kernel_ms) *kernel_ms = 0.0f;
    *n_groups = *n_key_bytes = *n_found = *n_counted = 0;

    const int L = guide_length, kw = (L + 3) / 4;

    // the whitelist: distinct keys in order of first line; the table of those that can be a guide
    Whitelist W;
    std::vector<unsigned long long> h_tkey;
    std::vector<int32_t> h_tlen;
    std::vector<uint32_t> h_tkeys;
    if (wl) {
        std::unordered_map<std::string, int64_t> seen;
        for (int64_t k = 0; k < n_wl; ++k) {
            std::string key((const char*)wl_bytes + wl_offsets[k], (size_t)(wl_offsets[k + 1] - wl_offsets[k]));
            if (seen.emplace(key, (int64_t)W.keys.size()).second) W.keys.push_back(std::move(key));
        }
    }
    // (free mode: 2^31 slots at most: a slot index is 32 bits with one value reserved; above 2^30 reads
    //  the load passes 1/2 but stays under 1, and the probe bound still holds)
    const grp::TableGeometry tg =
        grp::table_geometry(wl ? (int64_t)W.keys.size() : std::min<int64_t>(n, (int64_t)1 << 30), c->hash_bits);
    const size_t slots = tg.slots;
    if (wl) {
        h_tkey.assign(slots, 0);
        h_tlen.assign(slots, 0);
        h_tkeys.assign(slots * (size_t)std::max(kw, 1), 0);
        W.slot_key.assign(slots, -1);
        uint32_t dw[NWC_MAX_GUIDE / 4];
        for (size_t k = 0; k < W.keys.size(); ++k) {
            const std::string& key = W.keys[k];
            if ((int64_t)key.size() > L) continue;            // no guide is longer than L
            const uint64_t h = nwc::host_hash((const uint8_t*)key.data(), (int)key.size(), kw, tg.hash_mask, dw);
            size_t s = (size_t)((h * nwc::kPoly) >> tg.shift);
            while (h_tkey[s] != 0) s = (s + 1) & (slots - 1);   // distinct keys at load <= 1/2: ends
            h_tkey[s] = h;
            h_tlen[s] = (int32_t)key.size();
            for (int j = 0; j < kw; ++j) h_tkeys[s * (size_t)kw + (size_t)j] = dw[j];
            W.slot_key[s] = (int64_t)k;
        }
    }

    std::vector<Collided> collided;
    std::vector<uint32_t> slot_of_read;      // free mode: each counted read's slot until the groups are known
    const bool want_gor = group_of_read != nullptr;
    uint32_t ctr[nwc::kCounters] = {};
    float kms = 0.0f;
    nwc::Args a{};

    if (n > 0) {
        HIP_TRY(c, hipSetDevice(c->device));
        hipStream_t st = c->stream;
        HIP_TRY(c, c->d_pat.reserve(32));
        HIP_TRY(c, c->d_counters.reserve(nwc::kCounters));
        HIP_TRY(c, c->d_tkey.reserve(slots));
        HIP_TRY(c, c->d_tfirst.reserve(slots));
        HIP_TRY(c, c->d_tcount.reserve(slots));
        HIP_TRY(c, c->d_tlen.reserve(slots));
        HIP_TRY(c, c->d_tkeys.reserve(slots * (size_t)std::max(kw, 1)));
        uint32_t pat[32] = {};
        std::memcpy(pat, pattern, (size_t)m);
        HIP_TRY(c, hipMemcpyAsync(c->d_pat.p, pat, sizeof pat, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemsetAsync(c->d_counters.p, 0, sizeof(uint32_t) * nwc::kCounters, st));
        HIP_TRY(c, hipMemsetAsync(c->d_tcount.p, 0, sizeof(uint32_t) * slots, st));
        if (wl) {
            HIP_TRY(c, hipMemcpyAsync(c->d_tkey.p, h_tkey.data(), sizeof(unsigned long long) * slots, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(c->d_tlen.p, h_tlen.data(), sizeof(int32_t) * slots, hipMemcpyHostToDevice, st));
            if (kw > 0)
                HIP_TRY(c, hipMemcpyAsync(c->d_tkeys.p, h_tkeys.data(), sizeof(uint32_t) * slots * (size_t)kw,
                                          hipMemcpyHostToDevice, st));
        } else {
            HIP_TRY(c, hipMemsetAsync(c->d_tkey.p, 0, sizeof(unsigned long long) * slots, st));
            HIP_TRY(c, hipMemsetAsync(c->d_tfirst.p, 0xFF, sizeof(uint32_t) * slots, st));
            HIP_TRY(c, hipMemsetAsync(c->d_tlen.p, 0, sizeof(int32_t) * slots, st));
        }
        HIP_TRY(c, hipStreamSynchronize(st));       // (the host tables above are read by the copies)
        a.m = m;
        a.L = L;
        a.kw = kw;
        a.pat = c->d_pat.p;
        a.last_mask = (m & 3) ? (1u << (8 * (m & 3))) - 1u : 0xFFFFFFFFu;
        a.tkey = c->d_tkey.p;
        a.tfirst = c->d_tfirst.p;
        a.tcount = c->d_tcount.p;
        a.tlen = c->d_tlen.p;
        a.tkeys = c->d_tkeys.p;
        a.cap_mask = tg.cap_mask;
        a.shift = tg.shift;
        a.hash_mask = tg.hash_mask;
        a.counters = c->d_counters.p;
        if (!wl && want_gor) slot_of_read.assign((size_t)n, nwc::kNoSlot);

        std::vector<uint32_t> h_slot, h_coll, h_keys;
        std::vector<int32_t> h_klen;
        for (int64_t r0 = 0; r0 < n;) {
            int64_t r1;
            if (c->chunk_reads > 0) {
                r1 = std::min(n, r0 + c->chunk_reads);
            } else {
                r1 = std::min(n, r0 + nwc::kChunkReads);
                const int64_t* e = std::upper_bound(offsets + r0 + 1, offsets + r1 + 1, offsets[r0] + nwc::kChunkBytes);
                r1 = std::max<int64_t>(r0 + 1, (e - offsets) - 1);      // (one read at least, whatever its size)
            }
            // the chunk keeps the phase of its first byte within a word (lead), as a resident batch would
            const int64_t cn = r1 - r0, lead = offsets[r0] & 3, base = offsets[r0] - lead, nbytes = offsets[r1] - offsets[r0];
            const size_t words = (size_t)((lead + nbytes + 3) / 4);
            HIP_TRY(c, c->d_text.reserve(words));
            HIP_TRY(c, c->d_off.reserve((size_t)cn + 1));
            HIP_TRY(c, c->d_pos.reserve((size_t)cn));
            HIP_TRY(c, c->d_klen.reserve((size_t)cn));
            HIP_TRY(c, c->d_hash.reserve((size_t)cn));
            HIP_TRY(c, c->d_keys.reserve((size_t)cn * (size_t)std::max(kw, 1)));
            HIP_TRY(c, c->d_slot.reserve((size_t)cn));
            HIP_TRY(c, c->d_coll.reserve((size_t)cn));
            const auto t0 = std::chrono::steady_clock::now();
            if (nbytes > 0) {
                HIP_TRY(c, hipMemsetAsync(c->d_text.p, 0, 4, st));                   // (the bytes beside the batch
                HIP_TRY(c, hipMemsetAsync(c->d_text.p + (words - 1), 0, 4, st));     //  in its first and last word)
                HIP_TRY(c, hipMemcpyAsync((uint8_t*)c->d_text.p + lead, reads + offsets[r0], (size_t)nbytes,
                                          hipMemcpyHostToDevice, st));
            }
            HIP_TRY(c, hipMemcpyAsync(c->d_off.p, offsets + r0, sizeof(int64_t) * (size_t)(cn + 1), hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipStreamSynchronize(st));
            c->phase_ms[5] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            a.text = c->d_text.p;
            a.off = c->d_off.p;
            a.base = base;
            a.r0 = r0;
            a.cn = (int32_t)cn;
            a.pos = c->d_pos.p;
            a.klen = c->d_klen.p;
            a.hash = c->d_hash.p;
            a.keys = c->d_keys.p;
            a.slot = c->d_slot.p;
            a.coll = c->d_coll.p;
            HIP_TRY(c, hipMemsetAsync(&a.counters[nwc::kCollided], 0, sizeof(uint32_t), st));
            const unsigned find_grid = (unsigned)((cn + 255) / 256), lane_grid = find_grid;
            HIP_TRY(c, hipEventRecord(c->ev[0], st));
            hipLaunchKernelGGL(nwc::nwc_find_kernel, dim3(find_grid), dim3(256), 0, st, a);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(c->ev[1], st));
            if (wl) {
                HIP_TRY(c, hipEventRecord(c->ev[2], st));
                HIP_TRY(c, hipEventRecord(c->ev[3], st));
                hipLaunchKernelGGL(nwc::nwc_lookup_kernel, dim3(lane_grid), dim3(256), 0, st, a);
                HIP_TRY(c, hipGetLastError());
            } else {
                hipLaunchKernelGGL(nwc::nwc_insert_kernel, dim3(lane_grid), dim3(256), 0, st, a);
                HIP_TRY(c, hipGetLastError());
                HIP_TRY(c, hipEventRecord(c->ev[2], st));
                hipLaunchKernelGGL(nwc::nwc_publish_kernel, dim3(lane_grid), dim3(256), 0, st, a);
                HIP_TRY(c, hipGetLastError());
                HIP_TRY(c, hipEventRecord(c->ev[3], st));
                hipLaunchKernelGGL(nwc::nwc_verify_kernel, dim3(lane_grid), dim3(256), 0, st, a);
                HIP_TRY(c, hipGetLastError());
            }
            HIP_TRY(c, hipEventRecord(c->ev[4], st));
            HIP_TRY(c, hipMemcpyAsync(ctr, a.counters, sizeof ctr, hipMemcpyDeviceToHost, st));
            if (pos) HIP_TRY(c, hipMemcpyAsync(pos + r0, a.pos, sizeof(int32_t) * (size_t)cn, hipMemcpyDeviceToHost, st));
            if (want_gor) {
                h_slot.resize((size_t)cn);
                HIP_TRY(c, hipMemcpyAsync(h_slot.data(), a.slot, sizeof(uint32_t) * (size_t)cn, hipMemcpyDeviceToHost, st));
            }
            HIP_TRY(c, hipStreamSynchronize(st));
            for (int i = 0; i < 4; ++i) {
                float ms = 0.0f;
                HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
                c->phase_ms[i] += ms;
                kms += ms;
            }
            if (ctr[nwc::kError])
                return fail(c, NW_E_STATE, "the hash table's probe bound was reached (%zu slots, %lld reads)", slots,
                            (long long)n);
            if (want_gor) {
                if (wl)
                    for (int64_t i = 0; i < cn; ++i)
                        group_of_read[r0 + i] = h_slot[(size_t)i] == nwc::kNoSlot ? -1 : (int32_t)W.slot_key[h_slot[(size_t)i]];
                else
                    std::copy(h_slot.begin(), h_slot.end(), slot_of_read.begin() + r0);
            }
            const int64_t nc = ctr[nwc::kCollided];
            if (nc > cn) return fail(c, NW_E_STATE, "inconsistent collided count");
            if (nc > 0) {      // equal hashes, different guides: their keys come back, the host groups them
                h_coll.resize((size_t)nc);
                h_klen.resize((size_t)cn);
                h_keys.resize((size_t)cn * (size_t)std::max(kw, 1));
                h_slot.resize((size_t)cn);
                HIP_TRY(c, hipMemcpy(h_coll.data(), a.coll, sizeof(uint32_t) * (size_t)nc, hipMemcpyDeviceToHost));
                HIP_TRY(c, hipMemcpy(h_klen.data(), a.klen, sizeof(int32_t) * (size_t)cn, hipMemcpyDeviceToHost));
                HIP_TRY(c, hipMemcpy(h_slot.data(), a.slot, sizeof(uint32_t) * (size_t)cn, hipMemcpyDeviceToHost));
                if (kw > 0)
                    HIP_TRY(c, hipMemcpy(h_keys.data(), a.keys, sizeof(uint32_t) * (size_t)cn * (size_t)kw, hipMemcpyDeviceToHost));
                std::sort(h_coll.begin(), h_coll.end());
                for (uint32_t i : h_coll) {
                    if (i >= (uint32_t)cn || h_klen[i] < 0 || h_klen[i] > L || h_slot[i] == nwc::kNoSlot)
                        return fail(c, NW_E_STATE, "inconsistent collided read");
                    collided.push_back({r0 + (int64_t)i, h_slot[i],
                                        std::string((const char*)(h_keys.data() + (size_t)i * (size_t)kw), (size_t)h_klen[i])});
                }
            }
            r0 = r1;
        }
    }
    *n_found = ctr[nwc::kFound];
    c->collided = (int64_t)collided.size();

    if (wl) {
        std::vector<uint32_t> tcount;
        if (n > 0) {
            tcount.resize(slots);
            HIP_TRY(c, hipMemcpy(tcount.data(), a.tcount, sizeof(uint32_t) * slots, hipMemcpyDeviceToHost));
        }
        const size_t ng = W.keys.size();
        c->g_first.assign(ng, -1);
        c->g_count.assign(ng, 0);
        for (size_t s = 0; s < tcount.size(); ++s)
            if (W.slot_key[s] >= 0) c->g_count[(size_t)W.slot_key[s]] = tcount[s];
        for (size_t k = 0; k < ng; ++k) {
            c->g_kbytes.insert(c->g_kbytes.end(), W.keys[k].begin(), W.keys[k].end());
            c->g_koff.push_back((int64_t)c->g_kbytes.size());
        }
        *n_counted = ctr[nwc::kCounted];
    } else if (n > 0) {
        hipStream_t st = c->stream;
        HIP_TRY(c, c->d_list.reserve((size_t)std::min<int64_t>((int64_t)slots, n)));
        HIP_TRY(c, hipEventRecord(c->ev[0], st));
        hipLaunchKernelGGL(nwc::nwc_occupied_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, a, c->d_list.p);
        HIP_TRY(c, hipGetLastError());
        uint32_t ngd = 0;
        HIP_TRY(c, hipMemcpyAsync(&ngd, &a.counters[nwc::kGroups], sizeof ngd, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        const int64_t ng_dev = ngd;
        if (ng_dev > n) return fail(c, NW_E_STATE, "inconsistent group count");
        std::vector<uint32_t> gslot((size_t)ng_dev), gfirst((size_t)ng_dev), gcount((size_t)ng_dev), gkeys;
        std::vector<int32_t> glen((size_t)ng_dev);
        if (ng_dev > 0) {
            HIP_TRY(c, c->d_gfirst.reserve((size_t)ng_dev));
            HIP_TRY(c, c->d_gcount.reserve((size_t)ng_dev));
            HIP_TRY(c, c->d_glen.reserve((size_t)ng_dev));
            HIP_TRY(c, c->d_gkeys.reserve((size_t)ng_dev * (size_t)std::max(kw, 1)));
            hipLaunchKernelGGL(nwc::nwc_gather_kernel, dim3((unsigned)((ng_dev + 255) / 256)), dim3(256), 0, st, a,
                               c->d_list.p, ng_dev, c->d_gfirst.p, c->d_gcount.p, c->d_glen.p, c->d_gkeys.p);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(c->ev[1], st));
            gkeys.resize((size_t)ng_dev * (size_t)std::max(kw, 1));
            HIP_TRY(c, hipMemcpyAsync(gslot.data(), c->d_list.p, sizeof(uint32_t) * (size_t)ng_dev, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipMemcpyAsync(gfirst.data(), c->d_gfirst.p, sizeof(uint32_t) * (size_t)ng_dev, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipMemcpyAsync(gcount.data(), c->d_gcount.p, sizeof(uint32_t) * (size_t)ng_dev, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipMemcpyAsync(glen.data(), c->d_glen.p, sizeof(int32_t) * (size_t)ng_dev, hipMemcpyDeviceToHost, st));
            if (kw > 0)
                HIP_TRY(c, hipMemcpyAsync(gkeys.data(), c->d_gkeys.p, sizeof(uint32_t) * (size_t)ng_dev * (size_t)kw,
                                          hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipStreamSynchronize(st));
            HIP_TRY(c, hipEventElapsedTime(&c->phase_ms[4], c->ev[0], c->ev[1]));
            kms += c->phase_ms[4];
        }
        // the slots in order of first appearance (the firsts are distinct read indices)
        std::vector<int64_t> order((size_t)ng_dev);
        for (int64_t i = 0; i < ng_dev; ++i) order[(size_t)i] = i;
        std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return gfirst[(size_t)x] < gfirst[(size_t)y]; });
        std::vector<int32_t> rank_of_slot(slots, -1);            // slot -> rank among the device groups
        for (int64_t i = 0; i < ng_dev; ++i) {
            const size_t g = (size_t)order[(size_t)i];
            if (glen[g] < 0 || glen[g] > L || (int64_t)gfirst[g] >= n) return fail(c, NW_E_STATE, "inconsistent group");
            if (gslot[g] >= slots) return fail(c, NW_E_STATE, "inconsistent group");
            rank_of_slot[gslot[g]] = (int32_t)i;
        }
        // the collided reads leave their slot's count and form groups of their own
        std::map<std::string, int64_t> cseen;
        std::vector<int64_t> cg_first, cg_count, cgrp(collided.size());
        std::vector<const std::string*> cg_key;
        for (size_t i = 0; i < collided.size(); ++i) {
            const int32_t rk = collided[i].slot < slots ? rank_of_slot[collided[i].slot] : -1;
            if (rk < 0) return fail(c, NW_E_STATE, "collided read of an empty slot");
            --gcount[(size_t)order[(size_t)rk]];
            auto ins = cseen.emplace(collided[i].key, (int64_t)cg_first.size());
            if (ins.second) {
                cg_first.push_back(collided[i].read);
                cg_count.push_back(0);
                cg_key.push_back(&ins.first->first);
            }
            cgrp[i] = ins.first->second;
            ++cg_count[(size_t)ins.first->second];
        }
        // merge the two lists (both ascending in first)
        const int64_t ng_new = (int64_t)cg_first.size();
        std::vector<int64_t> dev_id((size_t)ng_dev), new_id((size_t)ng_new);
        int64_t i = 0, j = 0, counted = 0;
        while (i < ng_dev || j < ng_new) {
            const int64_t g = (int64_t)c->g_first.size();
            if (j >= ng_new || (i < ng_dev && (int64_t)gfirst[(size_t)order[(size_t)i]] < cg_first[(size_t)j])) {
                const size_t d = (size_t)order[(size_t)i];
                c->g_first.push_back(gfirst[d]);
                c->g_count.push_back(gcount[d]);
                const uint8_t* kb = (const uint8_t*)(gkeys.data() + d * (size_t)kw);
                c->g_kbytes.insert(c->g_kbytes.end(), kb, kb + glen[d]);
                dev_id[(size_t)i++] = g;
            } else {
                c->g_first.push_back(cg_first[(size_t)j]);
                c->g_count.push_back(cg_count[(size_t)j]);
                c->g_kbytes.insert(c->g_kbytes.end(), cg_key[(size_t)j]->begin(), cg_key[(size_t)j]->end());
                new_id[(size_t)j++] = g;
            }
            counted += c->g_count.back();
            c->g_koff.push_back((int64_t)c->g_kbytes.size());
        }
        *n_counted = counted;
        if (counted != (int64_t)ctr[nwc::kFound]) return fail(c, NW_E_STATE, "the counts do not add up to the found reads");
        if (want_gor) {
            for (int64_t r = 0; r < n; ++r) {
                const uint32_t s = slot_of_read[(size_t)r];
                if (s == nwc::kNoSlot) {
                    group_of_read[r] = -1;
                    continue;
                }
                const int32_t rk = s < slots ? rank_of_slot[s] : -1;
                if (rk < 0) return fail(c, NW_E_STATE, "read %lld in an empty slot", (long long)r);
                group_of_read[r] = (int32_t)dev_id[(size_t)rk];
            }
            for (size_t k = 0; k < collided.size(); ++k)
                group_of_read[collided[k].read] = (int32_t)new_id[(size_t)cgrp[k]];
        }
    }
    if (kernel_ms) *kernel_ms = kms;
    *n_groups = (int64_t)c->g_first.size();
    *n_key_bytes = (int64_t)c->g_kbytes.size();
    const int rc = hand_out(c, first, count, key_offsets, key_bytes, cap, key_cap);
    if (rc == NW_E_CAPACITY)
        return fail(c, rc, "%lld groups with %lld key bytes, capacity %lld and %lld", (long long)*n_groups,
                    (long long)*n_key_bytes, (long long)cap, (long long)key_cap);
    if (rc != NW_OK) return fail(c, rc, "null group array");
    return NW_OK;
}

}  // extern "C"
