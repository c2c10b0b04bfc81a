// nwa_device.h -- the context of include/crispr_alleles.h, shared by its two translation units:
// nw_alleles.hip (groups of byte-identical reads) and nw_windows.hip (the around-cut windows,
// which feed their records to nwa_group_device on the same context).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/crispr_alleles.h"
#include "../../include/crispr_nw.h"

namespace nwa {

template <class T>
struct Buf {
    T* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        release();
        hipError_t e = hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct CollInfo {
    int64_t start, len;        // the read's bytes at reads + start
    int32_t tag, group;        // its slot's group
};

// The around-cut windows of one cut point (nwa_windows_device keeps them for nwa_windows_fetch).
struct WinTable {
    std::vector<int64_t> first, count;
    std::vector<uint8_t> unedited;
    std::vector<int32_t> win_len, gor;
    std::vector<uint8_t> win;          // [groups][2][W]
};

}  // namespace nwa

struct nwa_ctx {
    int device = 0;
    int num_cus = 256;
    int hash_bits = 64;
    hipStream_t stream = nullptr;
    hipEvent_t ev[5] = {};
    std::string err;
    int64_t collided = 0;
    float phase_ms[4] = {0, 0, 0, 0};
    nwa::Buf<uint8_t> d_keep, d_is_first;
    nwa::Buf<int32_t> d_tag, d_gor;
    nwa::Buf<uint64_t> d_hash;
    nwa::Buf<unsigned long long> d_key;
    nwa::Buf<uint32_t> d_slot, d_first, d_count, d_gid, d_coll, d_counters, d_tile_sum, d_tile_off, d_gfirst, d_gcount;
    nwa::Buf<nwa::CollInfo> d_info;
    // nw_windows.hip
    hipEvent_t wev[2] = {};
    nwa::Buf<uint8_t> w_rec, w_amp, w_unmod, w_gwin, w_gun;
    nwa::Buf<int64_t> w_off;
    nwa::Buf<uint32_t> w_err, w_gfirst;
    int w_cuts = 0, w_width = 0;
    int64_t w_collided = 0;
    float w_ms[3] = {0, 0, 0};         // extract, grouping, gather + unedited
    std::vector<nwa::WinTable> w_tab;
};

namespace nwa {

inline int afail(nwa_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

// Frees what nw_windows.hip keeps on the context (nwa_destroy).
void windows_release(nwa_ctx* c);

}  // namespace nwa

#define AHIP(c, expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return nwa::afail((c), e_ == hipErrorOutOfMemory ? NW_E_NOMEM : NW_E_HIP, "%s: %s", #expr, \
                              hipGetErrorString(e_));                                                  \
    } while (0)
