// nwa_device.h -- the context of include/crispr_alleles.h, shared by its two translation units:
// nw_alleles.hip (groups of byte-identical reads) and nw_windows.hip (the around-cut windows,
// which feed their records to nwa_group_device on the same context).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/crispr_alleles.h"
#include "../../include/crispr_nw.h"
#include "host_dev.h"

namespace nwa {

constexpr int kEvents = 7;     // ev[0..4] the phases of nwa_group_device, ev[5..6] nw_windows.hip

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

struct nwa_ctx : hd::DevContext {
    int num_cus = 256;
    int hash_bits = 64;
    int64_t collided = 0;
    float phase_ms[4] = {0, 0, 0, 0};
    hd::DevBuf<uint8_t> d_keep, d_is_first;
    hd::DevBuf<int32_t> d_tag, d_gor;
    hd::DevBuf<uint64_t> d_hash;
    hd::DevBuf<unsigned long long> d_key;
    hd::DevBuf<uint32_t> d_slot, d_first, d_count, d_gid, d_coll, d_counters, d_tile_sum, d_tile_off, d_gfirst, d_gcount;
    hd::DevBuf<nwa::CollInfo> d_info;
    // nw_windows.hip
    hd::DevBuf<uint8_t> w_rec, w_amp, w_unmod, w_gwin, w_gun;
    hd::DevBuf<int64_t> w_off;
    hd::DevBuf<uint32_t> w_err, w_gfirst;
    int w_cuts = 0, w_width = 0;
    int64_t w_collided = 0;
    float w_ms[3] = {0, 0, 0};         // extract, grouping, gather + unedited
    std::vector<nwa::WinTable> w_tab;
};
