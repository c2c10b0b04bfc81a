// nwa_device.h -- the context of include/crispr_alleles.h, shared by its three translation units:
// nw_alleles.hip (groups of byte-identical reads), nw_windows.hip (the around-cut windows, which
// feed their records to the grouping on the same context) and nw_allele_rows.hip (the allele
// table's representative rows, built after the same grouping).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/crispr_alleles.h"
#include "../../include/crispr_nw.h"
#include "host_dev.h"

namespace nwa {

constexpr int kEvents = 7;     // ev[0..4] the phases of the grouping, ev[5..6] nw_windows.hip and nw_allele_rows.hip

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

struct nwa_ctx;

namespace nwa {

// The number of non-zero bytes of the DEVICE array d_keep[n] (a device reduction; n when d_keep
// is null).
int count_kept(nwa_ctx* c, const uint8_t* d_keep, int64_t n, int64_t* kept);

// The body of nwa_group_device (nw_alleles.hip) with the keep flags already on the device:
// d_keep is a DEVICE array or null, `kept` its non-zero count (count_kept; n without d_keep).
// tag, first, count, group_of_read are HOST arrays as nwa_group_device takes them.  After a
// return of NW_OK without collided reads (c->collided == 0) c->d_gfirst / c->d_gcount hold the
// groups' first reads and sizes on the device as well.
int group_resident(nwa_ctx* c, const uint8_t* d_reads, const int64_t* d_offsets, int64_t reads_bias, int64_t n,
                   const uint8_t* d_keep, int64_t kept, const int32_t* tag, int64_t* first, int64_t* count,
                   int64_t cap, int32_t* group_of_read, int64_t* n_groups, float* kernel_ms);

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
    // nw_allele_rows.hip
    hd::DevBuf<uint8_t> t_amp, t_rows;       // rows: [groups][2][t_stride]
    hd::DevBuf<int32_t> t_cols, t_res;       // res: [groups][4], the representative's nwq_read
    hd::DevBuf<int64_t> t_first, t_count;
    hd::DevBuf<uint32_t> t_err;              // [0] error word, [1] the largest column count
    int64_t t_groups = 0, t_collided = 0;
    int32_t t_stride = 0;
    float t_ms[2] = {0, 0};                  // grouping, columns + rows
};
