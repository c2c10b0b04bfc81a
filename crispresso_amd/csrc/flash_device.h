// What flash_merge.hip (nwf_merge_batch, the merge kernel) shares with the front end
// (front_pack.hip): the kernel's arguments and its launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crispr_flash.h"

namespace nwf {

constexpr int kWpb = 4;

struct Args {
    const uint8_t* seq1;
    const uint8_t* qual1;
    const int64_t* off1;
    const uint8_t* seq2;
    const uint8_t* qual2;
    const int64_t* off2;
    int64_t n;
    uint8_t* out_seq;
    uint8_t* out_qual;
    int32_t* out_len;
    int32_t* out_flags;
    int32_t min_ov, max_ov, allow_outies, phred, cap;
    float max_density;
    int32_t lbuf;   // LDS bytes per staged read (>= longest read, 16-B multiple)
    // the windowed launch only (launch_merge(..., true)): per-read windows as nwt_trim_program
    // writes them (all four or none) and a per-pair live byte (or null)
    const int32_t* start1;
    const int32_t* keep1;
    const int32_t* start2;
    const int32_t* keep2;
    const uint8_t* live;
};

// the FLASH parameters and the LDS row for reads up to lmax bases
void set_params(Args& a, const nwf_params* params, int lmax);
inline size_t merge_lds(const Args& a) { return (size_t)4 * a.lbuf * kWpb; }
// nwf_merge_kernel on the null stream; windows: the instantiation that reads start / keep / live
void launch_merge(const Args& a, unsigned grid, size_t lds, bool windows);

}  // namespace nwf
