// What trim_clip.hip (the C ABI, the clip kernel) and trim_steps.hip (the steps kernel) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crispr_trim.h"

namespace nwt {

constexpr int kWpb = 4;   // waves per block of both kernels when the reads are short

// The steps kernel's arguments: the reads as the clip path uploaded them, mate 1 then mate 2
// (reads n .. 2n - 1 when paired), and the program by value.
struct StepsArgs {
    const uint8_t* seq[2];
    const uint8_t* qual[2];
    const int64_t* off[2];
    const int32_t* keep_in[2];   // the clip kernel's output, or null: the record enters whole
    int32_t* start[2];
    int32_t* keep[2];
    int64_t n;                   // reads per mate
    int32_t paired;
    int32_t n_steps;
    int32_t lb;                  // LDS bytes of a wave's staged qualities (16-B multiple, >= longest read + 4)
    int32_t wpb;
    nwt_step steps[NWT_MAX_STEPS];
};

// LDS bytes of one wave of the steps kernel for reads up to lmax bases; fills lb.
size_t steps_lds_per_wave(int lmax, int32_t* lb);
// Launches nwt_steps_kernel on the null stream (a.wpb waves per block, `grid` blocks).
void launch_steps(const StepsArgs& a, unsigned grid, size_t lds);

}  // namespace nwt
