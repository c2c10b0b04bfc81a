// What trim_clip.hip (the C ABI, the clip kernel), trim_steps.hip (the steps kernel) and
// front_pack.hip (the front end, which runs both on its own upload) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/crispr_trim.h"
#include "host_dev.h"

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

// The device side of one call: the bag of its allocations and events, the uploaded reads and
// the launch cap.
struct Batch : hd::DevBag {
    uint8_t *s1 = nullptr, *q1 = nullptr, *s2 = nullptr, *q2 = nullptr;
    int64_t *o1 = nullptr, *o2 = nullptr;
    int cus = 256;

    // allocates the read buffers (the caller allocates its own before upload() and checks them all there)
    bool alloc_reads(int64_t t1, int64_t t2, int64_t n) {
        s1 = (uint8_t*)dev(t1 + 8);
        q1 = (uint8_t*)dev(t1 + 8);
        s2 = (uint8_t*)dev(t2 + 8);
        q2 = (uint8_t*)dev(t2 + 8);
        o1 = (int64_t*)dev(sizeof(int64_t) * (n + 1));
        o2 = (int64_t*)dev(sizeof(int64_t) * (n + 1));
        return s1 && q1 && s2 && q2 && o1 && o2;
    }
    bool upload(int device, const uint8_t* seq1, const uint8_t* qual1, const int64_t* off1, const uint8_t* seq2,
                const uint8_t* qual2, const int64_t* off2, int64_t n, bool paired) {
        const int64_t t1 = off1[n], t2 = paired ? off2[n] : 0;
        bool ok = hipMemcpy(s1, seq1, t1, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(q1, qual1, t1, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(o1, off1, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice) == hipSuccess;
        if (ok && paired)
            ok = hipMemcpy(s2, seq2, t2, hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(q2, qual2, t2, hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(o2, off2, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice) == hipSuccess;
        set_launch_cap(device);
        return ok;
    }
    // the launch cap: what a call needs once its reads are on the device
    void set_launch_cap(int device) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            cus = prop.multiProcessorCount;
    }
    // blocks for `items` wavefront jobs at wpb a block: the launch cap both kernels share
    unsigned grid(int64_t items, int wpb) const {
        return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + wpb - 1) / wpb, (int64_t)cus * 16));
    }
};

// A validated nwt_trim_program program: the steps (in sa), ILLUMINACLIP's parameters and tables,
// and the device arrays program_alloc adds to a Batch.
struct Program {
    bool clip = false;
    nwt_params params{};
    StepsArgs sa{};
    int plmax = 0;                       // the longest palindrome prefix
    std::vector<unsigned char> tables;   // the clip kernel's tables (host image)
    int32_t *d_c1 = nullptr, *d_c2 = nullptr;
    void* d_t = nullptr;
};

// What nwt_trim_program and the front end (front_pack.hip) share; `who` starts the message of a
// refusal, which nwt_last_error() returns.
int check_counts(const char* who, const uint8_t* adapters, const int32_t* adapter_off, const int32_t* adapter_role,
                 int32_t n_adapters, const uint8_t* prefixes, const int32_t* prefix_off, int32_t n_prefix_pairs);
int check_reads(const char* who, const uint8_t* qual1, const int64_t* off1, const uint8_t* qual2, const int64_t* off2,
                int64_t n, bool paired, int* lmax);
int program_check(const char* who, const nwt_params* clip, const uint8_t* adapters, const int32_t* adapter_off,
                  const int32_t* adapter_role, int32_t n_adapters, const uint8_t* prefixes, const int32_t* prefix_off,
                  int32_t n_prefix_pairs, const nwt_step* steps, int32_t n_steps, Program& P);
bool program_alloc(Batch& b, Program& P, int64_t n, int32_t* d_out[4]);
bool program_run(Batch& b, Program& P, int lmax, int64_t n, bool paired, int32_t* const d_out[4], float* kernel_ms);

}  // namespace nwt
