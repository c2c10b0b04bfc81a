// What the front end (front_pack.hip: nwp_prepare) needs of the aligner context (nw_host.cpp),
// which alone knows nw_ctx: the batch state nw_batch_upload_packed leaves, set from device arrays.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crispr_nw.h"

struct nwp_result;

namespace nw_front {

// A packed batch as nw_batch_upload_packed takes it; on_device: every pointer is a device
// pointer, gbase holds every nw::kLenGroup-th offset (n / kLenGroup + 1 of them), and the
// context's stream waits for `ready` (may be null) before it copies.
struct PackedSrc {
    const uint8_t* packed;
    const uint16_t* lens;
    const int64_t* gbase;      // device source only (the host source's come from the offsets)
    const int64_t* exc_pos;
    const uint8_t* exc_byte;
    bool on_device;
    hipEvent_t ready;
};

// nw_batch_upload_packed's body: offsets and lens are host arrays (n + 1 and n) either way.
int set_packed_batch(nw_ctx* c, const PackedSrc& src, const int64_t* offsets, const uint16_t* lens, int64_t n,
                     int64_t n_exc);
// NW_OK when nw_batch_upload_packed's preconditions hold (a reference, NW_OUT_OPS), else NW_E_STATE
int check_state(nw_ctx* c);
int device_of(const nw_ctx* c);

// A live nwp_result (include/crispr_front.h) as another stage reads it where it lies: the dense
// text and qualities in HBM (quals null unless want_quals; both null when m == 0), the host
// offsets [m + 1] from 0, and the event recorded behind the packer (null when m == 0).  Nothing
// is copied or owned: the view holds until nwp_release.
struct PreparedView {
    const uint8_t* text;       // device, total bytes (+ padding)
    const uint8_t* quals;      // device, or null
    const int64_t* offsets;    // host
    int64_t m, total;
    int device;
    hipEvent_t ready;
};

// NW_OK, or NW_E_INVALID for a null or released result (front_pack.hip)
int view_prepared(const struct ::nwp_result* res, PreparedView* out);

}  // namespace nw_front
