// host_dev.h -- the host plumbing every stage shares (host-only, header-only): the grow-only
// device array, the per-context error recorder and HIP check, the context base (device, stream,
// events, error text) and the per-call bag of device allocations.  A new stage starts from here
// and, if it groups keys in a hash table, from group_device.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/crispr_nw.h"

namespace hd {

// A grow-only device array of T.  After any successful reserve p is non-null (reserve(0) of a
// fresh buffer allocates one element).  Freed with its owner: a context's buffers go with
// `delete ctx`, on the device the caller has set.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n) {
        if (n <= cap && p) return hipSuccess;
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

// Records the message in c->err (any context with a std::string err; c may be null); returns code.
template <class Ctx>
int fail(Ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

// What a device context starts from: its device, one non-blocking stream, n events, the text of
// its last error.  A stage's context derives from it and holds its buffers as DevBuf members:
// on `delete` those free themselves first, then this base destroys the events and the stream
// (the order of the hand-written destroy functions this replaces).
struct DevContext {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev;
    std::string err;

    DevContext() = default;
    DevContext(const DevContext&) = delete;
    DevContext& operator=(const DevContext&) = delete;
    ~DevContext() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
    bool open(int dev, int n_events) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || dev < 0 || dev >= ndev) return false;
        device = dev;
        bool ok = hipSetDevice(dev) == hipSuccess && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess;
        for (int i = 0; ok && i < n_events; ++i) {
            hipEvent_t e = nullptr;
            ok = hipEventCreate(&e) == hipSuccess;
            if (ok) ev.push_back(e);
        }
        return ok;
    }
};

// *_create: a Ctx (derived from DevContext) open on `device` with n_events events, or NW_E_HIP
// and a null *out.
template <class Ctx>
int create_context(int device, int n_events, Ctx** out) {
    if (!out) return NW_E_INVALID;
    *out = nullptr;
    Ctx* c = new Ctx();
    if (!c->open(device, n_events)) {
        delete c;
        return NW_E_HIP;
    }
    *out = c;
    return NW_OK;
}

// *_destroy: everything the context owns goes with it, on its device.
template <class Ctx>
void destroy_context(Ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

// The device side of one call: its allocations and two events on the null stream, all released
// when it goes out of scope.
struct DevBag {
    std::vector<void*> bufs;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    DevBag() = default;
    DevBag(const DevBag&) = delete;
    DevBag& operator=(const DevBag&) = delete;
    ~DevBag() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        for (void* p : bufs) (void)hipFree(p);
    }
    // at least 16 bytes; null on failure
    void* dev(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr;
        bufs.push_back(p);
        return p;
    }
    // marks the start of a timed stretch (the events are made at the first one)
    bool begin() {
        if (!e0 && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) return false;
        return hipEventRecord(e0, nullptr) == hipSuccess;
    }
    // waits for what ran since begin(); its time in ms to *ms (ms may be null)
    bool elapsed(float* ms) {
        return hipGetLastError() == hipSuccess && hipEventRecord(e1, nullptr) == hipSuccess &&
               hipEventSynchronize(e1) == hipSuccess && (!ms || hipEventElapsedTime(ms, e0, e1) == hipSuccess);
    }
};

}  // namespace hd

// Returns from the enclosing function through hd::fail when a HIP call fails: NW_E_NOMEM for a
// failed allocation, NW_E_HIP for everything else.
#define HIP_TRY(ctx, expr)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return hd::fail((ctx), e_ == hipErrorOutOfMemory ? NW_E_NOMEM : NW_E_HIP, "%s failed: %s", #expr, \
                            hipGetErrorString(e_));                                                          \
    } while (0)
