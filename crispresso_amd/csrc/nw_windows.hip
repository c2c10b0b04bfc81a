// nw_windows.hip -- the allele table around a cut site from a device-resident batch (gfx950):
// CRISPResso's get_row_around_cut / get_dataframe_around_cut (CRISPRessoCORE.py:801-836) per read
// instead of per full-length allele, behind the C ABI of include/crispr_alleles.h.
//
// The window of a read around cut point p is columns [cut_idx - offset + 1, cut_idx + offset + 1)
// of its aligned-read and reference rows cut to min(aln_len, awidth) columns, with Python's slice
// rules; cut_idx is the column of amplicon base p.  It is a function of the read's traceback
// runs, its bytes and the amplicon, all in HBM after an ops-mode pass (nw_batch_device_ops).
//
//   extract  one lane per (cut point, read): walk the runs to the column of base p, apply the
//            slice rule, walk again and write the window's two rows into a record in LDS; the
//            block then copies its 128 records, contiguous in the [cuts][n][stride] record
//            buffer, with coalesced dword stores.  The amplicon is staged in LDS once per block.
//   group    the records of one cut point are n "reads" of `stride` bytes at r * stride:
//            nwa::group_resident (nw_alleles.hip, the body of nwa_group_device: hash / insert /
//            verify / compaction, the collided records grouped exactly on the host) groups them
//            as it stands, on the keep flags where they lie on the device.
//   finish   unedited[g] = OR over the group's reads of cls == 0 (every writer stores the same
//            1), and the records of the groups' first reads gathered for the copy back.
// nwa_windows_device takes keep and the nwq_read records as HOST arrays, nwa_windows_resident as
// DEVICE arrays (a resident summary's d_keep / d_out): one body.
#include <cstring>

#include "nwa_device.h"

namespace nwa {

constexpr int kWinBlock = 128;        // records per block of the extract kernel
constexpr int kWinCuts = 4;           // cut points per extract launch
constexpr int kWinMaxOffset = 64;
constexpr int kWinMaxAmp = 16384;     // amplicon bytes staged in LDS

struct WinArgs {
    const uint32_t* ops;       // runs: type << 28 | length
    const int64_t* ops_off;    // [n + 1]
    const int32_t* stats;      // nw_stat records, 8 int32 each: aln_len first
    const uint8_t* reads;      // read r at reads + off[r] - bias
    const int64_t* off;
    int64_t bias;
    int64_t n;
    int awidth;
    const uint8_t* amp;
    int La;
    const uint8_t* keep;       // device copy (or null)
    int K;
    int cut[kWinCuts];
    int offset;
    int W;                     // 2 * offset
    int stride;                // 4 + 2 * W: win_len (uint32), the read row, the reference row
    uint8_t* rec;              // [K][n][stride]
    uint32_t* err;             // [0] kept (cut, read) pairs without a cut column, [1] the smallest such read
};

__global__ __launch_bounds__(kWinBlock) void window_extract_kernel(WinArgs a) {
    extern __shared__ uint32_t lds32[];
    uint8_t* amp = reinterpret_cast<uint8_t*>(lds32);                     // [La rounded up to 4]
    const int amp_words = (a.La + 3) >> 2;
    const int s4 = a.stride >> 2;
    uint32_t* mine32 = lds32 + amp_words + (int)threadIdx.x * s4;
    uint8_t* mine = reinterpret_cast<uint8_t*>(mine32);
    for (int i = threadIdx.x; i < a.La; i += kWinBlock) amp[i] = a.amp[i];
    for (int j = 0; j < s4; ++j) mine32[j] = 0;
    __syncthreads();

    const int64_t total = a.n * a.K;
    const int64_t base = (int64_t)blockIdx.x * kWinBlock;
    const int64_t i = base + threadIdx.x;
    if (i < total) {
        const int64_t r = i % a.n;
        const int cut = a.cut[i / a.n];
        if (!a.keep || a.keep[r]) {
            const int64_t q0 = a.ops_off[r], q1 = a.ops_off[r + 1];
            const int64_t o0 = a.off[r], Lb = a.off[r + 1] - o0;
            const uint8_t* rd = a.reads + (o0 - a.bias);
            int64_t len = a.stats[r * 8];
            if (len > a.awidth) len = a.awidth;
            // the column of amplicon base `cut`: in an M or a Y run (an X run holds no reference byte)
            int64_t col = 0, ia = 0, cut_idx = -1;
            for (int64_t q = q0; q < q1; ++q) {
                const uint32_t op = a.ops[q];
                const int64_t l = NW_RUN_LEN(op);
                if (NW_RUN_TYPE(op) != NW_RUN_X) {
                    if (cut < ia + l) {
                        cut_idx = col + (cut - ia);
                        break;
                    }
                    ia += l;
                }
                col += l;
            }
            if (cut_idx < 0 || cut_idx >= len) {
                atomicAdd(&a.err[0], 1u);
                atomicMin(&a.err[1], (uint32_t)r);
            } else {
                // s[cut_idx - offset + 1 : cut_idx + offset + 1] on a string of len columns
                int64_t start = cut_idx - a.offset + 1, stop = cut_idx + a.offset + 1;
                if (start < 0) {
                    start += len;
                    if (start < 0) start = 0;
                }
                if (stop > len) stop = len;
                mine32[0] = stop > start ? (uint32_t)(stop - start) : 0u;
                uint8_t* row_read = mine + 4;
                uint8_t* row_ref = row_read + a.W;
                int64_t jb = 0;
                col = 0;
                ia = 0;
                for (int64_t q = q0; q < q1 && col < stop; ++q) {
                    const uint32_t op = a.ops[q];
                    const uint32_t type = NW_RUN_TYPE(op);
                    const int64_t l = NW_RUN_LEN(op);
                    const int64_t c0 = col > start ? col : start;
                    const int64_t c1 = col + l < stop ? col + l : stop;
                    for (int64_t cc = c0; cc < c1; ++cc) {
                        const int64_t d = cc - col;
                        uint8_t rb = '-', fb = '-';
                        if (type != NW_RUN_Y) rb = jb + d < Lb ? rd[jb + d] : 0;
                        if (type != NW_RUN_X) fb = ia + d < a.La ? amp[ia + d] : 0;
                        row_read[cc - start] = rb;
                        row_ref[cc - start] = fb;
                    }
                    if (type != NW_RUN_Y) jb += l;
                    if (type != NW_RUN_X) ia += l;
                    col += l;
                }
            }
        }
    }
    __syncthreads();
    // the block's records are contiguous in HBM: coalesced dword stores
    const int64_t cnt = total - base < kWinBlock ? total - base : kWinBlock;
    if (cnt <= 0) return;
    uint32_t* out = reinterpret_cast<uint32_t*>(a.rec) + base * s4;
    const uint32_t* src = lds32 + amp_words;
    for (int64_t j = threadIdx.x; j < cnt * s4; j += kWinBlock) out[j] = src[j];
}

__global__ __launch_bounds__(256) void window_offsets_kernel(int64_t* off, int64_t n, int64_t stride) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r <= n) off[r] = r * stride;
}

__global__ __launch_bounds__(256) void window_unedited_kernel(const int32_t* gor, const uint8_t* unmod, int64_t n,
                                                              uint8_t* out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int32_t g = gor[r];
    if (g >= 0 && unmod[r]) out[g] = 1;
}

__global__ __launch_bounds__(256) void window_gather_kernel(const uint32_t* rec, const uint32_t* first, int64_t ng,
                                                            int s4, uint32_t* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ng * s4) return;
    const int64_t g = i / s4;
    out[i] = rec[(int64_t)first[g] * s4 + (i - g * s4)];
}

// unmod[r] = the nwq_read of read r has cls == 0
__global__ __launch_bounds__(256) void window_unmod_kernel(const int32_t* results, int64_t n, uint8_t* unmod) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < n) unmod[r] = results[4 * r] == 0;
}

}  // namespace nwa

using hd::fail;

namespace {

// The body of nwa_windows_device and nwa_windows_resident.  on_device: keep and read_results are
// DEVICE arrays (the kept count comes from a device reduction, cls == 0 is tested there);
// otherwise HOST arrays, copied to the device here.
int windows_body(nwa_ctx* c, const uint32_t* d_ops, const int64_t* d_ops_off, const void* d_stats, const uint8_t* d_reads,
                 const int64_t* d_offsets, int64_t reads_bias, int64_t n, int32_t awidth, const char* amplicon,
                 int32_t amp_len, const int32_t* cut_points, int32_t n_cuts, int32_t offset, const uint8_t* keep,
                 const int32_t* tag, const int32_t* read_results, bool on_device, int32_t want_group_of_read,
                 int64_t* n_groups, int64_t* n_no_cut, int64_t* first_no_cut) {
    if (!c) return NW_E_INVALID;
    c->w_tab.clear();
    c->w_cuts = 0;
    c->w_collided = 0;
    std::fill(c->w_ms, c->w_ms + 3, 0.0f);
    if (n < 0 || n > 0x7FFFFFFFll) return fail(c, NW_E_INVALID, "read count %lld out of range", (long long)n);
    if (n_cuts < 0 || (n_cuts > 0 && (!cut_points || !n_groups)) || !n_no_cut || !first_no_cut || !amplicon ||
        amp_len <= 0 || awidth <= 0)
        return fail(c, NW_E_INVALID, "null or empty argument");
    if (n > 0 && (!d_ops_off || !d_stats || !d_reads || !d_offsets || !read_results))
        return fail(c, NW_E_INVALID, "null batch array");
    if (offset < 1 || offset > nwa::kWinMaxOffset)
        return fail(c, NW_E_UNSUPPORTED, "offset %d outside 1..%d", (int)offset, nwa::kWinMaxOffset);
    if (amp_len > nwa::kWinMaxAmp)
        return fail(c, NW_E_UNSUPPORTED, "amplicon of %d bases (at most %d)", (int)amp_len, nwa::kWinMaxAmp);
    for (int32_t i = 0; i < amp_len; ++i)
        if (!std::strchr("ACGTN", amplicon[i]) || amplicon[i] == 0)
            return fail(c, NW_E_UNSUPPORTED, "amplicon byte %d at %d is not one of ACGTN", (int)(unsigned char)amplicon[i],
                        (int)i);
    for (int32_t k = 0; k < n_cuts; ++k)
        if (cut_points[k] < 0 || cut_points[k] >= amp_len)
            return fail(c, NW_E_UNSUPPORTED, "cut point %d outside the amplicon", (int)cut_points[k]);
    *n_no_cut = 0;
    *first_no_cut = -1;
    c->w_width = 2 * offset;
    c->w_cuts = n_cuts;
    c->w_tab.resize((size_t)n_cuts);
    for (int32_t k = 0; k < n_cuts; ++k) n_groups[k] = 0;
    int64_t kept = n;
    if (keep && on_device) {
        const int rc = nwa::count_kept(c, keep, n, &kept);
        if (rc != NW_OK) return rc;
    } else if (keep) {
        kept = 0;
        for (int64_t r = 0; r < n; ++r) kept += keep[r] != 0;
    }
    if (want_group_of_read)
        for (auto& t : c->w_tab) t.gor.assign((size_t)n, -1);
    if (kept == 0 || n_cuts == 0) return NW_OK;

    HIP_TRY(c, hipSetDevice(c->device));
    hipEvent_t* const wev = &c->ev[5];
    const int W = 2 * offset, stride = 4 + 2 * W, s4 = stride / 4;
    const int Kmax = std::min<int>(nwa::kWinCuts, n_cuts);
    HIP_TRY(c, c->w_rec.reserve((size_t)Kmax * (size_t)n * (size_t)stride));
    HIP_TRY(c, c->w_amp.reserve((size_t)amp_len));
    HIP_TRY(c, c->w_unmod.reserve((size_t)n));
    HIP_TRY(c, c->w_off.reserve((size_t)n + 1));
    HIP_TRY(c, c->w_err.reserve(2));
    HIP_TRY(c, c->w_gfirst.reserve((size_t)kept));
    HIP_TRY(c, c->w_gun.reserve((size_t)kept));
    hipStream_t st = c->stream;
    const uint8_t* d_keep = keep;
    if (on_device) {
        hipLaunchKernelGGL(nwa::window_unmod_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, read_results, n,
                           c->w_unmod.p);
        HIP_TRY(c, hipGetLastError());
    } else {
        if (keep) {
            HIP_TRY(c, c->d_keep.reserve((size_t)n));
            HIP_TRY(c, hipMemcpy(c->d_keep.p, keep, (size_t)n, hipMemcpyHostToDevice));
            d_keep = c->d_keep.p;
        }
        std::vector<uint8_t> unmod((size_t)n);
        for (int64_t r = 0; r < n; ++r) unmod[(size_t)r] = read_results[4 * r] == 0;
        HIP_TRY(c, hipMemcpy(c->w_unmod.p, unmod.data(), (size_t)n, hipMemcpyHostToDevice));
    }
    HIP_TRY(c, hipMemcpy(c->w_amp.p, amplicon, (size_t)amp_len, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(nwa::window_offsets_kernel, dim3((unsigned)(n / 256 + 1)), dim3(256), 0, st, c->w_off.p, n,
                       (int64_t)stride);
    HIP_TRY(c, hipGetLastError());

    std::vector<int64_t> first((size_t)kept), count((size_t)kept);
    std::vector<int32_t> gor((size_t)n);
    std::vector<uint32_t> first32, recs;
    for (int32_t k0 = 0; k0 < n_cuts; k0 += nwa::kWinCuts) {
        const int K = std::min<int>(nwa::kWinCuts, n_cuts - k0);
        nwa::WinArgs a;
        a.ops = d_ops;
        a.ops_off = d_ops_off;
        a.stats = static_cast<const int32_t*>(d_stats);
        a.reads = d_reads;
        a.off = d_offsets;
        a.bias = reads_bias;
        a.n = n;
        a.awidth = awidth;
        a.amp = c->w_amp.p;
        a.La = amp_len;
        a.keep = d_keep;
        a.K = K;
        for (int k = 0; k < nwa::kWinCuts; ++k) a.cut[k] = k < K ? cut_points[k0 + k] : 0;
        a.offset = offset;
        a.W = W;
        a.stride = stride;
        a.rec = c->w_rec.p;
        a.err = c->w_err.p;
        const uint32_t err0[2] = {0u, 0xFFFFFFFFu};
        HIP_TRY(c, hipMemcpyAsync(c->w_err.p, err0, sizeof err0, hipMemcpyHostToDevice, st));
        const int64_t blocks = (n * K + nwa::kWinBlock - 1) / nwa::kWinBlock;
        const size_t lds = sizeof(uint32_t) * ((size_t)((amp_len + 3) >> 2) + (size_t)nwa::kWinBlock * s4);
        HIP_TRY(c, hipEventRecord(wev[0], st));
        hipLaunchKernelGGL(nwa::window_extract_kernel, dim3((unsigned)blocks), dim3(nwa::kWinBlock), lds, st, a);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(wev[1], st));
        uint32_t err[2] = {0, 0};
        HIP_TRY(c, hipMemcpyAsync(err, c->w_err.p, sizeof err, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, wev[0], wev[1]));
        c->w_ms[0] += ms;
        if (err[0]) {                 // the reference's ValueError: the caller raises, nothing is kept
            *n_no_cut = err[0];
            *first_no_cut = err[1];
            c->w_tab.clear();
            c->w_cuts = 0;
            for (int32_t k = 0; k < n_cuts; ++k) n_groups[k] = 0;
            return NW_OK;
        }
        for (int k = 0; k < K; ++k) {
            nwa::WinTable& t = c->w_tab[(size_t)(k0 + k)];
            const uint8_t* rec_k = c->w_rec.p + (size_t)k * (size_t)n * (size_t)stride;
            int64_t ng = 0;
            const int rc = nwa::group_resident(c, rec_k, c->w_off.p, 0, n, d_keep, kept, tag, first.data(), count.data(),
                                               kept, gor.data(), &ng, &ms);
            if (rc != NW_OK) return rc;
            if (ng <= 0 || ng > kept) return fail(c, NW_E_STATE, "inconsistent window group count");
            c->w_ms[1] += ms;
            c->w_collided += c->collided;
            // collided records were regrouped on the host: the device copy of group_of_read follows
            if (c->collided)
                HIP_TRY(c, hipMemcpyAsync(c->d_gor.p, gor.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
            first32.resize((size_t)ng);
            for (int64_t g = 0; g < ng; ++g) first32[(size_t)g] = (uint32_t)first[(size_t)g];
            HIP_TRY(c, c->w_gwin.reserve((size_t)ng * (size_t)stride));
            HIP_TRY(c, hipMemcpyAsync(c->w_gfirst.p, first32.data(), sizeof(uint32_t) * (size_t)ng, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemsetAsync(c->w_gun.p, 0, (size_t)ng, st));
            HIP_TRY(c, hipEventRecord(wev[0], st));
            hipLaunchKernelGGL(nwa::window_unedited_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                               c->d_gor.p, c->w_unmod.p, n, c->w_gun.p);
            HIP_TRY(c, hipGetLastError());
            hipLaunchKernelGGL(nwa::window_gather_kernel, dim3((unsigned)((ng * s4 + 255) / 256)), dim3(256), 0, st,
                               reinterpret_cast<const uint32_t*>(rec_k), c->w_gfirst.p, ng, s4,
                               reinterpret_cast<uint32_t*>(c->w_gwin.p));
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(wev[1], st));
            t.unedited.resize((size_t)ng);
            recs.resize((size_t)ng * (size_t)s4);
            HIP_TRY(c, hipMemcpyAsync(t.unedited.data(), c->w_gun.p, (size_t)ng, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipMemcpyAsync(recs.data(), c->w_gwin.p, (size_t)ng * (size_t)stride, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipStreamSynchronize(st));
            HIP_TRY(c, hipEventElapsedTime(&ms, wev[0], wev[1]));
            c->w_ms[2] += ms;
            t.first.assign(first.begin(), first.begin() + ng);
            t.count.assign(count.begin(), count.begin() + ng);
            t.win_len.resize((size_t)ng);
            t.win.resize((size_t)ng * 2 * (size_t)W);
            for (int64_t g = 0; g < ng; ++g) {
                const uint32_t* rg = recs.data() + (size_t)g * (size_t)s4;
                t.win_len[(size_t)g] = (int32_t)rg[0];
                std::memcpy(t.win.data() + (size_t)g * 2 * (size_t)W, rg + 1, 2 * (size_t)W);
            }
            if (want_group_of_read) t.gor = gor;
            n_groups[k0 + k] = ng;
        }
    }
    return NW_OK;
}

}  // namespace

extern "C" {

int nwa_windows_device(nwa_ctx* c, const uint32_t* d_ops, const int64_t* d_ops_off, const void* d_stats,
                       const uint8_t* d_reads, const int64_t* d_offsets, int64_t reads_bias, int64_t n, int32_t awidth,
                       const char* amplicon, int32_t amp_len, const int32_t* cut_points, int32_t n_cuts, int32_t offset,
                       const uint8_t* keep, const int32_t* tag, const int32_t* read_results, int32_t want_group_of_read,
                       int64_t* n_groups, int64_t* n_no_cut, int64_t* first_no_cut) {
    return windows_body(c, d_ops, d_ops_off, d_stats, d_reads, d_offsets, reads_bias, n, awidth, amplicon, amp_len,
                        cut_points, n_cuts, offset, keep, tag, read_results, false, want_group_of_read, n_groups, n_no_cut,
                        first_no_cut);
}

int nwa_windows_resident(nwa_ctx* c, const uint32_t* d_ops, const int64_t* d_ops_off, const void* d_stats,
                         const uint8_t* d_reads, const int64_t* d_offsets, int64_t reads_bias, int64_t n, int32_t awidth,
                         const char* amplicon, int32_t amp_len, const int32_t* cut_points, int32_t n_cuts, int32_t offset,
                         const uint8_t* d_keep, const int32_t* tag, const int32_t* d_results, int32_t want_group_of_read,
                         int64_t* n_groups, int64_t* n_no_cut, int64_t* first_no_cut) {
    return windows_body(c, d_ops, d_ops_off, d_stats, d_reads, d_offsets, reads_bias, n, awidth, amplicon, amp_len,
                        cut_points, n_cuts, offset, d_keep, tag, d_results, true, want_group_of_read, n_groups, n_no_cut,
                        first_no_cut);
}

int nwa_windows_fetch(const nwa_ctx* c, int32_t k, uint8_t* win, int32_t* win_len, int64_t* first, int64_t* count,
                      uint8_t* unedited, int32_t* group_of_read) {
    if (!c || k < 0 || k >= c->w_cuts) return NW_E_INVALID;
    const nwa::WinTable& t = c->w_tab[(size_t)k];
    if (group_of_read && t.gor.empty() && !t.first.empty()) return NW_E_STATE;
    if (win && !t.win.empty()) std::memcpy(win, t.win.data(), t.win.size());
    if (win_len && !t.win_len.empty()) std::memcpy(win_len, t.win_len.data(), sizeof(int32_t) * t.win_len.size());
    if (first && !t.first.empty()) std::memcpy(first, t.first.data(), sizeof(int64_t) * t.first.size());
    if (count && !t.count.empty()) std::memcpy(count, t.count.data(), sizeof(int64_t) * t.count.size());
    if (unedited && !t.unedited.empty()) std::memcpy(unedited, t.unedited.data(), t.unedited.size());
    if (group_of_read && !t.gor.empty()) std::memcpy(group_of_read, t.gor.data(), sizeof(int32_t) * t.gor.size());
    return NW_OK;
}

int64_t nwa_windows_collided(const nwa_ctx* c) { return c ? c->w_collided : -1; }

int nwa_windows_times(const nwa_ctx* c, float* ms) {
    if (!c || !ms) return NW_E_INVALID;
    std::memcpy(ms, c->w_ms, sizeof c->w_ms);
    return NW_OK;
}

}  // extern "C"
