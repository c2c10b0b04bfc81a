// nw_allele_rows.hip -- the allele table's rows from a device-resident batch (gfx950): the groups of
// byte-identical kept reads (nw_alleles.hip, with the keep flags already in HBM) and, for the first
// read of every group, the aligned-read row and the reference row that CRISPResso's allele table
// holds (CRISPRessoCORE.py:2923-2946), behind the C ABI of include/crispr_alleles.h.  The rows are
// a function of the read's traceback runs, its bytes and the amplicon, all in HBM after an
// ops-mode pass (nw_batch_device_ops): no read's text is needed on the host, and only
// groups x 2 x row_stride bytes come back.
//
//   columns  one lane per group: min(aln_len, awidth) of the group's first read, the largest of
//            them by atomicMax (the host sizes the row buffer from it).
//   rows     one wavefront per group: the runs of the first read in steps of 64 (lane l takes run
//            l of the step; three inclusive scans give every run its first column, amplicon base
//            and read byte), then run by run the lanes take consecutive columns of the run, so
//            the byte stores of a run are coalesced.  Columns past min(aln_len, awidth) are not
//            written, the row is zero-filled from there to row_stride.  A byte index past the
//            read or the amplicon writes 0 and is never loaded; runs that do not end at both
//            ends, an unknown run type or fewer columns than the record says set the error word.
//            Lanes 0..3 copy the read's nwq_read, lane 0 the group's cols / first / count.
#include <cstring>

#include "group_device.h"
#include "nwa_device.h"

namespace nwa {

struct RowArgs {
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
    const int32_t* results;    // nwq_read [n]: 4 int32 each
    const uint32_t* gfirst;    // [ng] the groups' first reads, ascending
    const uint32_t* gcount;    // [ng]
    int64_t ng;
    int stride;
    uint8_t* rows;             // [ng][2][stride]
    int32_t* cols;             // [ng]
    int64_t* first;
    int64_t* count;
    int32_t* res;              // [ng][4]
    uint32_t* err;             // [0] error word, [1] the largest column count
};

__device__ inline int row_columns(const RowArgs& a, int64_t r) {
    int len = a.stats[r * 8];
    if (len < 0) len = 0;
    return len < a.awidth ? len : a.awidth;
}

__global__ __launch_bounds__(256) void allele_cols_kernel(RowArgs a) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.ng) return;
    const int64_t r = a.gfirst[g];
    if (r >= a.n) {
        a.err[0] = 1;
        return;
    }
    atomicMax(&a.err[1], (uint32_t)row_columns(a, r));
}

// inclusive scan of one 64-bit value per lane over the wavefront
__device__ inline int64_t wave_scan64(int64_t v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const int lo = __shfl_up((int)(uint32_t)(uint64_t)v, o, 64);
        const int hi = __shfl_up((int)(uint32_t)((uint64_t)v >> 32), o, 64);
        if (lane >= o) v += (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
    }
    return v;
}

__global__ __launch_bounds__(256) void allele_rows_kernel(RowArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t g = wave; g < a.ng; g += nwaves) {
        const int64_t r = a.gfirst[g];
        uint8_t* row_read = a.rows + g * 2 * (int64_t)a.stride;
        uint8_t* row_ref = row_read + a.stride;
        bool bad = r >= a.n;
        int64_t cols = 0, col = 0;
        if (!bad) {
            const int64_t q0 = a.ops_off[r], q1 = a.ops_off[r + 1];
            const int64_t o0 = a.off[r], Lb = a.off[r + 1] - o0;
            const uint8_t* rd = a.reads + (o0 - a.bias);
            cols = row_columns(a, r);
            if (cols > a.stride) cols = a.stride;
            int64_t ia = 0, jb = 0;                           // the totals before this step (wave-uniform)
            for (int64_t qb = q0; qb < q1; qb += 64) {
                const int64_t q = qb + lane;
                const uint32_t op = q < q1 ? a.ops[q] : 0u;   // (past the end: an M run of no column)
                const uint32_t type = NW_RUN_TYPE(op);
                const int64_t len = NW_RUN_LEN(op);
                if (type > NW_RUN_Y) bad = true;
                const int64_t c_inc = wave_scan64(len, lane);
                const int64_t a_inc = wave_scan64(type == NW_RUN_M || type == NW_RUN_Y ? len : 0, lane);
                const int64_t b_inc = wave_scan64(type == NW_RUN_M || type == NW_RUN_X ? len : 0, lane);
                const int cnt = q1 - qb < 64 ? (int)(q1 - qb) : 64;
                for (int j = 0; j < cnt; ++j) {
                    const uint32_t op_j = (uint32_t)__shfl((int)op, j, 64);
                    const uint32_t t = NW_RUN_TYPE(op_j);
                    const int64_t l = NW_RUN_LEN(op_j);
                    const int64_t c0 = col + (int64_t)grp::shfl64((uint64_t)c_inc, j) - l;
                    if (c0 >= cols) break;                    // (wave-uniform: the rest is cut off)
                    const int64_t a0 = ia + (int64_t)grp::shfl64((uint64_t)a_inc, j) - (t == NW_RUN_M || t == NW_RUN_Y ? l : 0);
                    const int64_t b0 = jb + (int64_t)grp::shfl64((uint64_t)b_inc, j) - (t == NW_RUN_M || t == NW_RUN_X ? l : 0);
                    const int64_t lim = l < cols - c0 ? l : cols - c0;
                    for (int64_t k = lane; k < lim; k += 64) {
                        uint8_t rb = '-', fb = '-';
                        if (t == NW_RUN_M || t == NW_RUN_X) rb = b0 + k < Lb ? rd[b0 + k] : (uint8_t)0;
                        if (t == NW_RUN_M || t == NW_RUN_Y) fb = a0 + k < a.La ? a.amp[a0 + k] : (uint8_t)0;
                        if (t > NW_RUN_Y) rb = fb = 0;
                        row_read[c0 + k] = rb;
                        row_ref[c0 + k] = fb;
                    }
                }
                col += (int64_t)grp::shfl64((uint64_t)c_inc, 63);
                ia += (int64_t)grp::shfl64((uint64_t)a_inc, 63);
                jb += (int64_t)grp::shfl64((uint64_t)b_inc, 63);
            }
            // nw_expand_ops_subset's rule: the runs end at both ends (a read without a byte and
            // without a run has an empty row), and they hold the columns the record counts
            if (!(q1 == q0 && Lb == 0) && (ia != a.La || jb != Lb)) bad = true;
            if (col < cols) bad = true;
        }
        const int64_t written = col < cols ? col : cols;
        for (int64_t k = written + lane; k < a.stride; k += 64) {
            row_read[k] = 0;
            row_ref[k] = 0;
        }
        if (lane < 4) a.res[g * 4 + lane] = r >= a.n ? 0 : a.results[r * 4 + lane];
        if (lane == 0) {
            a.cols[g] = (int32_t)cols;
            a.first[g] = r;
            a.count[g] = a.gcount[g];
        }
        if (__ballot(bad) && lane == 0) a.err[0] = 1;
    }
}

}  // namespace nwa

using hd::fail;

extern "C" {

int nwa_table_device(nwa_ctx* c, const uint32_t* d_ops, const int64_t* d_ops_off, const void* d_stats,
                     const uint8_t* d_reads, const int64_t* d_offsets, int64_t reads_bias, int64_t n, int32_t awidth,
                     const char* amplicon, int32_t amp_len, const uint8_t* d_keep, const int32_t* d_results,
                     int64_t* n_groups, int32_t* row_stride) {
    if (!c) return NW_E_INVALID;
    c->t_groups = 0;
    c->t_collided = 0;
    c->t_stride = 0;
    c->t_ms[0] = c->t_ms[1] = 0.0f;
    if (n < 0 || n > 0x7FFFFFFFll) return fail(c, NW_E_INVALID, "read count %lld out of range", (long long)n);
    if (!n_groups || !row_stride || !amplicon || amp_len <= 0 || awidth <= 0)
        return fail(c, NW_E_INVALID, "null or empty argument");
    if (n > 0 && (!d_ops_off || !d_stats || !d_reads || !d_offsets || !d_results))
        return fail(c, NW_E_INVALID, "null batch array");
    *n_groups = 0;
    *row_stride = 0;
    int64_t kept = n;
    int rc = nwa::count_kept(c, d_keep, n, &kept);
    if (rc != NW_OK) return rc;
    if (kept == 0) return NW_OK;

    std::vector<int64_t> first((size_t)kept), count((size_t)kept);
    int64_t ng = 0;
    rc = nwa::group_resident(c, d_reads, d_offsets, reads_bias, n, d_keep, kept, nullptr, first.data(), count.data(), kept,
                             nullptr, &ng, &c->t_ms[0]);
    if (rc != NW_OK) return rc;
    if (ng <= 0 || ng > kept) return fail(c, NW_E_STATE, "inconsistent group count");
    c->t_collided = c->collided;
    hipStream_t st = c->stream;
    if (c->collided) {          // the lists merged with the host's exact groups replace the device's
        std::vector<uint32_t> f32((size_t)ng), c32((size_t)ng);
        for (int64_t g = 0; g < ng; ++g) {
            f32[(size_t)g] = (uint32_t)first[(size_t)g];
            c32[(size_t)g] = (uint32_t)count[(size_t)g];
        }
        HIP_TRY(c, hipMemcpy(c->d_gfirst.p, f32.data(), sizeof(uint32_t) * (size_t)ng, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(c->d_gcount.p, c32.data(), sizeof(uint32_t) * (size_t)ng, hipMemcpyHostToDevice));
    }
    HIP_TRY(c, c->t_amp.reserve((size_t)amp_len));
    HIP_TRY(c, c->t_err.reserve(2));
    HIP_TRY(c, c->t_cols.reserve((size_t)ng));
    HIP_TRY(c, c->t_first.reserve((size_t)ng));
    HIP_TRY(c, c->t_count.reserve((size_t)ng));
    HIP_TRY(c, c->t_res.reserve(4 * (size_t)ng));
    HIP_TRY(c, hipMemcpy(c->t_amp.p, amplicon, (size_t)amp_len, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemsetAsync(c->t_err.p, 0, sizeof(uint32_t) * 2, st));

    nwa::RowArgs a;
    a.ops = d_ops;
    a.ops_off = d_ops_off;
    a.stats = static_cast<const int32_t*>(d_stats);
    a.reads = d_reads;
    a.off = d_offsets;
    a.bias = reads_bias;
    a.n = n;
    a.awidth = awidth;
    a.amp = c->t_amp.p;
    a.La = amp_len;
    a.results = d_results;
    a.gfirst = c->d_gfirst.p;
    a.gcount = c->d_gcount.p;
    a.ng = ng;
    a.stride = 0;
    a.rows = nullptr;
    a.cols = c->t_cols.p;
    a.first = c->t_first.p;
    a.count = c->t_count.p;
    a.res = c->t_res.p;
    a.err = c->t_err.p;
    hipEvent_t* const tev = &c->ev[5];
    uint32_t err[2] = {0, 0};
    float ms = 0;
    HIP_TRY(c, hipEventRecord(tev[0], st));
    hipLaunchKernelGGL(nwa::allele_cols_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(tev[1], st));
    HIP_TRY(c, hipMemcpyAsync(err, c->t_err.p, sizeof err, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipEventElapsedTime(&ms, tev[0], tev[1]));
    c->t_ms[1] = ms;
    if (err[0]) return fail(c, NW_E_STATE, "a group's first read is outside the batch");
    if ((int64_t)err[1] > (int64_t)awidth) return fail(c, NW_E_STATE, "inconsistent column count");
    const int stride = std::max(16, (int)((err[1] + 15u) & ~15u));
    HIP_TRY(c, c->t_rows.reserve((size_t)ng * 2 * (size_t)stride));
    a.stride = stride;
    a.rows = c->t_rows.p;
    const unsigned grid = (unsigned)std::min<int64_t>((ng + 3) / 4, (int64_t)16 * c->num_cus);
    HIP_TRY(c, hipEventRecord(tev[0], st));
    hipLaunchKernelGGL(nwa::allele_rows_kernel, dim3(grid), dim3(256), 0, st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(tev[1], st));
    HIP_TRY(c, hipMemcpyAsync(err, c->t_err.p, sizeof err, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipEventElapsedTime(&ms, tev[0], tev[1]));
    c->t_ms[1] += ms;
    if (err[0])
        return fail(c, NW_E_INVALID, "the runs of a group's first read do not match its bytes, the amplicon or its record");
    c->t_groups = ng;
    c->t_stride = stride;
    *n_groups = ng;
    *row_stride = stride;
    return NW_OK;
}

int nwa_table_fetch(nwa_ctx* c, uint8_t* rows, int32_t* cols, int64_t* first, int64_t* count, int32_t* results) {
    if (!c) return NW_E_INVALID;
    const size_t ng = (size_t)c->t_groups;
    if (ng == 0) return NW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (rows) HIP_TRY(c, hipMemcpy(rows, c->t_rows.p, ng * 2 * (size_t)c->t_stride, hipMemcpyDeviceToHost));
    if (cols) HIP_TRY(c, hipMemcpy(cols, c->t_cols.p, sizeof(int32_t) * ng, hipMemcpyDeviceToHost));
    if (first) HIP_TRY(c, hipMemcpy(first, c->t_first.p, sizeof(int64_t) * ng, hipMemcpyDeviceToHost));
    if (count) HIP_TRY(c, hipMemcpy(count, c->t_count.p, sizeof(int64_t) * ng, hipMemcpyDeviceToHost));
    if (results) HIP_TRY(c, hipMemcpy(results, c->t_res.p, sizeof(int32_t) * 4 * ng, hipMemcpyDeviceToHost));
    return NW_OK;
}

int64_t nwa_table_collided(const nwa_ctx* c) { return c ? c->t_collided : -1; }

int nwa_table_times(const nwa_ctx* c, float* ms) {
    if (!c || !ms) return NW_E_INVALID;
    std::memcpy(ms, c->t_ms, sizeof c->t_ms);
    return NW_OK;
}

}  // extern "C"
