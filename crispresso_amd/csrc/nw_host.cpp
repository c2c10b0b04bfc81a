// nw_host.cpp -- C ABI (include/crispr_nw.h) over the gfx950 alignment kernel.
//
// Owns one HIP stream and the device buffers of one GPU.  Everything the
// reference did by spawning `needle` (CRISPRessoCORE.py:1788-1936) happens here
// in-process: the amplicon becomes a substitution profile in HBM, reads are
// copied once, one kernel aligns the whole batch, results come back as the
// three alignment strings plus per-read statistics.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/crispr_nw.h"
#include "front_device.h"
#include "host_dev.h"
#include "host_pool.h"
#include "nw_device.h"
#include "nw_edna.h"

namespace {

constexpr int kMaxRef = 8192;       // the exact multi-wave kernel (nw_exact.hip)
constexpr int kMaxRefWave = 1024;   // the band, stream and one-wave kernels
constexpr int kMaxLds = 160 * 1024;

using hd::DevBuf;
using hd::fail;

}  // namespace

// One amplicon's device tables (pointers into nw_ctx::d_arena).
struct Profile {
    const int8_t* prof = nullptr;      // [NCODE][64][RP] int8: exact kernel
    const uint32_t* rowpos = nullptr;  // band walk: codes each row scores > 0 against
    const uint8_t* amp = nullptr;      // amplicon bytes (+16 pad)
    int R = 0;
    // window seeds (classify, packed input): the amplicon 2 bits per base (the reads' packing) and
    // its A C G T 16-mers sorted by (key, position); null for amplicons over 1024 bp
    const uint32_t* amp2 = nullptr;
    const uint32_t* seed_key = nullptr;
    const uint16_t* seed_pos = nullptr;
    int32_t n_seed = 0;
    // classify's LDS image of the amplicon (cls_image): copied as it is by every block
    const uint32_t* cls_img = nullptr;
    int32_t cls_words = 0;
    int32_t sub12_words = 0;           // the image's self-mismatch prefix counts (its last words; 0: none)
    bool amp_acgt = false;             // every amplicon byte A C G T (either case)
};

// Device buffers of one chunk's kernels.  The pipelined calls alternate two sets on
// two compute streams, so a chunk's latency-bound tail (second band level, exact
// kernel, compaction) overlaps the next chunk's bulk kernels.
struct Scratch {
    DevBuf<uint8_t> d_tb;              // exact kernel: traceback slabs when they do not fit LDS
    DevBuf<int64_t> d_fallback;        // reads the 16 / 32-diagonal levels gave up on (the wide level's input)
    DevBuf<int32_t> d_seed;            // seeded band: per read of the chunk, its hits' diagonals (seed_pack)
    DevBuf<int32_t> d_seed2;           // ... and its blocks' facts for the refined certificate (seed2_pack)
    DevBuf<int32_t> d_seed_list;       // seeded band: the chunk's seeded reads (the segment sort's third list)
    DevBuf<uint8_t> d_seed_flags;      // ... per entry: left to the wide level by the 32-diagonal level
    DevBuf<int32_t> d_seed_list2;      // ... those entries, in order (the wide level's seeded list)
    DevBuf<int64_t> d_fallback2;       // reads the wide level gave up on (the exact kernel's list)
    DevBuf<int32_t> d_fallback_count;  // the chunk's counters (nw::ChunkCounter)
    DevBuf<int32_t> d_redo;            // reads the first band level could not certify
    DevBuf<uint8_t> d_redo_flags;      // per sorted position: handed to the second level
    DevBuf<int32_t> d_order, d_sort_key;
    DevBuf<int32_t> d_cert_q, d_cert_cnt;   // classify's queues for nw_band_cert (KernelArgs::cert_q)
    DevBuf<unsigned long long> d_lb;   // look-back words of the single-pass scans (sort, redo list, ops)
    DevBuf<uint8_t> d_bregion;         // band regions (per read pair)
    DevBuf<int32_t> d_wf_list;         // wide first: the segment sort's list of those reads
    DevBuf<uint8_t> d_wf_region;       // ... and their launch's band regions (it runs beside the first level)
    DevBuf<uint32_t> d_slots, d_spill, d_staging;   // ops output: run slots, spill area, compaction output
    DevBuf<int32_t> d_nops, d_opsctl;
};
constexpr int kScratchSets = 6;   // 3 per pass of a dual call, 3 otherwise
constexpr int kComputeStreams = 3;
constexpr int64_t kWidePairs = 2048;     // read pairs of one chunk's wide level (region capacity)
constexpr int64_t kWideFirstPairs = 4096;   // read pairs of the wide-first launch (its region; twice this: its cap)

// Test switches (environment, read_switches() at every public entry point that uses one: a value
// set between two calls holds for the second).  Each forces a path the defaults reach only on
// particular inputs, so the tests can hold every path to the oracle.
struct Switches {
    // CRISPR_NW_KERNEL: "full": every read through the exact int32 kernel (no band); "diag32":
    // the band path without its 16-diagonal level
    bool band = true, diag32 = false;
    // CRISPR_NW_EXACT: "multi[:grid]": the exact work lists through the multi-wave kernel (the
    // first `grid` entries, the rest through the one-wave kernel; 0: no `:grid`); "lds": the
    // one-wave kernel keeps its traceback in LDS however few waves fit
    bool exact_multi = false, exact_lds = false;
    int exact_multi_grid = 0;
    bool wide = true;                  // CRISPR_NW_WIDE "0": no 128-diagonal level
    bool wide_first = true;            // CRISPR_NW_WIDE_FIRST "0": no wide-first list (its reads wait for the wide level)
    int64_t wide_first_cap = 2 * kWideFirstPairs;   // CRISPR_NW_WIDE_FIRST_CAP: reads of a chunk's list run beside the first level
    bool sub12_table = true;           // CRISPR_NW_SUB12_TABLE "0": classify's one- / two-substitution checks by word passes
    bool indel_onepass = true;         // CRISPR_NW_INDEL_ONEPASS "0": the one-indel check's two long diagonals by scans
    int direct = -1;                   // CRISPR_NW_DIRECT: reads up to which the first level hands straight to the wide level
    bool l1skip = true;                // CRISPR_NW_L1SKIP "0": chunks of >= 65536 reads with few DP reads keep the first level
    bool adapt = true;                 // CRISPR_NW_ADAPT "0": no adaptive level choice across chunks
    bool seed32 = true;                // CRISPR_NW_SEED32 "0": the seeded list straight to the wide level
    int64_t chunk = 262144;            // CRISPR_NW_CHUNK: reads per chunk of a call
    int ops_slot = nw::kOpsSlot;       // CRISPR_NW_OPS_SLOT: runs per read slot (tests force spills)
    int64_t spill_words = (64ll << 20) / 4;   // CRISPR_NW_SPILL_WORDS
    int64_t region_bytes = 16ll << 30; // CRISPR_NW_REGION_MB: the band regions' cap
    int trace = 0;                     // CRISPR_NW_TRACE (diagnostics): an event after every launch of the call's last chunks
    bool host_timing = false;          // CRISPR_NW_HOST_TIMING=1 (diagnostics): the host's phase split of a call on stderr
};

static Switches read_switches() {
    Switches w;
    auto off = [](const char* name) {   // set, and a number that is 0
        const char* e = std::getenv(name);
        return e && std::atoi(e) == 0;
    };
    const char* kern = std::getenv("CRISPR_NW_KERNEL");
    w.band = !kern || std::strncmp(kern, "diag", 4) == 0;
    w.diag32 = kern && std::strcmp(kern, "diag32") == 0;
    if (const char* e = std::getenv("CRISPR_NW_EXACT")) {
        w.exact_lds = std::strcmp(e, "lds") == 0;
        w.exact_multi = std::strncmp(e, "multi", 5) == 0;
        if (w.exact_multi && e[5] == ':') w.exact_multi_grid = std::max(1, std::atoi(e + 6));
    }
    w.wide = !off("CRISPR_NW_WIDE");
    w.wide_first = !off("CRISPR_NW_WIDE_FIRST");
    if (const char* e = std::getenv("CRISPR_NW_WIDE_FIRST_CAP")) w.wide_first_cap = std::max(0ll, std::atoll(e));
    w.sub12_table = !off("CRISPR_NW_SUB12_TABLE");
    w.indel_onepass = !off("CRISPR_NW_INDEL_ONEPASS");
    if (const char* e = std::getenv("CRISPR_NW_DIRECT")) w.direct = std::max(0, std::atoi(e));
    w.l1skip = !off("CRISPR_NW_L1SKIP");
    if (const char* e = std::getenv("CRISPR_NW_ADAPT")) w.adapt = std::strcmp(e, "0") != 0;
    w.seed32 = !off("CRISPR_NW_SEED32");
    if (const char* e = std::getenv("CRISPR_NW_CHUNK")) w.chunk = std::max(1ll, std::atoll(e));
    if (const char* e = std::getenv("CRISPR_NW_OPS_SLOT")) w.ops_slot = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("CRISPR_NW_SPILL_WORDS")) w.spill_words = std::max(1ll, std::atoll(e));
    if (const char* e = std::getenv("CRISPR_NW_REGION_MB")) w.region_bytes = std::max(1ll, std::atoll(e)) << 20;
    if (const char* e = std::getenv("CRISPR_NW_TRACE")) w.trace = std::atoi(e);
    if (const char* e = std::getenv("CRISPR_NW_HOST_TIMING")) w.host_timing = std::strcmp(e, "1") == 0;
    return w;
}

// What configure() decides for one amplicon and one batch shape: path choice, launch
// configurations, geometry.  A pooled call keeps one per group and assigns it per chunk.
struct AmpConfig {
    nw::LaunchCfg cfg{};              // full-storage kernel
    // certified diagonal-band kernels (nw_band_device.h, the stage files): the default path
    bool use_diag = false;
    nw::LaunchCfg diag_fill{}, diag_walk{};          // 32-diagonal level (the certificate's last resort)
    nw::LaunchCfg diag16_fill{}, diag16_walk{};      // 16-diagonal first level (0 grid: off)
    int64_t diag16_pass_pairs = 0, diag16_stride = 0;
    int64_t diag_pass_pairs = 0, diag_stride = 0;
    int diag_words = 0, diag_lb_cap = 0;
    // the wide level (kWideDiags diagonals, one read pair per wavefront) over what the 16 / 32
    // levels gave up on, before the exact kernel (0 grid: off)
    nw::LaunchCfg wide_fill{}, wide_walk{};
    int64_t wide_pairs = 0, wide_stride = 0;
    int wide_words = 0, wide_lb_cap = 0;
    // wide first: the wide level's kernels over the segment sort's wide-first list, on
    // the second compute stream beside the first level (0 pairs: off)
    nw::LaunchCfg wf_fill{}, wf_walk{};
    int64_t wf_pairs = 0;
    int wf_cap = 0;
    // exact multi-wave kernel on work lists (0 grid: the one-wave kernel, cfg)
    int exact_grid = 0, exact_lds = 0;
    bool exact_tb_lds = true;
    bool exact_full = false;          // long amplicon: every read through the multi-wave kernel
    int64_t exact_slab = 0;
    int64_t stride = 0;               // bytes per output row
};

// What an ops_call decides once for all its chunks; reset on every exit (CallReset).
struct CallState {
    // seeded band: reads the 16-diagonal band cannot hold (La - Lb >= 16) go to the
    // wide level centred on their 16-mer hits; seed_pairs widens the wide level's region for
    // them, seed_keys their sort keys
    bool seed_on = false;
    // the seeded list through the second level (32 diagonals, 4 pairs per wavefront) before the wide
    // level, which takes what it leaves (KernelArgs::seed_l2)
    bool seed_l2 = true;
    int64_t seed_pairs = 0;
    int32_t seed_keys = 0;
    size_t trace_used = 0;            // entries of nw_ctx::trace_ev the call's launches marked
};

// What launch_range reports back (nw_ctx::last_launch keeps the newest for the getters).
struct ChunkLaunch {
    bool seed_chunk = false, wf_chunk = false;
    int redo_direct = 0;              // the launch's KernelArgs::redo_direct
    hipStream_t cs = nullptr;         // the stream it ended on (the tail stream after a split)
};

// known copies: one known sequence's alignment (a dual call has one per pass)
struct KnownSet {
    DevBuf<uint8_t> d_kbytes, d_ktb;
    DevBuf<int64_t> d_koff, d_kfb;
    DevBuf<uint32_t> d_k2, d_kslots;
    DevBuf<nw::Stat> d_kstat;
    DevBuf<int32_t> d_kmisc;   // [0] nops, [1..2] ops_ctl, [8..16) fallback counts
    hipEvent_t ev_known = nullptr;
    bool on = false;
    ~KnownSet() {
        if (ev_known) (void)hipEventDestroy(ev_known);
    }
};

// One launch_range / launch_range_ops: what its caller decides for these reads.
struct ChunkPlan {
    const Switches* sw = nullptr;
    Scratch* s = nullptr;             // the scratch set
    hipStream_t cs = nullptr;         // the compute stream
    // tail split (ops_call): the chunk's first band level on cs, then split_ev recorded there and
    // the rest (second level, exact kernel, compaction) on split_to
    hipStream_t split_to = nullptr;
    hipEvent_t split_ev = nullptr;
    int64_t n = 0;                    // reads
    bool ops = false;                 // ops output (runs into slots), else rows
    bool skip16 = false;              // the 32-diagonal level only (ops_call's adaptive choice)
    bool exact_small = false;         // the exact kernel's work list on a small grid
    bool lane = false;                // the first level's lane walk + stop summary
    bool wide_first_ok = false;       // the other compute stream is free for the wide-first launch
    bool phase_events = false;        // record the phase events between the kernels (resident passes)
    const KnownSet* known = nullptr;  // the prepared known set, if any
    // a dual call: the chunk's pass writes its records and run offsets at d_stats / d_opsoff +
    // out_off and keeps its running base in ctl block ctl_pass
    int64_t out_off = 0;
    int ctl_pass = 0;
    nw::KernelArgs pk{};              // the packed-input fields (pk_*): classify decodes the reads
    int64_t* zero_ctl = nullptr;      // classify zeroes the compaction's control block
    bool trace = false;               // diagnostics: an event after every launch, named by `chunk`
    int chunk = 0;
    ChunkPlan(const Switches& w, Scratch* set, hipStream_t stream, int64_t reads, bool ops_out)
        : sw(&w), s(set), cs(stream), n(reads), ops(ops_out) {}
};

struct nw_ctx {
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    Scratch sc[kScratchSets];                          // [0]: the nw_batch_* API's and the rows calls'
    hipStream_t cstream[kComputeStreams] = {};            // compute stream of each set ([0] = stream)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_fill = nullptr, ev_walk = nullptr;   // after the fill / walk kernels
    hipEvent_t ev_sort = nullptr, ev_l2 = nullptr;     // band path: after the sort, after the second level
    std::string err;
    // params
    int scale = 2, gap_open = 20, gap_extend = 1;
    bool end_weight = false;           // needle -endweight: end gaps cost end_open + (k-1) end_extend
    int end_open = 20, end_extend = 1; // scaled
    // reference
    std::string ref;
    DevBuf<uint8_t> d_arena;          // every amplicon's tables (upload_profiles)
    // what d_arena / the shared tables hold (a repeated pooled call reuses them)
    std::vector<std::string> arena_refs;
    std::vector<Profile> arena_profs;
    std::string arena_key, shared_key;
    Profile cur{};                    // the amplicon being aligned
    DevBuf<uint8_t> d_lut6, d_lut;
    // batch
    int64_t n = 0;                    // reads of the uploaded batch (0 after a call)
    int32_t lb_max = 0;
    int64_t cells = 0;
    std::vector<int32_t> read_lens;
    DevBuf<uint8_t> d_reads;
    DevBuf<uint8_t> d_packed, d_exc_byte;   // 2-bit packed input (nw_align_ops_packed) and its exceptions
    DevBuf<int64_t> d_exc_pos;
    DevBuf<int64_t> d_offsets;
    // packed calls: the chunks' length segments (nw::LenSeg), pinned on the host and in HBM
    DevBuf<uint8_t> d_lens;
    uint8_t* h_lens = nullptr;
    int64_t h_lens_cap = 0;
    DevBuf<uint8_t> d_out;
    DevBuf<nw::Stat> d_stats;
    AmpConfig ac{};                   // the current amplicon's configuration (configure)
    hipEvent_t ev_wf0 = nullptr, ev_wf1 = nullptr;   // wide first: the fork after the sort, the join before the exact kernel
    int64_t call_wide_first = 0;       // reads of the last call the wide-first launches took
    CallState call{};                 // the running ops_call's
    ChunkLaunch last_launch{};        // the newest launch's report
    DevBuf<uint32_t> d_btab;
    DevBuf<uint32_t> d_sub16;         // exact multi-wave kernel's score rows
    bool lane_walk = false;           // resident passes: the first level's lane walk + stop summary (nw_batch_set_lane_walk)
    // resident passes: the phase events between the kernels (nw_batch_set_phase_events; each timing event
    // recorded between two kernels held the stream ~5-7 us: it writes back the L2's dirty lines)
    bool phase_events = true, phases_recorded = false;
    hipEvent_t ev_h1 = nullptr;       // ops_call: after the last upload (the upload span; ev_in[] do not time)
    unsigned epoch = 0;               // look-back launches so far (each launch uses a new value)
    int tail_prio = 1;                // KernelArgs::tail_prio
    bool ran = false;
    // ops output (nw_align_ops / nw_batch_set_output(NW_OUT_OPS)): per-read run slots,
    // spill area, compaction scratch; the pipelined call's copy streams and events
    int out_mode = NW_OUT_ROWS;
    int64_t reads_bias = 0;            // kernels index reads with the caller's offsets minus this
    DevBuf<int64_t> d_ctl64, d_opsoff;
    int64_t spill_cap = 0, staging_cap = 0;
    int ops_slot = nw::kOpsSlot;       // runs per read slot (CRISPR_NW_OPS_SLOT: tests force spills)
    int64_t ops_stride = 1;            // reads per slot row (the chunk capacity: ops_reserve)
    hipStream_t s_in = nullptr, s_out = nullptr;
    std::vector<hipEvent_t> ev_in, ev_cs, ev_ce, ev_out, ev_bulk;
    std::vector<hipEvent_t> ev_up;    // a dual call's exact-kernel path: after chunk k's unpack (its twin waits for it)
    hipEvent_t ev_h0 = nullptr;
    hipEvent_t ev_start = nullptr;     // the second compute stream starts after the first's set-up
    int64_t* h_ctl = nullptr;          // pinned: per chunk ctl[0, kOpsCtl) copied back
    int64_t h_ctl_chunks = 0;
    float ops_h2d_ms = 0.0f, ops_compute_ms = 0.0f;
    bool call_done = false;            // the last operation was nw_align_ops: the getters report its counts
    bool resident_ok = false;          // d_reads / d_offsets hold the last nw_align_ops batch
    // ... or d_packed / d_exc_* / d_offsets (a packed call: classify decodes the reads again)
    bool resident_packed = false;
    int64_t resident_n_exc = 0;
    // nw_batch_upload_packed: the batch is the 2-bit stream (classify decodes it, writing only
    // the DP reads' bytes); the bytes of every read exist once bytes_full (nw_batch_device_ops)
    bool bytes_full = true;
    nw::KernelArgs batch_pk{};         // its packed-input fields (pk_*) for the runs' classify
    int64_t batch_pos0 = 0, batch_base0 = 0, batch_nbytes = 0, batch_n_exc = 0;
    int64_t resident_n = 0, resident_lo = 0, resident_hi = 0;
    int64_t call_counts[4] = {0, 0, 0, 0};
    int64_t call_exact = 0;            // reads of the last call that reached the exact kernel
    int64_t ops_h2d_bytes = 0, ops_d2h_bytes = 0;
    // known copies: a resident pass against a new amplicon takes the reads equal to
    // the amplicon the batch was last aligned against (resident_ref: the HDR pass's copies of the
    // reference amplicon) from ONE alignment of that sequence, computed by the exact kernel on the
    // upload stream while the chunks start (d_k*: its bytes, offsets, 2-bit words, record, runs,
    // scratch); KernelArgs::known2 / nw::OpsKnown
    std::string resident_ref;
    std::string known_seq;     // nw_set_known: a sequence whose copies take one alignment in every call
    KnownSet kset[2];
    // Switches::trace: the launches' events, printed (us from the first upload) at the end of the call
    std::vector<std::pair<std::string, hipEvent_t>> trace_ev;
};

namespace {

// diagnostics: an event after the launch just queued on cs (Switches::trace)
void tmark(nw_ctx* c, const ChunkPlan& p, hipStream_t cs, const char* what) {
    if (!p.trace) return;
    if (c->call.trace_used == c->trace_ev.size()) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return;
        c->trace_ev.push_back({std::string(), e});
    }
    auto& slot = c->trace_ev[c->call.trace_used++];
    slot.first = std::to_string(p.chunk) + " " + what;
    (void)hipEventRecord(slot.second, cs);
}

// a look-back launch's epoch: new per launch, never 0 (30 bits, nw_common.h lookback_excl)
unsigned next_epoch(nw_ctx* c) {
    c->epoch = (c->epoch + 1) & 0x3fffffffu;
    if (c->epoch == 0) c->epoch = 1;
    return c->epoch;
}

// One amplicon's score tables (host side): the int8 profile of the exact kernel and
// the markup bits of the band walk (codes each row scores > 0 against).
struct AmpTables {
    int R = 0;
    std::vector<int8_t> prof;
    std::vector<uint32_t> rowpos;
    std::vector<uint32_t> amp2, seed_key;   // window seeds (Profile::amp2 / seed_key / seed_pos)
    std::vector<uint16_t> seed_pos;
    std::vector<uint32_t> cls;              // classify's LDS image (cls_image)
    int32_t sub12_words = 0;                // its self-mismatch prefix counts (its last words; 0: none)
    bool amp_acgt = false;
};

// classify's LDS image of the amplicon, in the kernel's LDS order: [nd] dwords of the folded
// amplicon (lower-case A C G T, 0 at any other byte and past La), [nd] of its raw bytes (0
// past La), then, with window seeds, amp2, the seed keys and the seed positions (uint16, two
// per word) -- one coalesced copy per block instead of per-byte folding and three table loads.
// Last, for an A C G T amplicon of at most 256 bp, the prefix counts of its self-mismatch at
// shifts 1, 2, 3 (sub12_words = La + 1 words): with A_sh[q] = amp[q] != amp[q + sh] for q < La - sh
// (0 from there on), word q holds C_sh[q] = sum of A_sh[i], i < q, in byte sh - 1; word La the
// totals.  Classify's one- and two-substitution certificates read their shifted diagonals' facts
// from them.
void cls_image(const std::string& ref, AmpTables* t) {
    const int La = (int)ref.size(), nd = (La + 3) / 4;
    t->cls.assign((size_t)(2 * nd), 0u);
    t->amp_acgt = La > 0;
    for (int q = 0; q < La; ++q) {
        const unsigned char c = (unsigned char)ref[(size_t)q], u = c & 0xDF;
        const bool acgt = u == 'A' || u == 'C' || u == 'G' || u == 'T';
        t->amp_acgt = t->amp_acgt && acgt;
        t->cls[(size_t)(q / 4)] |= (uint32_t)(acgt ? (u | 0x20) : 0) << (8 * (q % 4));
        t->cls[(size_t)(nd + q / 4)] |= (uint32_t)c << (8 * (q % 4));
    }
    t->sub12_words = 0;
    if (t->amp2.empty()) return;
    t->cls.insert(t->cls.end(), t->amp2.begin(), t->amp2.end());
    t->cls.insert(t->cls.end(), t->seed_key.begin(), t->seed_key.end());
    for (size_t i = 0; i < t->seed_pos.size(); i += 2)
        t->cls.push_back((uint32_t)t->seed_pos[i] | (i + 1 < t->seed_pos.size() ? (uint32_t)t->seed_pos[i + 1] << 16 : 0u));
    // the self-mismatch prefix counts (the lane path's amplicons: A C G T, La <= 256)
    if (!t->amp_acgt || La > 256) return;
    uint32_t c[3] = {0u, 0u, 0u};
    for (int q = 0; q <= La; ++q) {
        t->cls.push_back(c[0] | c[1] << 8 | c[2] << 16);
        for (int sh = 1; sh <= 3; ++sh)
            if (q + sh < La) c[sh - 1] += (ref[(size_t)q] & 0xDF) != (ref[(size_t)(q + sh)] & 0xDF);
    }
    t->sub12_words = La + 1;
}

// The amplicon's 2-bit stream (A C T G = 0 1 2 3 = (byte >> 1) & 3, base p in bits 2 (p % 16)
// of dword p / 16, as nw_pack_reads packs reads; two spare dwords) and its 16-mers of A C G T
// bases only, sorted by (key, position): classify's window seeds.
void seed_tables(const std::string& ref, AmpTables* t) {
    const int La = (int)ref.size();
    if (La < 16 || La > 1024) return;
    t->amp2.assign((size_t)(La + 15) / 16 + 2, 0u);
    std::vector<uint8_t> ok((size_t)La);
    for (int p = 0; p < La; ++p) {
        const unsigned char u = (unsigned char)ref[p] & 0xDF;
        ok[(size_t)p] = u == 'A' || u == 'C' || u == 'G' || u == 'T';
        t->amp2[(size_t)p / 16] |= (uint32_t)(((unsigned char)ref[p] >> 1) & 3u) << (2 * (p % 16));
    }
    std::vector<std::pair<uint32_t, uint16_t>> kp;
    for (int p = 0; p + 16 <= La; ++p) {
        bool all = true;
        uint32_t key = 0;
        for (int b = 0; b < 16; ++b) {
            all = all && ok[(size_t)(p + b)];
            key |= (uint32_t)(((unsigned char)ref[p + b] >> 1) & 3u) << (2 * b);
        }
        if (all) kp.emplace_back(key, (uint16_t)p);
    }
    std::sort(kp.begin(), kp.end());
    for (auto& e : kp) {
        t->seed_key.push_back(e.first);
        t->seed_pos.push_back(e.second);
    }
}

bool amp_tables(const std::string& ref, int scale, AmpTables* t) {
    const int La = (int)ref.size();
    if (La > kMaxRef) return false;
    // markup bits first: an amplicon longer than the one-wave kernels take (R = 0) has
    // only these (the multi-wave kernel aligns it)
    t->rowpos.resize((size_t)La);
    for (int ai = 0; ai < La; ++ai) {
        const uint8_t ca = nw::code_of((unsigned char)ref[ai]);
        uint32_t m = 0;
        for (int code = 0; code < nw::NCODE; ++code)
            if (ca < 16 && code < 16 && nw::kEdna[ca][code] > 0) m |= 1u << code;
        t->rowpos[(size_t)ai] = m;
    }
    const int R = La <= kMaxRefWave ? nw::rows_per_lane_for(La) : 0;
    t->R = R;
    seed_tables(ref, t);
    cls_image(ref, t);
    if (R <= 0) return true;
    const int RP = nw::profile_rp(R);
    t->prof.assign((size_t)nw::NCODE * 64 * RP, 0);
    for (int ai = 0; ai < La; ++ai) {
        const uint8_t ca = nw::code_of((unsigned char)ref[ai]);
        for (int code = 0; code < nw::NCODE; ++code) {
            int s = (ca < 16 && code < 16) ? nw::kEdna[ca][code] * scale : 0;
            t->prof[(size_t)code * 64 * RP + (ai / R) * RP + ai % R] = (int8_t)s;
        }
    }
    return true;
}

// The tables every amplicon shares (they depend on the penalties only): ascii ->
// A T G C N pad/unknown (0..5, 6 = other IUPAC: the band / pair-table alphabet),
// ascii -> EDNAFULL code, and the certified-band score table [amplicon code][read A
// code][read B code] over A T G C N pad, packed int16x2 + 2 * extend.
int upload_shared(nw_ctx* c) {
    const std::string key = std::to_string(c->scale) + "/" + std::to_string(c->gap_extend);
    if (key == c->shared_key && c->d_sub16.p) return NW_OK;
    c->shared_key.clear();
    const int codes6[6] = {0, 1, 2, 3, 14, nw::NCODE_PAD};
    std::vector<uint8_t> lut6(256), lut(256);
    for (int q = 0; q < 256; ++q) {
        const int code = nw::code_of((unsigned char)q);
        int r = 6;
        for (int i = 0; i < 6; ++i)
            if (codes6[i] == code) r = i;
        lut6[(size_t)q] = (uint8_t)r;
        lut[(size_t)q] = (uint8_t)code;
    }
    // amplicon rows by EDNAFULL code (IUPAC amplicons keep the band path), read codes by the
    // 6-code alphabet (reads with other IUPAC codes leave the band: REGION_BAD_*)
    auto sub6 = [&](int cx, int y) {
        const int cy = codes6[y];
        return (cx < 16 && cy < 16) ? nw::kEdna[cx][cy] * c->scale : 0;
    };
    std::vector<uint32_t> btab((size_t)nw::NCODE * 36);
    for (int x = 0; x < nw::NCODE; ++x)
        for (int ya = 0; ya < 6; ++ya)
            for (int yb = 0; yb < 6; ++yb) {
                const uint16_t sa = (uint16_t)(int16_t)(sub6(x, ya) + 2 * c->gap_extend);
                const uint16_t sb = (uint16_t)(int16_t)(sub6(x, yb) + 2 * c->gap_extend);
                btab[(size_t)x * 36 + ya * 6 + yb] = sa | ((uint32_t)sb << 16);
            }
    std::vector<uint32_t> sub16((size_t)nw::NCODE * 4, 0u);
    for (int ca = 0; ca < 16; ++ca)
        for (int code = 0; code < 16; ++code)
            sub16[(size_t)ca * 4 + code / 4] |= (uint32_t)(uint8_t)(int8_t)(nw::kEdna[ca][code] * c->scale)
                                                << (8 * (code % 4));
    HIP_TRY(c, c->d_sub16.reserve(sub16.size()));
    HIP_TRY(c, hipMemcpy(c->d_sub16.p, sub16.data(), sub16.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, c->d_lut6.reserve(256));
    HIP_TRY(c, c->d_lut.reserve(256));
    HIP_TRY(c, c->d_btab.reserve(btab.size()));
    HIP_TRY(c, hipMemcpy(c->d_lut6.p, lut6.data(), 256, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_lut.p, lut.data(), 256, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_btab.p, btab.data(), btab.size() * 4, hipMemcpyHostToDevice));
    c->shared_key = key;
    return NW_OK;
}

// Every amplicon's tables in one device arena (one upload): profs[g] points into it.
int upload_profiles(nw_ctx* c, const std::vector<std::string>& refs, std::vector<Profile>* profs) {
    // the tables depend on the amplicons and the score scale
    const std::string key = std::to_string(c->scale);
    if (key == c->arena_key && refs == c->arena_refs && c->d_arena.p) {
        *profs = c->arena_profs;
        return NW_OK;
    }
    c->arena_key.clear();
    std::vector<AmpTables> tabs(refs.size());
    size_t total = 0;
    auto sec = [&](size_t bytes) {
        const size_t at = total;
        total += (bytes + 255) & ~(size_t)255;
        return at;
    };
    struct Off { size_t prof, rowpos, amp, amp2, skey, spos, cls; };
    std::vector<Off> offs(refs.size());
    for (size_t g = 0; g < refs.size(); ++g) {
        if (!amp_tables(refs[g], c->scale, &tabs[g]))
            return fail(c, NW_E_UNSUPPORTED, "amplicon length %d exceeds %d", (int)refs[g].size(), kMaxRef);
        const AmpTables& t = tabs[g];
        const size_t o1 = sec(t.prof.size()), o5 = sec(t.rowpos.size() * 4), o6 = sec(refs[g].size() + 16);
        const size_t o7 = sec(t.amp2.size() * 4), o8 = sec(t.seed_key.size() * 4), o9 = sec(t.seed_pos.size() * 2);
        const size_t o10 = sec(t.cls.size() * 4);
        offs[g] = {o1, o5, o6, o7, o8, o9, o10};
    }
    std::vector<uint8_t> host(std::max<size_t>(total, 256), 0);
    for (size_t g = 0; g < refs.size(); ++g) {
        const AmpTables& t = tabs[g];
        const Off& o = offs[g];
        std::memcpy(host.data() + o.prof, t.prof.data(), t.prof.size());
        std::memcpy(host.data() + o.rowpos, t.rowpos.data(), t.rowpos.size() * 4);
        std::memcpy(host.data() + o.amp, refs[g].data(), refs[g].size());
        std::memcpy(host.data() + o.amp2, t.amp2.data(), t.amp2.size() * 4);
        std::memcpy(host.data() + o.skey, t.seed_key.data(), t.seed_key.size() * 4);
        std::memcpy(host.data() + o.spos, t.seed_pos.data(), t.seed_pos.size() * 2);
        std::memcpy(host.data() + o.cls, t.cls.data(), t.cls.size() * 4);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // no kernel may still read the old arena
    HIP_TRY(c, c->d_arena.reserve(host.size()));
    HIP_TRY(c, hipMemcpy(c->d_arena.p, host.data(), host.size(), hipMemcpyHostToDevice));
    profs->resize(refs.size());
    for (size_t g = 0; g < refs.size(); ++g) {
        const Off& o = offs[g];
        uint8_t* b = c->d_arena.p;
        Profile& p = (*profs)[g];
        p.prof = (const int8_t*)(b + o.prof);
        p.rowpos = (const uint32_t*)(b + o.rowpos);
        p.amp = b + o.amp;
        p.R = tabs[g].R;
        p.cls_img = (const uint32_t*)(b + o.cls);
        p.cls_words = (int32_t)tabs[g].cls.size();
        p.sub12_words = tabs[g].sub12_words;
        p.amp_acgt = tabs[g].amp_acgt;
        if (!tabs[g].amp2.empty()) {
            p.amp2 = (const uint32_t*)(b + o.amp2);
            p.seed_key = (const uint32_t*)(b + o.skey);
            p.seed_pos = (const uint16_t*)(b + o.spos);
            p.n_seed = (int32_t)tabs[g].seed_key.size();
        }
    }
    c->arena_refs = refs;
    c->arena_profs = *profs;
    c->arena_key = key;
    return NW_OK;
}

int build_profile(nw_ctx* c) {
    int rc = upload_shared(c);
    if (rc) return rc;
    std::vector<Profile> one;
    if ((rc = upload_profiles(c, {c->ref}, &one))) return rc;
    c->cur = one[0];
    return NW_OK;
}

int ops_reserve(nw_ctx* c, const Switches& sw, Scratch& S, int64_t chunk, int64_t n);

int64_t stride_for(int La, int32_t lb_max) { return ((int64_t)La + lb_max + 15) & ~(int64_t)15; }

// the exact multi-wave kernel's LDS, its traceback there if it fits, else in slabs of HBM
void exact_sizes(int La, int32_t lb_max, AmpConfig& ac) {
    ac.exact_lds = nw::exact_lds_bytes(La, lb_max, true);
    if (ac.exact_lds <= kMaxLds) return;
    ac.exact_tb_lds = false;
    ac.exact_lds = nw::exact_lds_bytes(La, lb_max, false);
    ac.exact_slab = (nw::exact_slab_bytes(La, lb_max) + 255) & ~(int64_t)255;
}

// Amplicons longer than the one-wave kernels take (kMaxRefWave < La <= kMaxRef):
// every read through the exact multi-wave kernel (nw_exact.hip), one workgroup per
// read, as many workgroups as the CUs hold.
int configure_long(nw_ctx* c, Scratch& S, int64_t n, AmpConfig& ac) {
    const int La = (int)c->ref.size();
    exact_sizes(La, c->lb_max, ac);
    const int W = nw::exact_waves(La);
    int per_cu = std::max(1, 32 / W);   // 32 wavefronts per CU
    if (ac.exact_lds <= 0 || ac.exact_lds > kMaxLds)
        return fail(c, NW_E_UNSUPPORTED, "reads of %d bases do not fit the kernel for a %d bp amplicon", c->lb_max, La);
    per_cu = std::max(1, std::min(per_cu, kMaxLds / ac.exact_lds));
    int64_t grid = std::max<int64_t>(1, std::min<int64_t>((int64_t)c->num_cus * per_cu, std::max<int64_t>(n, 1)));
    if (!ac.exact_tb_lds) {
        grid = std::max<int64_t>(1, std::min<int64_t>(grid, (2ll << 30) / ac.exact_slab));
        HIP_TRY(c, S.d_tb.reserve((size_t)(ac.exact_slab * grid)));
    }
    ac.exact_grid = (int)grid;
    ac.exact_full = true;
    HIP_TRY(c, S.d_fallback.reserve((size_t)std::max<int64_t>(n, 1)));
    HIP_TRY(c, S.d_fallback_count.reserve(nw::kChunkCounters));
    return NW_OK;
}

// ... and the amplicons they take: the band path where its certificate holds, else the exact kernel.
int configure_wave(nw_ctx* c, const Switches& sw, Scratch& S, int64_t n, AmpConfig& ac) {
    const int La = (int)c->ref.size();
    const int R = c->cur.R;
    // full-storage kernel: every alignment (band disabled) or only the fallbacks
    nw::LaunchCfg cfg{};
    cfg.R = R;
    cfg.tb_mode = nw::TB_GLOBAL_FULL;
    cfg.wpb = 4;
    for (int wpb : {4, 2, 1}) {
        int b = nw::lds_bytes_for(R, La, c->lb_max, nw::TB_LDS_FULL, wpb);
        if (b > 0 && b <= kMaxLds) {
            cfg.tb_mode = nw::TB_LDS_FULL;
            cfg.wpb = wpb;
            cfg.lds_bytes = b;
            break;
        }
    }
    // Traceback in HBM instead of LDS when the LDS traceback leaves a SIMD without a second
    // wavefront (a read's whole matrix at 4 bits per cell: 151 x 280 C1-shape reads take 41 KB per
    // wavefront, three per CU): a lone wavefront issues a VALU instruction per ~4 cycles and
    // waits out its own latencies.  CRISPR_NW_EXACT=lds keeps the LDS traceback (A/Bs).
    if (cfg.tb_mode == nw::TB_LDS_FULL && !sw.exact_lds &&
        cfg.wpb * std::min(8, kMaxLds / cfg.lds_bytes) < 8) {
        cfg.tb_mode = nw::TB_GLOBAL_FULL;
        cfg.wpb = 4;
    }
    if (cfg.tb_mode == nw::TB_GLOBAL_FULL) cfg.lds_bytes = nw::lds_bytes_for(R, La, c->lb_max, nw::TB_GLOBAL_FULL, cfg.wpb);
    if (cfg.lds_bytes <= 0 || cfg.lds_bytes > kMaxLds)
        return fail(c, NW_E_UNSUPPORTED, "reads of %d bases do not fit the kernel", c->lb_max);
    int per_cu = std::max(1, std::min(8, kMaxLds / cfg.lds_bytes));
    cfg.grid = c->num_cus * per_cu;
    if (cfg.tb_mode == nw::TB_GLOBAL_FULL) {
        const int64_t per_wave = nw::tb_bytes_per_wave(R, c->lb_max);
        HIP_TRY(c, S.d_tb.reserve((size_t)per_wave * cfg.grid * cfg.wpb));
    }
    ac.cfg = cfg;
    // exact multi-wave kernel for the work lists (the reads no band certifies)
    // Off by default: at the ~15 reads per 1M C2 reads it is not faster than the one-wave
    // kernel (both are VALU-issue bound), so it serves the long amplicons
    if (nw::exact_rows_per_lane(La) > 0 && sw.exact_multi) {   // fallbacks through it (tests)
        exact_sizes(La, c->lb_max, ac);
        int grid = c->num_cus;
        if (!ac.exact_tb_lds) {
            grid = (int)std::max<int64_t>(1, std::min<int64_t>(grid, (1ll << 30) / std::max<int64_t>(ac.exact_slab, 1)));
            HIP_TRY(c, S.d_tb.reserve((size_t)(ac.exact_slab * grid)));
        }
        if (sw.exact_multi_grid > 0) grid = std::min(grid, sw.exact_multi_grid);   // split the list between the kernels
        if (ac.exact_lds > 0 && ac.exact_lds <= kMaxLds) ac.exact_grid = grid;
    }
    // -endweight: the band certificate assumes free end gaps; every read goes through
    // the exact kernel (nw_align_kernel), which takes both
    if (c->end_weight) {
        HIP_TRY(c, S.d_fallback.reserve((size_t)std::max<int64_t>(n, 1)));
        HIP_TRY(c, S.d_fallback_count.reserve(nw::kChunkCounters));
        return NW_OK;
    }
    // certified diagonal band (default): scores and biases within int16, amplicon
    // within the band table's alphabet, non-negative gap costs (the certificate)
    const int64_t diag_hi = 5ll * c->scale * La + (int64_t)c->gap_extend * (2 * La + 300) + c->gap_open;
    if (sw.band && La <= 1024 && diag_hi < 15000 && c->gap_extend >= 0 &&
        c->gap_open >= c->gap_extend) {
        const int64_t pairs = (n + 2) / 2;   // (the second level's list may hold one hole)
        const int64_t cap_bytes = sw.region_bytes;
        ac.diag_lb_cap = La + nw::kBandDiags - 1;
        ac.diag_words = nw::band_region_words(La, c->lb_max);
        // one level: fill + walk launch configs, region stride and pairs per pass
        // (the wide level at 8, 2 or 4 wavefronts per fill block measured slower or no faster)
        const int wide_fill_wpb = 1, wide_walk_wpb = 2;
        int occ_fill = 0, occ_walk = 0;   // blocks per CU of the level configured last
        auto level = [&](int W, nw::LaunchCfg& f, nw::LaunchCfg& w, int64_t& stride, int64_t& pass_pairs,
                         int64_t max_pairs = INT64_MAX) -> int {
            f = nw::LaunchCfg{};
            w = nw::LaunchCfg{};
            f.R = w.R = R;
            f.tb_mode = w.tb_mode = nw::TB_DIAG;
            // the wide level aligns few reads, latency-bound: one wavefront per block (fill) and
            // two (walk) spread them over the CUs instead of stacking 8 on a CU's 4 SIMDs
            const bool wide = W > nw::kBandDiags;
            f.wpb = wide ? wide_fill_wpb : 8;
            w.wpb = wide ? wide_walk_wpb : 8;
            f.lds_bytes = nw::band_fill_lds_bytes(La, f.wpb, W);
            w.lds_bytes = nw::band_walk_lds_bytes(La, w.wpb, c->lb_max, W);
            int fb = 0, wb = 0;
            if (f.lds_bytes > kMaxLds || w.lds_bytes > kMaxLds) return 0;
            if (nw::band_occupancy(W, f.wpb, w.wpb, f.lds_bytes, w.lds_bytes, &fb, &wb) != hipSuccess || fb <= 0 ||
                wb <= 0)
                return 0;
            occ_fill = fb;
            occ_walk = wb;
            const int ppw = W == 16 ? 8 : (W == 32 ? 4 : 1);   // read pairs per wavefront
            stride = nw::band_region_bytes(La, c->lb_max, W);
            pass_pairs = std::max<int64_t>(ppw, std::min<int64_t>(std::min(pairs, max_pairs), cap_bytes / stride));
            pass_pairs = (pass_pairs + ppw - 1) / ppw * ppw;
            const int64_t pp = std::min<int64_t>(std::max<int64_t>(pairs, 1), pass_pairs);
            f.grid = (int)std::max<int64_t>(1, std::min<int64_t>(((pp + ppw - 1) / ppw + f.wpb - 1) / f.wpb,
                                                                 (int64_t)c->num_cus * fb));
            w.grid = (int)std::max<int64_t>(1, std::min<int64_t>((2 * pp + w.wpb - 1) / w.wpb, (int64_t)c->num_cus * wb));
            return 1;
        };
        const bool use16 = !sw.diag32 &&
                           level(16, ac.diag16_fill, ac.diag16_walk, ac.diag16_stride, ac.diag16_pass_pairs);
        if (!use16) ac.diag16_fill.grid = 0;
        if (level(32, ac.diag_fill, ac.diag_walk, ac.diag_stride, ac.diag_pass_pairs)) {
            int64_t rbytes = std::max(std::min<int64_t>(std::max<int64_t>(pairs, 1), ac.diag_pass_pairs) * ac.diag_stride,
                                      use16 ? std::min<int64_t>(std::max<int64_t>(pairs, 1), ac.diag16_pass_pairs) *
                                                  ac.diag16_stride : 0);
            // the wide level: at most kWidePairs read pairs per chunk in the region (the rest of
            // its list goes to the exact kernel); Switches::wide: off
            if (sw.wide &&
                level(nw::kWideDiags, ac.wide_fill, ac.wide_walk, ac.wide_stride, ac.wide_pairs,
                      kWidePairs + c->call.seed_pairs)) {
                ac.wide_words = nw::band_region_words(La, c->lb_max, nw::kWideDiags);
                ac.wide_lb_cap = La + nw::kWideDiags - 1;
                rbytes = std::max(rbytes, ac.wide_pairs * ac.wide_stride);
                HIP_TRY(c, S.d_fallback2.reserve((size_t)std::max<int64_t>(n, 1)));
            } else {
                ac.wide_fill.grid = 0;
            }
            // wide first: the same kernels on a region of their own, at most wf_cap reads of the chunk
            if (use16 && ac.wide_fill.grid > 0 && sw.wide_first) {
                const int64_t cap = sw.wide_first_cap;
                if (cap > 0) {   // the wide level's launch shape (its occupancy: no second query), grids for this list
                    ac.wf_pairs = std::max<int64_t>(1, std::min(std::min(pairs, (cap + 1) / 2), cap_bytes / ac.wide_stride));
                    ac.wf_cap = (int)std::min<int64_t>(cap, 2 * ac.wf_pairs);
                    ac.wf_fill = ac.wide_fill;
                    ac.wf_walk = ac.wide_walk;
                    ac.wf_fill.grid = (int)std::max<int64_t>(1, std::min<int64_t>((ac.wf_pairs + wide_fill_wpb - 1) / wide_fill_wpb,
                                                                                 (int64_t)c->num_cus * occ_fill));
                    ac.wf_walk.grid = (int)std::max<int64_t>(1, std::min<int64_t>((2 * ac.wf_pairs + wide_walk_wpb - 1) / wide_walk_wpb,
                                                                                 (int64_t)c->num_cus * occ_walk));
                    HIP_TRY(c, S.d_wf_region.reserve((size_t)(ac.wf_pairs * ac.wide_stride)));
                    HIP_TRY(c, S.d_wf_list.reserve((size_t)std::max<int64_t>(n, 1)));
                }
            }
            HIP_TRY(c, S.d_bregion.reserve((size_t)rbytes));
            HIP_TRY(c, S.d_order.reserve((size_t)std::max<int64_t>(n, 1)));
            HIP_TRY(c, S.d_redo.reserve((size_t)std::max<int64_t>(n, 1)));
            HIP_TRY(c, S.d_redo_flags.reserve((size_t)std::max<int64_t>(n, 1)));
            HIP_TRY(c, S.d_lb.reserve((size_t)nw::band_lookback_words(n)));
            HIP_TRY(c, S.d_sort_key.reserve((size_t)std::max<int64_t>(n, 1)));
            // 64 entries per classify wavefront: 4 per block of 256 reads, ceil(n / 256) + 1 blocks
            HIP_TRY(c, S.d_cert_q.reserve((size_t)std::max<int64_t>(n, 1) + 1024));
            HIP_TRY(c, S.d_cert_cnt.reserve((size_t)std::max<int64_t>(n, 1) / 64 + 16));
            if (c->call.seed_on) {
                HIP_TRY(c, S.d_seed.reserve((size_t)std::max<int64_t>(n, 1)));
                HIP_TRY(c, S.d_seed2.reserve((size_t)std::max<int64_t>(n, 1)));
                // the segment sort pads each 4096-read segment's seeded list to an even length (one
                // entry per segment at most): the list, its flags and its compaction hold n + n/4096 + 2
                const size_t nseed = (size_t)(n + n / 4096 + 2);
                HIP_TRY(c, S.d_seed_list.reserve(nseed));
                HIP_TRY(c, S.d_seed_flags.reserve(nseed));
                HIP_TRY(c, S.d_seed_list2.reserve(nseed));
            }
            ac.use_diag = true;
        }
    }
    HIP_TRY(c, S.d_fallback.reserve((size_t)std::max<int64_t>(n, 1)));
    HIP_TRY(c, S.d_fallback_count.reserve(nw::kChunkCounters));
    return NW_OK;
}

// The current amplicon's (c->ref, c->cur) configuration for launches of up to n reads of at most c->lb_max
// bases on scratch set S, whose buffers it sizes: built afresh (no route keeps another amplicon's fields).
int configure(nw_ctx* c, const Switches& sw, Scratch& S, int64_t n) {
    AmpConfig ac{};
    ac.stride = stride_for((int)c->ref.size(), c->lb_max);
    const int rc = c->cur.R <= 0 ? configure_long(c, S, n, ac) : configure_wave(c, sw, S, n, ac);
    if (!rc) c->ac = ac;
    return rc;
}

}  // namespace

extern "C" {

int nw_create(int device, nw_ctx** out) {
    if (!out) return NW_E_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return NW_E_HIP;
    if (device < 0 || device >= count) return NW_E_INVALID;
    nw_ctx* c = new nw_ctx();
    c->device = device;
    // Creation order decides which streams share a hardware queue (a process gets
    // GPU_MAX_HW_QUEUES = 4; the fifth stream shares the first one's queue, and a queue runs
    // its packets in order, so a cross-stream wait queued there holds back the other
    // stream too).  Default: s_in first and the third compute stream (the pipelined call's
    // tail stream) last, so those two share: the uploads of a call are all queued before its
    // first tail packet.  (Round 2's order, where s_out shared the first compute stream's
    // queue: 2.475 vs 2.423 ms per 1M-read call.)
    hipStream_t* order[5] = {&c->s_in, &c->stream, &c->cstream[1], &c->s_out, &c->cstream[2]};
    bool streams_ok = hipSetDevice(device) == hipSuccess;
    for (hipStream_t* sp : order)
        streams_ok = streams_ok && hipStreamCreateWithFlags(sp, hipStreamNonBlocking) == hipSuccess;
    if (!streams_ok || hipEventCreate(&c->ev_h0) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_start, hipEventDisableTiming) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreate(&c->ev_fill) != hipSuccess || hipEventCreate(&c->ev_walk) != hipSuccess ||
        hipEventCreate(&c->ev_sort) != hipSuccess || hipEventCreate(&c->ev_l2) != hipSuccess ||
        hipEventCreate(&c->ev_h1) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_wf0, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_wf1, hipEventDisableTiming) != hipSuccess) {
        delete c;
        return NW_E_HIP;
    }
    c->cstream[0] = c->stream;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        c->num_cus = prop.multiProcessorCount;
    *out = c;
    return NW_OK;
}

void nw_destroy(nw_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->s_in) (void)hipStreamSynchronize(c->s_in);
    for (auto& t : c->trace_ev) (void)hipEventDestroy(t.second);
    for (hipEvent_t e : c->ev_bulk) (void)hipEventDestroy(e);
    for (int k = 1; k < kComputeStreams; ++k)
        if (c->cstream[k]) (void)hipStreamSynchronize(c->cstream[k]);
    if (c->s_out) (void)hipStreamSynchronize(c->s_out);
    for (auto* v : {&c->ev_in, &c->ev_cs, &c->ev_ce, &c->ev_out, &c->ev_up})
        for (hipEvent_t e : *v) (void)hipEventDestroy(e);
    if (c->h_ctl) (void)hipHostFree(c->h_ctl);
    if (c->h_lens) (void)hipHostFree(c->h_lens);
    if (c->s_in) (void)hipStreamDestroy(c->s_in);
    for (int k = 1; k < kComputeStreams; ++k)
        if (c->cstream[k]) (void)hipStreamDestroy(c->cstream[k]);
    if (c->s_out) (void)hipStreamDestroy(c->s_out);
    for (hipEvent_t e : {c->ev_h0, c->ev_start, c->ev_fill, c->ev_wf0, c->ev_wf1, c->ev_h1, c->ev_sort, c->ev_l2,
                         c->ev_walk, c->ev0, c->ev1})
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* nw_last_error(const nw_ctx* c) { return c ? c->err.c_str() : "null context"; }

int nw_set_params(nw_ctx* c, float gap_open, float gap_extend, int end_weight, float end_open,
                  float end_extend, const char* matrix, int tie_policy) {
    if (!c) return NW_E_INVALID;
    if (matrix && *matrix) {
        std::string m(matrix);
        for (auto& ch : m) ch = (char)std::toupper((unsigned char)ch);
        if (m != "EDNAFULL") return fail(c, NW_E_UNSUPPORTED, "matrix %s not supported (EDNAFULL only)", matrix);
    }
    if (tie_policy != NW_TIE_EMBOSS) return fail(c, NW_E_UNSUPPORTED, "tie policy %d not supported", tie_policy);
    if (!(gap_open >= 0.0f) || !(gap_extend >= 0.0f) || gap_open > 1000.0f || gap_extend > 1000.0f)
        return fail(c, NW_E_INVALID, "gap penalties out of range: %g %g", gap_open, gap_extend);
    if (end_weight && (!(end_open >= 0.0f) || !(end_extend >= 0.0f) || end_open > 1000.0f || end_extend > 1000.0f))
        return fail(c, NW_E_INVALID, "end gap penalties out of range: %g %g", end_open, end_extend);
    int scale = 0;
    for (int s = 1; s <= 16; s *= 2) {
        double o = (double)gap_open * s, e = (double)gap_extend * s;
        double eo = end_weight ? (double)end_open * s : 0.0, ee = end_weight ? (double)end_extend * s : 0.0;
        if (o == std::floor(o) && e == std::floor(e) && eo == std::floor(eo) && ee == std::floor(ee)) {
            scale = s;
            break;
        }
    }
    if (!scale) return fail(c, NW_E_INEXACT, "gap penalties %g/%g (end %g/%g) are not multiples of 1/16", gap_open,
                            gap_extend, end_open, end_extend);
    c->scale = scale;
    c->gap_open = (int)std::lround((double)gap_open * scale);
    c->gap_extend = (int)std::lround((double)gap_extend * scale);
    c->end_weight = end_weight != 0;
    c->end_open = end_weight ? (int)std::lround((double)end_open * scale) : 0;
    c->end_extend = end_weight ? (int)std::lround((double)end_extend * scale) : 0;
    if (!c->ref.empty()) {
        (void)hipSetDevice(c->device);
        return build_profile(c);
    }
    return NW_OK;
}

int nw_score_scale(const nw_ctx* c) { return c ? c->scale : 0; }

int nw_set_reference(nw_ctx* c, const char* ref, int32_t ref_len) {
    if (!c || !ref || ref_len <= 0) return fail(c, NW_E_INVALID, "empty amplicon");
    if (ref_len > kMaxRef) return fail(c, NW_E_UNSUPPORTED, "amplicon length %d exceeds %d", ref_len, kMaxRef);
    (void)hipSetDevice(c->device);
    c->ref.assign(ref, ref + ref_len);
    c->ran = false;
    c->call_done = false;
    return build_profile(c);
}

int64_t nw_required_stride(const nw_ctx* c, int32_t max_read_len) {
    if (!c || c->ref.empty()) return 0;
    return stride_for((int)c->ref.size(), std::max(max_read_len, 1));
}

int nw_batch_upload(nw_ctx* c, const char* reads, const int64_t* offsets, int64_t n) {
    if (!c) return NW_E_INVALID;
    if (c->ref.empty()) return fail(c, NW_E_STATE, "nw_set_reference must come first");
    if (n < 0 || (n > 0 && (!offsets || !reads))) return fail(c, NW_E_INVALID, "bad batch");
    (void)hipSetDevice(c->device);
    const int La = (int)c->ref.size();
    int32_t lb_max = 1;
    int64_t cells = 0;
    c->read_lens.resize((size_t)n);
    for (int64_t r = 0; r < n; ++r) {
        const int64_t len = offsets[r + 1] - offsets[r];
        if (len < 0 || len > (1 << 20)) return fail(c, NW_E_INVALID, "read %lld has length %lld", (long long)r, (long long)len);
        c->read_lens[(size_t)r] = (int32_t)len;
        lb_max = std::max<int32_t>(lb_max, (int32_t)len);
        cells += (int64_t)La * len;
    }
    const int64_t base = n ? offsets[0] : 0;
    const int64_t nbytes = n ? offsets[n] - base : 0;
    std::vector<int64_t> rel((size_t)n + 1);
    for (int64_t r = 0; r <= n; ++r) rel[(size_t)r] = n ? offsets[r] - base : 0;
    c->n = n;
    c->lb_max = lb_max;
    c->cells = cells;
    HIP_TRY(c, c->d_reads.reserve((size_t)nbytes + 512));   // the walk DMAs whole 256-B chunks
    HIP_TRY(c, c->d_offsets.reserve((size_t)n + 1));
    if (c->out_mode == NW_OUT_ROWS)
        HIP_TRY(c, c->d_out.reserve((size_t)std::max<int64_t>(n, 1) * 3 * stride_for(La, lb_max)));
    HIP_TRY(c, c->d_stats.reserve((size_t)std::max<int64_t>(n, 1)));
    c->resident_ok = false;
    c->bytes_full = true;
    c->batch_pk = nw::KernelArgs{};
    if (nbytes) HIP_TRY(c, hipMemcpyAsync(c->d_reads.p, reads + base, (size_t)nbytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_offsets.p, rel.data(), sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->reads_bias = 0;
    const Switches sw = read_switches();
    int rc = configure(c, sw, c->sc[0], n);
    if (rc) return rc;
    if (c->out_mode == NW_OUT_OPS && (rc = ops_reserve(c, sw, c->sc[0], n, n))) return rc;
    c->ran = false;
    c->call_done = false;
    return NW_OK;
}

int nw_batch_upload_packed(nw_ctx* c, const uint8_t* packed, const int64_t* offsets, const uint16_t* lens, int64_t n,
                           const int64_t* exc_pos, const uint8_t* exc_byte, int64_t n_exc) {
    const nw_front::PackedSrc src{packed, lens, nullptr, exc_pos, exc_byte, false, nullptr};
    return nw_front::set_packed_batch(c, src, offsets, lens, n, n_exc);
}

}  // extern "C"

// nw_batch_upload_packed, and nw_front::adopt_packed with the batch already in HBM (src.on_device:
// the copies are device-to-device, ordered after src.ready on the context's stream).
int nw_front::set_packed_batch(nw_ctx* c, const PackedSrc& src, const int64_t* offsets, const uint16_t* lens, int64_t n,
                               int64_t n_exc) {
    const uint8_t* packed = src.packed;
    const int64_t* exc_pos = src.exc_pos;
    const uint8_t* exc_byte = src.exc_byte;
    const hipMemcpyKind kind = src.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (!c) return NW_E_INVALID;
    if (c->ref.empty()) return fail(c, NW_E_STATE, "nw_set_reference must come first");
    if (c->out_mode != NW_OUT_OPS) return fail(c, NW_E_STATE, "a packed batch needs nw_batch_set_output(NW_OUT_OPS)");
    if (n <= 0 || !offsets || !packed || !lens || !src.lens || (n_exc > 0 && (!exc_pos || !exc_byte)) || n_exc < 0)
        return fail(c, NW_E_INVALID, "bad batch");
    (void)hipSetDevice(c->device);
    const int La = (int)c->ref.size();
    int32_t lb_max = 1;
    int64_t cells = 0;
    c->read_lens.resize((size_t)n);
    for (int64_t r = 0; r < n; ++r) {
        const int64_t len = offsets[r + 1] - offsets[r];
        if (len < 0 || len > 65535 || len != lens[r])
            return fail(c, NW_E_INVALID, "read %lld: length %lld, lens %u", (long long)r, (long long)len, (unsigned)lens[r]);
        c->read_lens[(size_t)r] = (int32_t)len;
        lb_max = std::max<int32_t>(lb_max, (int32_t)len);
        cells += (int64_t)La * len;
    }
    const int64_t base0 = offsets[0], nbytes = offsets[n] - base0;
    const int64_t P0 = (base0 / 16) * 4, pk_hi = (offsets[n] + 3) / 4, q0 = base0 / 4;
    const int64_t ngroups = n / nw::kLenGroup + 1;
    c->n = n;
    c->lb_max = lb_max;
    c->cells = cells;
    HIP_TRY(c, c->d_reads.reserve((size_t)nbytes + 512 + 16));
    HIP_TRY(c, c->d_offsets.reserve((size_t)n + 1));
    HIP_TRY(c, c->d_stats.reserve((size_t)n));
    HIP_TRY(c, c->d_packed.reserve((size_t)(pk_hi - P0) + 64));
    HIP_TRY(c, c->d_exc_pos.reserve((size_t)std::max<int64_t>(n_exc, 1)));
    HIP_TRY(c, c->d_exc_byte.reserve((size_t)std::max<int64_t>(n_exc, 1)));
    HIP_TRY(c, c->d_lens.reserve((size_t)(8 * ngroups + 2 * n + 64)));
    std::vector<int64_t> gb((size_t)ngroups);
    for (int64_t g = 0; g < ngroups; ++g) gb[(size_t)g] = offsets[g * nw::kLenGroup];
    c->resident_ok = false;
    if (src.ready) HIP_TRY(c, hipStreamWaitEvent(c->stream, src.ready, 0));
    HIP_TRY(c, hipMemcpyAsync(c->d_packed.p + (q0 - P0), packed + q0, (size_t)(pk_hi - q0), kind, c->stream));
    if (n_exc) {
        HIP_TRY(c, hipMemcpyAsync(c->d_exc_pos.p, exc_pos, 8 * (size_t)n_exc, kind, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->d_exc_byte.p, exc_byte, (size_t)n_exc, kind, c->stream));
    }
    if (src.on_device)
        HIP_TRY(c, hipMemcpyAsync(c->d_lens.p, src.gbase, 8 * (size_t)ngroups, kind, c->stream));
    else
        HIP_TRY(c, hipMemcpyAsync(c->d_lens.p, gb.data(), 8 * (size_t)ngroups, kind, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_lens.p + 8 * ngroups, src.lens, 2 * (size_t)n, kind, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->reads_bias = base0 & ~(int64_t)15;
    const Switches sw = read_switches();
    int rc = configure(c, sw, c->sc[0], n);
    if (rc) return rc;
    if ((rc = ops_reserve(c, sw, c->sc[0], n, n))) return rc;
    c->batch_pos0 = 4 * P0;
    c->batch_base0 = base0;
    c->batch_nbytes = nbytes;
    c->batch_n_exc = n_exc;
    c->batch_pk = nw::KernelArgs{};
    nw::LenSeg ls{(const uint16_t*)(c->d_lens.p + 8 * ngroups), (const int64_t*)c->d_lens.p, 0, ngroups, 0, n,
                  c->d_offsets.p};
    if (c->ac.use_diag) {   // classify decodes the batch on every run (KernelArgs::pk_*)
        c->batch_pk.pk_words = (const uint32_t*)c->d_packed.p;
        c->batch_pk.pk_pos0 = 4 * P0;
        c->batch_pk.pk_exc_pos = c->d_exc_pos.p;
        c->batch_pk.pk_exc_byte = c->d_exc_byte.p;
        c->batch_pk.pk_e0 = 0;
        c->batch_pk.pk_e1 = n_exc;
        c->batch_pk.pk_len = ls.len;
        c->batch_pk.pk_gbase = ls.gbase;
        c->batch_pk.pk_call_lo = 0;
        c->bytes_full = false;
    } else {   // the exact kernels read bytes: unpack once
        HIP_TRY(c, nw::launch_unpack((const uint32_t*)c->d_packed.p, P0, base0, offsets[n], c->d_exc_pos.p,
                                     c->d_exc_byte.p, 0, n_exc, c->d_reads.p, c->reads_bias, c->stream, &ls));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->bytes_full = true;
    }
    c->ran = false;
    c->call_done = false;
    return NW_OK;
}

int nw_front::check_state(nw_ctx* c) {
    if (!c) return NW_E_INVALID;
    if (c->ref.empty()) return fail(c, NW_E_STATE, "nw_set_reference must come first");
    if (c->out_mode != NW_OUT_OPS) return fail(c, NW_E_STATE, "a packed batch needs nw_batch_set_output(NW_OUT_OPS)");
    return NW_OK;
}

int nw_front::device_of(const nw_ctx* c) { return c->device; }

namespace {

// The exact int32 kernel over a device work list (a.work_list / a.work_count): the
// multi-wave kernel (nw_exact.hip) when configured, else the one-wave kernel.
// Entries [0, exact_grid) go to the multi-wave kernel (one read per workgroup: the
// latency of a few reads), the rest, if any, to the one-wave kernel (throughput when
// many reads need the exact DP, e.g. an unrelated amplicon's HDR pass).
hipError_t launch_work(nw_ctx* c, const nw::KernelArgs& a, bool exact_small, hipStream_t cs) {
    // a work list expected short (ops_call: the recent chunks sent few reads to the exact
    // kernel): a small grid, so that the launch's empty blocks do not wait behind the other
    // chunks' kernels for LDS (a full grid of early-exiting blocks measured ~20 us per chunk)
    nw::LaunchCfg cfg = c->ac.cfg;
    if (a.work_list && exact_small) cfg.grid = std::min(cfg.grid, std::max(1, c->num_cus / 2));
    if (c->ac.exact_grid <= 0) return nw::launch(a, cfg, cs);
    hipError_t e = nw::launch_exact(a, c->ac.exact_grid, c->ac.exact_lds, c->ac.exact_tb_lds, c->ac.exact_slab, true, cs);
    if (e != hipSuccess) return e;
    nw::KernelArgs rest = a;
    rest.work_lo = c->ac.exact_grid;
    return nw::launch(rest, c->ac.cfg, cs);
}

// Launches the kernels for the p.n reads that start at read `base` of the
// uploaded arrays (outputs, records and fallback queue at the same index), configured by
// c->ac.  Everything is queued on p.cs (after a tail split: p.split_to); nothing synchronises.
int launch_range(nw_ctx* c, const ChunkPlan& p, int64_t base, ChunkLaunch* out) {
    ChunkLaunch& L = *out;
    L = ChunkLaunch{};
    hipStream_t& cs = L.cs;
    cs = p.cs;
    nw::KernelArgs a = p.pk;   // packed input: classify decodes the reads (KernelArgs::pk_*)
    a.reads = c->d_reads.p - c->reads_bias;
    a.offsets = c->d_offsets.p + base;
    a.n = p.n;
    a.prof = c->cur.prof;
    a.lut = c->d_lut.p;
    a.amp = c->cur.amp;
    a.La = (int32_t)c->ref.size();
    a.gap_open = c->gap_open;
    a.gap_extend = c->gap_extend;
    a.Lb_max = c->lb_max;
    a.out = c->d_out.p + base * 3 * c->ac.stride;
    a.stride = c->ac.stride;
    a.stats = c->d_stats.p + p.out_off + base;
    a.tb_global = p.s->d_tb.p;
    a.sub16 = c->d_sub16.p;
    a.rowpos = c->cur.rowpos;
    a.end_weight = c->end_weight;
    a.tail_prio = c->tail_prio;   // the latency-bound kernels of a chunk's chain at raised issue priority (-1.1 %)
    a.band_summ = p.lane ? 1 : 0;   // resident passes, the call's large chunks
    a.end_open = c->end_open;
    a.end_extend = c->end_extend;
    a.tb_wave_bytes = c->ac.cfg.tb_mode == nw::TB_GLOBAL_FULL ? nw::tb_bytes_per_wave(c->cur.R, c->lb_max) : 0;
    a.fallback_list = p.s->d_fallback.p + base;
    a.fallback_count = p.s->d_fallback_count.p;
    if (p.ops) {
        // runs into chunk-relative slots; rows are not written
        a.out = nullptr;
        a.ops = p.s->d_slots.p;
        a.ops_slot = c->ops_slot;
        a.ops_stride = c->ops_stride;
        a.nops = p.s->d_nops.p;
        a.spill = p.s->d_spill.p;
        a.spill_cap = c->spill_cap;
        a.ops_ctl = p.s->d_opsctl.p;
        // the band path writes every read's run count and zeroes its counters in its
        // first kernel (nw_band_classify): no memset launches in the chunk's chain
        if (!c->ac.use_diag || p.n <= 0) {
            HIP_TRY(c, hipMemsetAsync(p.s->d_nops.p, 0, sizeof(int32_t) * (size_t)std::max<int64_t>(p.n, 1), cs));
            HIP_TRY(c, hipMemsetAsync(p.s->d_opsctl.p, 0, nw::kSpillCtl * sizeof(int32_t), cs));
        }
    }
    if (c->ac.use_diag) {
        // length sort, certified band fill + walk per pass, exact int32 kernel on the rest
        if (p.n <= 0) return hipMemsetAsync(p.s->d_fallback_count.p, 0, nw::kChunkCounters * sizeof(int32_t), cs) == hipSuccess
                                  ? NW_OK : fail(c, NW_E_HIP, "hipMemsetAsync failed");
        a.lut6 = c->d_lut6.p;
        a.band_order = p.s->d_order.p;
        a.band_region = p.s->d_bregion.p;
        a.band_stride = c->ac.diag_stride;
        a.band_words = c->ac.diag_words;
        a.band_lb_cap = c->ac.diag_lb_cap;
        a.band_maxsub = 5 * c->scale;
        a.band_tab = c->d_btab.p;
        a.sort_key = p.s->d_sort_key.p;
        a.band_count = p.s->d_fallback_count.p + nw::kCntDp;
        a.amp2 = c->cur.amp2;
        a.seed_key = c->cur.seed_key;
        a.seed_pos = c->cur.seed_pos;
        a.n_seed = c->cur.n_seed;
        a.cls_img = c->cur.cls_img;
        a.cls_words = c->cur.cls_words;
        a.sub12_words = c->cur.sub12_words;
        a.sub12_table = p.sw->sub12_table ? 1 : 0;
        a.indel_onepass = p.sw->indel_onepass ? 1 : 0;
        a.amp_acgt = c->cur.amp_acgt ? 1 : 0;
        // seeded band: the packed classify marks the reads, the segment sort lists them apart
        // (sorted by their hits' diagonals), the wide level takes that list after its own
        L.seed_chunk = c->call.seed_on && p.pk.pk_words && c->ac.wide_fill.grid > 0 && c->cur.n_seed > 0;
        if (L.seed_chunk) {
            a.seed_info = p.s->d_seed.p;
            a.seed_info2 = p.s->d_seed2.p;
            a.seed_keys = c->call.seed_keys;
            a.seed_list = p.s->d_seed_list.p;
            a.seed_count = p.s->d_fallback_count.p + nw::kCntSeeded;
        }
        a.lb_status = p.s->d_lb.p;
        a.known2 = p.known ? p.known->d_k2.p : nullptr;
        // the three-substitution and one-indel checks on classify's queues (nw_band_cert; packed input,
        // ops output: the only classify that has those certificates)
        if (a.pk_words && a.ops) {
            a.cert_q = p.s->d_cert_q.p;
            a.cert_cnt = p.s->d_cert_cnt.p;
        }
        a.zero_ctl64 = p.zero_ctl;
        a.zero_ctl64_n = nw::kOpsCtlAll;
        const bool two = c->ac.diag16_fill.grid > 0 && !p.skip16;
        // wide first: packed input, ops output (classify has each read's substitution
        // count), an A C G T amplicon of at most 256 bp, a two-level chunk of a resident pass or a
        // one-chunk call; its keys must fit the segment sort (11 key bits, LDS)
        {
            const int wfk = c->ac.diag_lb_cap + 1, nkeys = c->ac.diag_lb_cap + 3 + a.seed_keys + wfk;
            L.wf_chunk = two && c->ac.wf_pairs > 0 && c->ac.wf_cap > 0 && a.pk_words && a.ops && p.wide_first_ok &&
                          a.La <= 256 && c->cur.amp_acgt && c->cur.amp2 && nkeys <= 2048 &&
                          4 * 17 * nkeys + 128 <= 64 * 1024;
            if (L.wf_chunk) {
                a.wf_keys = wfk;
                a.wf_cap = c->ac.wf_cap;
                a.wf_list = p.s->d_wf_list.p;
                a.wf_count = p.s->d_fallback_count.p + nw::kCntWfCount;
                a.wf_taken_n = p.s->d_fallback_count.p + nw::kCntWfTaken;
            }
        }
        HIP_TRY(c, nw::launch_band_sort(a, next_epoch(c), cs));
        tmark(c, p, cs, "classify+sort");
        const bool pev = p.phase_events;   // (resident passes that ask for them)
        if (pev) HIP_TRY(c, hipEventRecord(c->ev_sort, cs));
        const int64_t pairs = (p.n + 2) / 2;   // (the second level's list may hold one hole)
        // level 1 (16 diagonals) over the sorted reads; what it cannot certify -> redo list
        // -> level 2 (32 diagonals) -> the exact int32 kernel.  Kernels clamp the pair
        // ranges to the device-side counts.
        a.redo_list = p.s->d_redo.p;
        a.redo_count = p.s->d_fallback_count.p + nw::kCntRedo;
        if (two) a.redo_flags = p.s->d_redo_flags.p;   // the first level's walk writes every position's
        // a chunk whose first level hands on at most `direct` reads skips the second level on
        // the device: the wide level takes them (up to 1/16 of the chunk, as many as its region
        // holds), or without it the exact kernel (1024).  A chunk where more reads need more than
        // 16 diagonals (the HDR pass) keeps the second level, 4 read pairs per wavefront, and the
        // adaptive first-level choice sees them.  CRISPR_NW_DIRECT=0: always both levels.
        int direct = c->ac.wide_fill.grid > 0
                         ? (int)std::max<int64_t>(1024, std::min<int64_t>(p.n / 16, 2 * c->ac.wide_pairs))
                         : 1024;
        if (p.sw->direct >= 0) direct = p.sw->direct;
        if (!two) direct = 0;
        L.redo_direct = direct;
        // a chunk of >= 65536 reads with at most `direct` DP reads (device count) skips the first level too,
        // when the wide level can take them: one level's latency in its chain instead of three (in-process
        // A/B, C2 call 1.849 -> 1.771 ms, outputs identical; C1, C3, C5 unchanged).  Smaller launches (the
        // tests' batches) keep the first level.  CRISPR_NW_L1SKIP=0: off
        a.l1_skip = two && c->ac.wide_fill.grid > 0 && p.n >= 65536 && p.sw->l1skip ? direct : 0;
        // the wide-first list on the wide level's kernels beside the first level: the other compute
        // stream (a hardware queue of its own) from the sort to the exact kernel.  Its give-ups
        // join the exact kernel's list, as the later wide launch's.
        hipStream_t wf_side = cs == c->cstream[1] ? c->cstream[0] : c->cstream[1];
        if (L.wf_chunk) {
            nw::KernelArgs af = a;
            af.wf_take = 1;
            af.redo_flags = nullptr;
            af.seed_info = nullptr;
            af.seed_info2 = nullptr;
            af.seed_list = nullptr;
            af.band_summ = 0;
            af.band_region = p.s->d_wf_region.p;
            af.band_stride = c->ac.wide_stride;
            af.band_words = c->ac.wide_words;
            af.band_lb_cap = c->ac.wide_lb_cap;
            af.band_pair_lo = 0;
            af.band_pair_hi = c->ac.wf_pairs;
            af.fallback_list = p.s->d_fallback2.p + base;
            af.fallback_count = p.s->d_fallback_count.p + nw::kCntWideGiveUp;
            HIP_TRY(c, hipEventRecord(c->ev_wf0, cs));
            HIP_TRY(c, hipStreamWaitEvent(wf_side, c->ev_wf0, 0));
            HIP_TRY(c, nw::launch_band(nw::kWideDiags, af, c->ac.wf_fill, c->ac.wf_walk, wf_side, nullptr));
            HIP_TRY(c, hipEventRecord(c->ev_wf1, wf_side));
        }
        for (int lvl = two ? 0 : 1; lvl < 2; ++lvl) {
            nw::KernelArgs al = a;
            al.redo_direct = lvl == 1 ? direct : 0;
            const int W = lvl == 0 ? 16 : 32;
            if (lvl == 1 && two) {
                HIP_TRY(c, nw::launch_redo_compact(a, p.n, next_epoch(c), cs));
                tmark(c, p, cs, "redo");
                al.band_order = p.s->d_redo.p;
                al.band_count = a.redo_count;
                al.wf_list = nullptr;   // (the redo list holds whichever of those reads the first level had)
            }
            if (lvl == 1 && L.seed_chunk && c->call.seed_l2) {   // then the seeded list
                al.seed_l2 = 1;
                al.seed_flags = p.s->d_seed_flags.p;
            }
            al.band_stride = lvl == 0 ? c->ac.diag16_stride : c->ac.diag_stride;
            const int64_t pp = lvl == 0 ? c->ac.diag16_pass_pairs : c->ac.diag_pass_pairs;
            const nw::LaunchCfg& fc = lvl == 0 ? c->ac.diag16_fill : c->ac.diag_fill;
            const nw::LaunchCfg& wc = lvl == 0 ? c->ac.diag16_walk : c->ac.diag_walk;
            const bool first = lvl == (two ? 0 : 1);
            for (int64_t lo = 0; lo < pairs; lo += pp) {
                nw::KernelArgs ap = al;
                ap.band_pair_lo = lo;
                ap.band_pair_hi = std::min(pairs, lo + pp);
                HIP_TRY(c, nw::launch_band(W, ap, fc, wc, cs, pev && first && lo == 0 ? c->ev_fill : nullptr));
                tmark(c, p, cs, W == 16 ? "fill16+walk16" : "fill32+walk32");
                if (pev && first && lo == 0) HIP_TRY(c, hipEventRecord(c->ev_walk, cs));
            }
            if (first && p.split_to) {   // the latency-bound rest of the chunk on the tail stream
                HIP_TRY(c, hipEventRecord(p.split_ev, cs));
                HIP_TRY(c, hipStreamWaitEvent(p.split_to, p.split_ev, 0));
                cs = p.split_to;
            }
        }
        if (L.seed_chunk && c->call.seed_l2) {
            // the pairs of seeded reads the 32-diagonal level did not certify both of, compacted in the
            // seeded list's order (the wide level's pairs are that level's pairs: reads of nearby hits,
            // one sort segment): they replace that list (a certified partner is aligned again, the same)
            nw::KernelArgs ac = a;
            ac.band_order = p.s->d_seed_list.p;
            ac.band_count = a.seed_count;
            ac.redo_flags = p.s->d_seed_flags.p;
            ac.l1_skip = 0;
            ac.wf_list = nullptr;
            ac.redo_list = p.s->d_seed_list2.p;
            ac.redo_count = p.s->d_fallback_count.p + nw::kCntSeededL2;
            HIP_TRY(c, nw::launch_redo_compact(ac, p.n + p.n / 4096 + 2, next_epoch(c), cs, true));
            tmark(c, p, cs, "seed compact");
            a.seed_list = ac.redo_list;
            a.seed_count = ac.redo_count;
        }
        if (pev) HIP_TRY(c, hipEventRecord(c->ev_l2, cs));
        a.work_list = a.fallback_list;   // what the 16 / 32 levels could not certify
        a.work_count = p.s->d_fallback_count.p + nw::kCntExact;
        a.redo_direct = direct;
        if (c->ac.wide_fill.grid > 0) {
            // the wide level over that list (and, direct hand-off, the first level's redo list):
            // one read pair per wavefront, 128 diagonals: a few fill + walk launches of ~20 us
            // latency where the exact kernel took ~80 us per chunk; its give-ups -> the exact kernel
            nw::KernelArgs aw = a;
            aw.band_from_work = 1;
            aw.wf_list = nullptr;
            aw.band_count = a.work_count;
            aw.redo_flags = nullptr;
            aw.band_stride = c->ac.wide_stride;
            aw.band_words = c->ac.wide_words;
            aw.band_lb_cap = c->ac.wide_lb_cap;
            aw.band_pair_lo = 0;
            aw.band_pair_hi = c->ac.wide_pairs;
            aw.fallback_list = p.s->d_fallback2.p + base;
            aw.fallback_count = p.s->d_fallback_count.p + nw::kCntWideGiveUp;
            HIP_TRY(c, nw::launch_band(nw::kWideDiags, aw, c->ac.wide_fill, c->ac.wide_walk, cs, nullptr));
            tmark(c, p, cs, "wide");
            a.work_list = aw.fallback_list;
            a.work_count = aw.fallback_count;
            a.redo_direct = 0;
        }
        // the wide-first launch's give-ups are on the exact kernel's list: the join (nothing between the
        // first level and here reads what that launch writes -- its reads are on no other list, its region
        // is its own, the lists it shares with the wide launch above grow by atomics)
        if (L.wf_chunk) HIP_TRY(c, hipStreamWaitEvent(cs, c->ev_wf1, 0));
        HIP_TRY(c, launch_work(c, a, p.exact_small, cs));
        tmark(c, p, cs, "exact");
        return NW_OK;
    }
    HIP_TRY(c, hipMemsetAsync(p.s->d_fallback_count.p, 0, nw::kChunkCounters * sizeof(int32_t), cs));
    if (c->ac.exact_full) {   // long amplicon: every read through the multi-wave kernel
        if (p.n > 0)
            HIP_TRY(c, nw::launch_exact(a, c->ac.exact_grid, c->ac.exact_lds, c->ac.exact_tb_lds, c->ac.exact_slab, false,
                                        cs));
        return NW_OK;
    }
    if (p.n > 0) HIP_TRY(c, launch_work(c, a, p.exact_small, cs));   // every read (null work list)
    return NW_OK;
}

// Ops-mode buffers for chunks of up to `chunk` reads of a call over n reads:
// slots and counts per chunk (reused chunk after chunk, the compaction copies them
// out in-stream), the spill area, and two staging arrays (chunk c compacts into
// staging[c % 2] while the copy of chunk c - 1's runs may still be in flight).
int ops_reserve(nw_ctx* c, const Switches& sw, Scratch& S, int64_t chunk, int64_t n) {
    chunk = std::max<int64_t>(chunk, 1);
    c->ops_slot = sw.ops_slot;
    c->spill_cap = sw.spill_words;
    c->staging_cap = chunk * c->ops_slot + c->spill_cap;
    c->ops_stride = chunk;
    HIP_TRY(c, S.d_slots.reserve((size_t)(2 * chunk * c->ops_slot)));   // column-major + row-major areas
    HIP_TRY(c, S.d_nops.reserve((size_t)chunk));
    HIP_TRY(c, S.d_spill.reserve((size_t)c->spill_cap));
    HIP_TRY(c, S.d_opsctl.reserve(nw::kSpillCtl));
    HIP_TRY(c, c->d_ctl64.reserve(2 * nw::kOpsCtlAll));   // a dual call: one block per pass
    HIP_TRY(c, S.d_lb.reserve((size_t)nw::band_lookback_words(chunk)));
    HIP_TRY(c, c->d_opsoff.reserve((size_t)std::max<int64_t>(n, 1) + 1));
    HIP_TRY(c, S.d_staging.reserve((size_t)c->staging_cap));
    return NW_OK;
}

// Kernels of p.n reads starting at read `base`, then their compaction into
// staging[which]: ops_off of those reads (global: the call's running base in
// nw::kCtlTotal) and the chunk's kCtlBase, kCtlChunkTotal, kCtlError.
int launch_range_ops(nw_ctx* c, const ChunkPlan& p, int64_t base, ChunkLaunch* out, hipEvent_t staging_free = nullptr,
                     hipEvent_t prev_done = nullptr, int64_t* hctl = nullptr, int parity = 0,
                     const nw::OpsHostOut* host = nullptr) {
    int rc = launch_range(c, p, base, out);
    if (rc) return rc;
    const ChunkLaunch& L = *out;
    const hipStream_t cs = L.cs;
    // only the compaction writes the set's staging array: it waits for the copy of the
    // runs it held two chunks ago, and (the running base of ctl) for the previous
    // chunk's compaction on the other stream; the kernels before it wait for neither
    if (staging_free) HIP_TRY(c, hipStreamWaitEvent(cs, staging_free, 0));
    if (prev_done) HIP_TRY(c, hipStreamWaitEvent(cs, prev_done, 0));
    nw::OpsCounts cnt{};
    cnt.fallback = p.s->d_fallback_count.p;
    cnt.prio = c->tail_prio;
    if (c->ac.use_diag && p.n > 0) {
        cnt.band = p.s->d_fallback_count.p + nw::kCntDp;
        // second-level reads of a two-level chunk; a chunk run on the 32-diagonal level alone
        // counts its DP reads apart (nw::kCtlDpOneLevel: the adaptive choice reads two-level chunks only)
        if (c->ac.diag16_fill.grid > 0 && !p.skip16) cnt.redo = p.s->d_fallback_count.p + nw::kCntRedo;
        cnt.one_level = c->ac.diag16_fill.grid > 0 && p.skip16;
        cnt.direct = p.skip16 ? 0 : L.redo_direct;
        if (c->ac.wide_fill.grid > 0) cnt.exact = p.s->d_fallback_count.p + nw::kCntWideGiveUp;
        if (L.seed_chunk) {
            cnt.seeded = p.s->d_fallback_count.p + nw::kCntSeeded;
            cnt.seed_pad = p.s->d_fallback_count.p + nw::kCntSeedPad;
        }
        if (L.seed_chunk && c->call.seed_l2) cnt.seeded_l2 = p.s->d_fallback_count.p + nw::kCntSeededL2;
        if (L.wf_chunk) cnt.wide_first = p.s->d_fallback_count.p + nw::kCntWfTaken;
    }
    if (p.n <= 0) cnt.fallback = nullptr;
    nw::OpsKnown kn{};
    if (p.known) {   // the known alignment (computed on the upload stream) before any copy takes it
        const KnownSet& K = *p.known;
        HIP_TRY(c, hipStreamWaitEvent(cs, K.ev_known, 0));
        kn = nw::OpsKnown{K.d_kstat.p, K.d_kmisc.p, K.d_kslots.p, K.d_kslots.p + 2 * nw::kOpsSlot, nw::kOpsSlot};
    }
    HIP_TRY(c, nw::launch_ops_compact(p.s->d_nops.p, p.s->d_slots.p, c->ops_slot, c->ops_stride, p.s->d_spill.p, p.n,
                                      p.s->d_lb.p, next_epoch(c), parity, c->d_ctl64.p + p.ctl_pass * nw::kOpsCtlAll,
                                      c->d_opsoff.p + p.out_off + base,
                                      p.s->d_staging.p, c->staging_cap, p.s->d_opsctl.p, cnt, cs, hctl, host,
                                      c->d_stats.p + p.out_off + base, p.known ? &kn : nullptr));
    tmark(c, p, cs, "compact");
    return NW_OK;
}

// Page-locked host memory the device addresses with the same pointer (hipHostMalloc /
// hipHostRegister'd buffers, e.g. nw_host_alloc): kernels may store into it directly.
bool host_mapped(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost && at.devicePointer == p;
}

// NW_OUT_ROWS for the scope of a rows-only entry point (nw_align_batch, nw_align_multi)
struct RowsMode {
    nw_ctx* c;
    int saved;
    explicit RowsMode(nw_ctx* ctx) : c(ctx), saved(ctx->out_mode) { c->out_mode = NW_OUT_ROWS; }
    ~RowsMode() { c->out_mode = saved; }
};

int ops_events(nw_ctx* c, size_t chunks) {
    auto grow = [&](std::vector<hipEvent_t>& v, unsigned flags) -> hipError_t {
        while (v.size() < chunks) {
            hipEvent_t e = nullptr;
            hipError_t r = hipEventCreateWithFlags(&e, flags);
            if (r != hipSuccess) return r;
            v.push_back(e);
        }
        return hipSuccess;
    };
    HIP_TRY(c, grow(c->ev_in, hipEventDisableTiming));
    HIP_TRY(c, grow(c->ev_cs, hipEventDefault));
    HIP_TRY(c, grow(c->ev_ce, hipEventDefault));
    HIP_TRY(c, grow(c->ev_out, hipEventDisableTiming));
    HIP_TRY(c, grow(c->ev_bulk, hipEventDisableTiming));
    HIP_TRY(c, grow(c->ev_up, hipEventDisableTiming));
    if ((int64_t)chunks > c->h_ctl_chunks) {
        if (c->h_ctl) (void)hipHostFree(c->h_ctl);
        c->h_ctl = nullptr;
        c->h_ctl_chunks = 0;
        HIP_TRY(c, hipHostMalloc((void**)&c->h_ctl, sizeof(int64_t) * nw::kOpsCtl * chunks, hipHostMallocDefault));
        c->h_ctl_chunks = (int64_t)chunks;
    }
    return NW_OK;
}

int ops_error(nw_ctx* c, int64_t err) {
    if (err & nw::kOpsErrLookback) return fail(c, NW_E_HIP, "a device prefix scan waited too long for its predecessor blocks");
    if (err & nw::kOpsErrSpill) return fail(c, NW_E_NOMEM, "ops spill area full: reads with more than %d traceback runs need more "
                                            "than the spill area (%lld MB)", c->ops_slot,
                             (long long)(c->spill_cap * 4 >> 20));
    if (err & nw::kOpsErrStaging) return fail(c, NW_E_NOMEM, "ops staging array full");
    return NW_OK;
}

// the last resident run's path counters (set 0's d_fallback_count), once it is through
bool run_counts(nw_ctx* c, int32_t (&fb)[nw::kChunkCounters]) {
    (void)hipSetDevice(c->device);
    return hipStreamSynchronize(c->stream) == hipSuccess &&
           hipMemcpy(fb, c->sc[0].d_fallback_count.p, sizeof fb, hipMemcpyDeviceToHost) == hipSuccess;
}
}  // namespace

extern "C" {

int nw_batch_run_async(nw_ctx* c) {
    if (!c) return NW_E_INVALID;
    if (c->ref.empty() || !c->d_offsets.p) return fail(c, NW_E_STATE, "no batch uploaded");
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    int rc;
    c->call_done = false;
    c->phases_recorded = c->phase_events;
    // a resident pass: set 0, the context's stream, the wide-first launch beside it (no other chunk's kernels)
    const Switches sw = read_switches();
    ChunkPlan p(sw, &c->sc[0], c->stream, c->n, c->out_mode == NW_OUT_OPS);
    p.lane = c->lane_walk;
    p.wide_first_ok = true;
    p.phase_events = c->phase_events;
    p.pk = c->batch_pk;
    if (p.ops) {
        if (!c->sc[0].d_slots.p || c->sc[0].d_nops.cap < (size_t)std::max<int64_t>(c->n, 1))
            return fail(c, NW_E_STATE, "batch uploaded before nw_batch_set_output(NW_OUT_OPS)");
        // the compaction's control block: zeroed by the band path's classify (the pass's first kernel;
        // a memset launch here cost two fill kernels, ~9 us, per pass), else by a memset
        if (c->ac.use_diag && c->n > 0) {
            p.zero_ctl = c->d_ctl64.p;
        } else {
            HIP_TRY(c, hipMemsetAsync(c->d_ctl64.p, 0, nw::kOpsCtlAll * sizeof(int64_t), c->stream));
        }
        rc = launch_range_ops(c, p, 0, &c->last_launch);
    } else {
        rc = launch_range(c, p, 0, &c->last_launch);
    }
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    c->ran = true;
    return NW_OK;
}

int nw_batch_sync(nw_ctx* c, float* kernel_ms) {
    if (!c) return NW_E_INVALID;
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (kernel_ms) {
        *kernel_ms = 0.0f;
        if (c->ran) HIP_TRY(c, hipEventElapsedTime(kernel_ms, c->ev0, c->ev1));
    }
    return NW_OK;
}

int nw_batch_download(nw_ctx* c, char* aln_out, int64_t stride, nw_stat* stats) {
    if (!c) return NW_E_INVALID;
    if (!c->ran) return fail(c, NW_E_STATE, "nothing has run");
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->n == 0) return NW_OK;
    if (aln_out && c->out_mode == NW_OUT_OPS) return fail(c, NW_E_STATE, "ops output: use nw_batch_download_ops");
    if (c->ac.use_diag) {   // the band path's single-pass scans report a cut-off look-back here
        int32_t fb[nw::kCntLookback + 1] = {};
        HIP_TRY(c, hipMemcpy(fb, c->sc[0].d_fallback_count.p, sizeof fb, hipMemcpyDeviceToHost));
        if (fb[nw::kCntLookback]) return ops_error(c, nw::kOpsErrLookback);
    }
    if (stats)
        HIP_TRY(c, hipMemcpy(stats, c->d_stats.p, sizeof(nw::Stat) * (size_t)c->n, hipMemcpyDeviceToHost));
    if (aln_out) {
        if (stride < c->ac.stride) return fail(c, NW_E_INVALID, "stride %lld < required %lld", (long long)stride, (long long)c->ac.stride);
        if (stride == c->ac.stride) {
            HIP_TRY(c, hipMemcpy(aln_out, c->d_out.p, (size_t)c->n * 3 * c->ac.stride, hipMemcpyDeviceToHost));
        } else {
            HIP_TRY(c, hipMemcpy2D(aln_out, (size_t)stride, c->d_out.p, (size_t)c->ac.stride, (size_t)c->ac.stride,
                                   (size_t)c->n * 3, hipMemcpyDeviceToHost));
        }
    }
    return NW_OK;
}

int64_t nw_batch_algo_bytes(nw_ctx* c) {
    if (!c || !c->ran) return -1;
    std::vector<nw::Stat> st((size_t)c->n);
    if (c->n && nw_batch_download(c, nullptr, 0, (nw_stat*)st.data()) != NW_OK) return -1;
    int64_t total = 0;
    for (int64_t r = 0; r < c->n; ++r)
        if (!(st[(size_t)r].flags & NW_FLAG_EMPTY)) total += c->read_lens[(size_t)r] + 3ll * st[(size_t)r].aln_len + 16;
    return total;
}

int64_t nw_batch_cells(const nw_ctx* c) { return c ? c->cells : -1; }

int nw_batch_kernel_times(nw_ctx* c, float* fill_ms, float* walk_ms, float* rest_ms) {
    if (!c) return NW_E_INVALID;
    if (!c->ran) return fail(c, NW_E_STATE, "nothing has run");
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float total = 0.0f, f = 0.0f, w = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&total, c->ev0, c->ev1));
    if (c->ac.use_diag && c->n > 0 && !c->phases_recorded)
        return fail(c, NW_E_STATE, "the last run recorded no phase events (nw_batch_set_phase_events)");
    if (c->ac.use_diag && c->n > 0) {
        HIP_TRY(c, hipEventElapsedTime(&f, c->ev0, c->ev_fill));
        HIP_TRY(c, hipEventElapsedTime(&w, c->ev_fill, c->ev_walk));
    } else {
        f = total;
    }
    if (fill_ms) *fill_ms = f;
    if (walk_ms) *walk_ms = w;
    if (rest_ms) *rest_ms = total - f - w;
    return NW_OK;
}

int nw_batch_device_output(nw_ctx* c, void** d_aln, int64_t* stride, void** d_stats) {
    if (!c) return NW_E_INVALID;
    if (!c->ran || c->n <= 0) return fail(c, NW_E_STATE, "no resident batch (run nw_batch_run_async first)");
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (d_aln) *d_aln = c->d_out.p;
    if (stride) *stride = c->ac.stride;
    if (d_stats) *d_stats = c->d_stats.p;
    return NW_OK;
}

int nw_batch_device_ops(nw_ctx* c, void** d_ops, void** d_ops_off, void** d_stats, void** d_reads, void** d_offsets,
                        int64_t* reads_bias, int64_t* max_cols) {
    if (!c) return NW_E_INVALID;
    if (!c->ran || c->n <= 0 || c->out_mode != NW_OUT_OPS)
        return fail(c, NW_E_STATE, "no resident ops-mode batch (nw_batch_set_output(NW_OUT_OPS), run first)");
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int64_t ctl[nw::kOpsCtl];
    HIP_TRY(c, hipMemcpy(ctl, c->d_ctl64.p, sizeof ctl, hipMemcpyDeviceToHost));
    int rc = ops_error(c, ctl[nw::kCtlError]);
    if (rc) return rc;
    if (!c->bytes_full) {   // a packed batch: classify wrote the DP reads' bytes only; now every read's
        HIP_TRY(c, nw::launch_unpack((const uint32_t*)c->d_packed.p, c->batch_pos0 / 4, c->batch_base0,
                                     c->batch_base0 + c->batch_nbytes, c->d_exc_pos.p, c->d_exc_byte.p, 0,
                                     c->batch_n_exc, c->d_reads.p, c->reads_bias, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->bytes_full = true;
    }
    if (d_ops) *d_ops = c->sc[0].d_staging.p;   // one chunk: the call's runs from offset 0
    if (d_ops_off) *d_ops_off = c->d_opsoff.p;
    if (d_stats) *d_stats = c->d_stats.p;
    if (d_reads) *d_reads = c->d_reads.p;
    if (d_offsets) *d_offsets = c->d_offsets.p;
    if (reads_bias) *reads_bias = c->reads_bias;
    if (max_cols) *max_cols = c->ac.stride;
    return NW_OK;
}

int nw_batch_geometry(const nw_ctx* c, int32_t* rows_per_lane, int32_t* waves_per_block, int32_t* grid,
                      int32_t* lds_bytes, int32_t* tb_mode) {
    if (!c) return NW_E_INVALID;
    const nw::LaunchCfg& k = c->ac.use_diag ? c->ac.diag_fill : c->ac.cfg;
    if (rows_per_lane) *rows_per_lane = k.R;
    if (waves_per_block) *waves_per_block = k.wpb;
    if (grid) *grid = k.grid;
    if (lds_bytes) *lds_bytes = k.lds_bytes;
    if (tb_mode) *tb_mode = k.tb_mode;
    return NW_OK;
}

int64_t nw_batch_fallbacks(nw_ctx* c) {
    if (c && c->call_done) return c->call_counts[3];
    if (!c || !c->ran) return -1;
    int32_t v[nw::kChunkCounters];
    if (!run_counts(c, v)) return -1;
    if (!c->ac.use_diag) return 0;
    // the wide-first launch's reads are the wide level's too; a skipped second level
    // (KernelArgs::redo_direct): its reads went to the exact kernel
    const int direct = c->ac.diag16_fill.grid > 0 ? c->last_launch.redo_direct : 0;
    return v[nw::kCntExact] + v[nw::kCntWfTaken] + (direct > 0 && v[nw::kCntRedo] <= direct ? v[nw::kCntRedo] : 0);
}

int nw_align_batch(nw_ctx* c, const char* reads, const int64_t* offsets, int64_t n, char* aln_out,
                   int64_t stride, nw_stat* stats) {
    if (!c) return NW_E_INVALID;
    RowsMode rows_mode(c);
    int rc = nw_batch_upload(c, reads, offsets, n);
    if (rc) return rc;
    if ((rc = nw_batch_run_async(c))) return rc;
    if ((rc = nw_batch_sync(c, nullptr))) return rc;
    return nw_batch_download(c, aln_out, stride, stats);
}

// Pooled batches (CRISPRessoPooled.py:882-908 runs one CRISPResso
// process -- and one needle -- per amplicon): every read carries the index of
// its amplicon.  Reads are grouped by amplicon and uploaded once; each group's
// kernels are queued back to back on the context's stream (the profile upload
// of the next amplicon is ordered after them); one sync; outputs come back
// group by group and are scattered to the callers' read order.
int nw_align_multi(nw_ctx* c, const char* refs, const int64_t* ref_offsets, int32_t n_refs, const char* reads,
                   const int64_t* offsets, const int32_t* ref_of_read, int64_t n, char* aln_out, int64_t stride,
                   nw_stat* stats) {
    if (!c) return NW_E_INVALID;
    RowsMode rows_mode(c);
    if (n_refs <= 0 || !refs || !ref_offsets) return fail(c, NW_E_INVALID, "no amplicons");
    if (n < 0 || (n > 0 && (!reads || !offsets || !ref_of_read))) return fail(c, NW_E_INVALID, "bad batch");
    for (int32_t g = 0; g < n_refs; ++g) {
        const int64_t L = ref_offsets[g + 1] - ref_offsets[g];
        if (L <= 0 || L > kMaxRef) return fail(c, NW_E_UNSUPPORTED, "amplicon %d has length %lld", g, (long long)L);
    }
    (void)hipSetDevice(c->device);
    // group reads by amplicon (stable)
    std::vector<int64_t> first((size_t)n_refs + 1, 0);
    int32_t lb_all = 1;
    for (int64_t r = 0; r < n; ++r) {
        const int32_t g = ref_of_read[r];
        const int64_t len = offsets[r + 1] - offsets[r];
        if (g < 0 || g >= n_refs) return fail(c, NW_E_INVALID, "read %lld has amplicon index %d", (long long)r, g);
        if (len < 0 || len > (1 << 20)) return fail(c, NW_E_INVALID, "read %lld has length %lld", (long long)r, (long long)len);
        ++first[(size_t)g + 1];
        lb_all = std::max<int32_t>(lb_all, (int32_t)len);
    }
    for (int32_t g = 0; g < n_refs; ++g) first[(size_t)g + 1] += first[(size_t)g];
    std::vector<int64_t> order((size_t)n), fill(first.begin(), first.end() - 1);
    for (int64_t r = 0; r < n; ++r) order[(size_t)fill[(size_t)ref_of_read[r]]++] = r;
    int64_t stride_all = 16;
    for (int32_t g = 0; g < n_refs; ++g)
        if (first[(size_t)g + 1] > first[(size_t)g])
            stride_all = std::max(stride_all, stride_for((int)(ref_offsets[g + 1] - ref_offsets[g]), lb_all));
    if (aln_out && stride < stride_all)
        return fail(c, NW_E_INVALID, "stride %lld < required %lld", (long long)stride, (long long)stride_all);
    // packed reads in group order
    std::vector<int64_t> soff((size_t)n + 1, 0);
    for (int64_t s = 0; s < n; ++s) soff[(size_t)s + 1] = soff[(size_t)s] + (offsets[order[(size_t)s] + 1] - offsets[order[(size_t)s]]);
    std::vector<char> sreads((size_t)soff[(size_t)n]);
    for (int64_t s = 0; s < n; ++s) {
        const int64_t r = order[(size_t)s];
        std::memcpy(sreads.data() + soff[(size_t)s], reads + offsets[r], (size_t)(offsets[r + 1] - offsets[r]));
    }
    c->resident_ok = false;
    HIP_TRY(c, c->d_reads.reserve(sreads.size() + 512));
    HIP_TRY(c, c->d_offsets.reserve((size_t)n + 1));
    HIP_TRY(c, c->d_out.reserve((size_t)std::max<int64_t>(n, 1) * 3 * stride_all));
    HIP_TRY(c, c->d_stats.reserve((size_t)std::max<int64_t>(n, 1)));
    HIP_TRY(c, c->sc[0].d_fallback.reserve((size_t)std::max<int64_t>(n, 1)));
    HIP_TRY(c, c->sc[0].d_fallback2.reserve((size_t)std::max<int64_t>(n, 1)));   // indexed like d_fallback (+ group base)
    if (!sreads.empty())
        HIP_TRY(c, hipMemcpyAsync(c->d_reads.p, sreads.data(), sreads.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_offsets.p, soff.data(), sizeof(int64_t) * soff.size(), hipMemcpyHostToDevice, c->stream));
    // every amplicon's tables uploaded once (one arena); then one kernel group per amplicon,
    // queued back to back on the stream (configure() may grow buffers between groups)
    std::vector<std::string> amps((size_t)n_refs);
    for (int32_t g = 0; g < n_refs; ++g) amps[(size_t)g].assign(refs + ref_offsets[g], refs + ref_offsets[g + 1]);
    std::vector<Profile> profs;
    {
        int rc = upload_shared(c);
        if (!rc) rc = upload_profiles(c, amps, &profs);
        if (rc) return rc;
    }
    const Switches sw = read_switches();
    ChunkPlan p(sw, &c->sc[0], c->stream, 0, false);   // (rows: RowsMode)
    for (int32_t g = 0; g < n_refs; ++g) {
        const int64_t lo = first[(size_t)g], hi = first[(size_t)g + 1];
        if (hi == lo) continue;
        c->ref = amps[(size_t)g];
        c->cur = profs[(size_t)g];
        int rc = NW_OK;
        int32_t lb = 1;
        int64_t cells = 0;
        for (int64_t s = lo; s < hi; ++s) {
            const int64_t len = soff[(size_t)s + 1] - soff[(size_t)s];
            lb = std::max<int32_t>(lb, (int32_t)len);
            cells += (int64_t)c->ref.size() * len;
        }
        p.n = hi - lo;
        c->lb_max = lb;
        c->cells = cells;
        if ((rc = configure(c, sw, c->sc[0], p.n))) return rc;
        c->ac.stride = stride_all;   // every group's rows in one array
        if ((rc = launch_range(c, p, lo, &c->last_launch))) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // back to the callers' order
    std::vector<nw::Stat> st((size_t)n);
    if (n) HIP_TRY(c, hipMemcpy(st.data(), c->d_stats.p, sizeof(nw::Stat) * (size_t)n, hipMemcpyDeviceToHost));
    if (stats)
        for (int64_t s = 0; s < n; ++s) std::memcpy(&stats[order[(size_t)s]], &st[(size_t)s], sizeof(nw::Stat));
    if (aln_out) {
        std::vector<char> rows;
        for (int32_t g = 0; g < n_refs; ++g) {
            const int64_t lo = first[(size_t)g], hi = first[(size_t)g + 1];
            if (hi == lo) continue;
            rows.resize((size_t)(hi - lo) * 3 * stride_all);
            HIP_TRY(c, hipMemcpy(rows.data(), c->d_out.p + lo * 3 * stride_all, rows.size(), hipMemcpyDeviceToHost));
            for (int64_t s = lo; s < hi; ++s)
                for (int k = 0; k < 3; ++k)
                    std::memcpy(aln_out + (order[(size_t)s] * 3 + k) * stride, rows.data() + ((s - lo) * 3 + k) * stride_all,
                                (size_t)stride_all);
        }
    }
    c->n = 0;          // the per-batch getters describe nw_batch_upload batches only
    c->ran = false;
    c->ref.clear();    // the arena holds every amplicon: nw_set_reference before single-amplicon calls
    c->cur = Profile{};
    c->call_done = false;
    return NW_OK;
}

int64_t nw_required_stride_multi(const int64_t* ref_offsets, int32_t n_refs, int32_t max_read_len) {
    if (!ref_offsets || n_refs <= 0) return 0;
    int64_t st = 16;
    for (int32_t g = 0; g < n_refs; ++g)
        st = std::max(st, stride_for((int)(ref_offsets[g + 1] - ref_offsets[g]), std::max(max_read_len, 1)));
    return st;
}

int nw_batch_set_output(nw_ctx* c, int mode) {
    if (!c) return NW_E_INVALID;
    if (mode != NW_OUT_ROWS && mode != NW_OUT_OPS) return fail(c, NW_E_INVALID, "output mode %d", mode);
    c->out_mode = mode;
    c->ran = false;
    c->call_done = false;
    return NW_OK;
}

int nw_batch_download_ops(nw_ctx* c, uint32_t* ops_out, int64_t ops_cap, int64_t* ops_off, nw_stat* stats) {
    if (!c) return NW_E_INVALID;
    if (!c->ran || c->out_mode != NW_OUT_OPS) return fail(c, NW_E_STATE, "no ops-mode run (nw_batch_set_output)");
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int64_t ctl[nw::kOpsCtl];
    HIP_TRY(c, hipMemcpy(ctl, c->d_ctl64.p, sizeof ctl, hipMemcpyDeviceToHost));
    int rc = ops_error(c, ctl[nw::kCtlError]);
    if (rc) return rc;
    if (c->n > 0) {
        if (stats) HIP_TRY(c, hipMemcpy(stats, c->d_stats.p, sizeof(nw::Stat) * (size_t)c->n, hipMemcpyDeviceToHost));
        if (ops_off) HIP_TRY(c, hipMemcpy(ops_off, c->d_opsoff.p, sizeof(int64_t) * (size_t)c->n, hipMemcpyDeviceToHost));
    }
    if (ops_off) ops_off[c->n] = ctl[nw::kCtlChunkTotal];
    if (ctl[nw::kCtlChunkTotal] > ops_cap)
        return fail(c, NW_E_CAPACITY, "ops_cap %lld < %lld runs", (long long)ops_cap, (long long)ctl[nw::kCtlChunkTotal]);
    if (ctl[nw::kCtlChunkTotal] > 0 && ops_out)
        HIP_TRY(c, hipMemcpy(ops_out, c->sc[0].d_staging.p, sizeof(uint32_t) * (size_t)ctl[nw::kCtlChunkTotal], hipMemcpyDeviceToHost));
    return NW_OK;
}

// The call-level path (host batch in -> per-read records in host
// memory).  Chunks of reads flow through three streams: every chunk's reads and
// offsets are queued on s_in up front; chunk k's kernels + compaction wait for its
// upload on the compute stream; its records and offsets go back on s_out as soon as
// they exist, its runs once the host has read the chunk's run total (the host waits
// for chunk k - 1 while chunk k computes).  Compute of chunk k + 2 reuses chunk k's
// staging array after its copy.  Host buffers should be pinned (nw_host_alloc /
// nw_host_register) for the copies to run asynchronously at PCIe rate.
}  // extern "C"

namespace {

// Switches::host_timing: where a pipelined call's host time goes (stderr; diagnostics)
struct HostTimer {
    bool on;
    const char* what;
    double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // ops_call: scan, configure, setup, uploads, launch, wait, sync
    std::chrono::steady_clock::time_point t0, last;
    HostTimer(bool on_, const char* w) : on(on_), what(w) { t0 = last = std::chrono::steady_clock::now(); }
    void lap(int k) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        t[k] += std::chrono::duration<double, std::milli>(now - last).count();
        last = now;
    }
    ~HostTimer() {
        if (!on) return;
        t[7] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::fprintf(stderr, "nw host ms (%s): %.2f %.2f %.2f %.2f %.2f %.2f %.2f total %.2f\n", what, t[0], t[1], t[2],
                     t[3], t[4], t[5], t[6], t[7]);
    }
};

// 2-bit packed batch (nw_align_ops_packed): bases by batch position, exceptions ascending.
struct PackedInput {
    const uint8_t* packed;
    const int64_t* exc_pos;
    const uint8_t* exc_byte;
    int64_t n_exc;
    const uint16_t* lens = nullptr;   // the reads' lengths (nw_align_ops_packed_lens): they cross instead of the offsets
};

// Amplicon groups of a pooled call: reads [first[g], first[g + 1]) align against
// refs[g] (tables profs[g] in the arena).
struct Groups {
    const std::vector<std::string>* refs;
    const std::vector<Profile>* profs;
    const std::vector<int64_t>* first;
};

// A dual call (nw_align_dual_ops_packed_lens, CORE:1808-1828): every read against refs[0] (pass 0:
// the caller's stats / ops_off / ops_out) and refs[1] (pass 1: these outputs; null ops_out2: records
// only), the two passes' chunks interleaved -- pass 1's chunk of a read range runs as soon as that
// range is uploaded, on the time the upload-bound pass 0 leaves the GPU idle.
struct Dual {
    uint32_t* ops_out2;
    int64_t ops_cap2;
    int64_t* ops_off2;
    nw_stat* stats2;
};

// Known copies (nw_ctx::resident_ref): the resident batch was aligned against amplicon A and is
// now aligned against H (the HDR pass, CORE:1808-1828): reads equal to A all have A's alignment
// against H.  A goes through the exact kernel once, as a one-read batch with its own buffers, on
// the upload stream (idle in a resident pass) while the chunks start; classify flags A's copies
// (KernelArgs::known2) and every chunk's compaction waits for the alignment and gives it to them.
// Off unless both sequences are A C G T, of one length <= 256 (classify's lane-per-read compare)
// and at most the batch's longest read (the exact kernel's LDS sizing).
int known_prepare(nw_ctx* c, const std::string& A, hipStream_t ks, int set = 0) {
    KnownSet& K = c->kset[set];
    K.on = false;
    const int La = (int)c->ref.size();
    if ((int)A.size() != La || La > 256 || La > c->lb_max || A == c->ref || !c->cur.amp_acgt || !c->cur.amp2 ||
        c->ac.cfg.R <= 0 || c->end_weight)
        return NW_OK;
    for (char ch : A) {
        const char u = (char)(ch & 0xDF);
        if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return NW_OK;
    }
    std::vector<uint32_t> w2((size_t)(La + 15) / 16 + 2, 0u);
    for (int p = 0; p < La; ++p) w2[(size_t)p / 16] |= (uint32_t)(((unsigned char)A[p] >> 1) & 3u) << (2 * (p % 16));
    const int64_t tbw = c->ac.cfg.tb_mode == nw::TB_GLOBAL_FULL ? nw::tb_bytes_per_wave(c->ac.cfg.R, c->lb_max) : 0;
    HIP_TRY(c, K.d_kbytes.reserve((size_t)La + 64));
    HIP_TRY(c, K.d_koff.reserve(2));
    HIP_TRY(c, K.d_k2.reserve(w2.size()));
    HIP_TRY(c, K.d_kslots.reserve(2 * nw::kOpsSlot + 4096));   // column-major + row-major slot, spill
    HIP_TRY(c, K.d_kstat.reserve(1));
    HIP_TRY(c, K.d_kmisc.reserve(16));
    HIP_TRY(c, K.d_kfb.reserve(1));
    HIP_TRY(c, K.d_ktb.reserve((size_t)std::max<int64_t>(tbw * c->ac.cfg.wpb, 16)));
    if (!K.ev_known) HIP_TRY(c, hipEventCreateWithFlags(&K.ev_known, hipEventDisableTiming));
    const int64_t off[2] = {0, La};
    HIP_TRY(c, hipMemcpyAsync(K.d_kbytes.p, A.data(), (size_t)La, hipMemcpyHostToDevice, ks));
    HIP_TRY(c, hipMemcpyAsync(K.d_koff.p, off, sizeof off, hipMemcpyHostToDevice, ks));
    HIP_TRY(c, hipMemcpyAsync(K.d_k2.p, w2.data(), 4 * w2.size(), hipMemcpyHostToDevice, ks));
    HIP_TRY(c, hipMemsetAsync(K.d_kmisc.p, 0, 16 * sizeof(int32_t), ks));
    nw::KernelArgs ka{};
    ka.reads = K.d_kbytes.p;
    ka.offsets = K.d_koff.p;
    ka.n = 1;
    ka.prof = c->cur.prof;
    ka.lut = c->d_lut.p;
    ka.amp = c->cur.amp;
    ka.La = La;
    ka.gap_open = c->gap_open;
    ka.gap_extend = c->gap_extend;
    ka.Lb_max = c->lb_max;
    ka.stats = K.d_kstat.p;
    ka.tb_global = K.d_ktb.p;
    ka.tb_wave_bytes = tbw;
    ka.fallback_list = K.d_kfb.p;
    ka.fallback_count = K.d_kmisc.p + 8;
    ka.ops = K.d_kslots.p;
    ka.ops_slot = nw::kOpsSlot;
    ka.ops_stride = 1;
    ka.nops = K.d_kmisc.p;
    ka.spill = K.d_kslots.p + 2 * nw::kOpsSlot;
    ka.spill_cap = 4096;
    ka.ops_ctl = K.d_kmisc.p + 1;
    nw::LaunchCfg one = c->ac.cfg;
    one.grid = 1;
    HIP_TRY(c, nw::launch(ka, one, ks));
    HIP_TRY(c, hipEventRecord(K.ev_known, ks));
    K.on = true;
    return NW_OK;
}

// A chunk [lo, hi) of a call's reads, of one amplicon group; a dual call's pass-1 chunk reads the
// bytes its pass-0 twin (chunk `up`) uploaded
struct Chunk { int64_t lo, hi; int g; int pass; int64_t up; };

// The chunks of a call over n reads, at most `chunk` reads each, none across two groups; a dual
// call's two passes over each read range alternate.
std::vector<Chunk> plan_chunks(int64_t n, int64_t chunk, const Groups* groups, bool dual) {
    std::vector<Chunk> chunks;
    const int ngroups = groups ? (int)groups->refs->size() : 1;
    // sizes ramp up and down at both ends of the call (chunk / 4, chunk / 2, ...): the
    // first chunk's upload and the last chunk's records are the pipeline's serial head
    // and tail; every chunk in between is a full chunk
    // (8:4:2 ramps and other chunk sizes measured no faster)
    auto sizes = [&](int64_t len) {
        std::vector<int64_t> v;
        if (len <= chunk) {
            v.push_back(len);
            return v;
        }
        std::vector<int64_t> head, tail;
        int64_t left = len;
        for (int64_t part : {chunk / 4, chunk / 2}) {   // ramp parts in pairs (one at each end)
            if (part >= 1024 && left > 2 * (part + chunk)) {
                head.push_back(part);
                tail.push_back(part);
                left -= 2 * part;
            }
        }
        for (int64_t x : head) v.push_back(x);
        const int64_t mid = (left + chunk - 1) / chunk;
        for (int64_t q = 0; q < mid; ++q) v.push_back(left / mid + (q < left % mid ? 1 : 0));
        for (auto it = tail.rbegin(); it != tail.rend(); ++it) v.push_back(*it);
        return v;
    };
    if (dual) {
        int64_t lo = 0;
        for (int64_t len : sizes(n)) {
            if (len <= 0) continue;
            const int64_t k0 = (int64_t)chunks.size();
            chunks.push_back({lo, lo + len, 0, 0, k0});
            chunks.push_back({lo, lo + len, 1, 1, k0});
            lo += len;
        }
    } else {
        for (int g = 0; g < ngroups; ++g) {
            const int64_t g0 = groups ? (*groups->first)[(size_t)g] : 0, g1 = groups ? (*groups->first)[(size_t)g + 1] : n;
            int64_t lo = g0;
            for (int64_t len : sizes(g1 - g0)) {
                if (len <= 0) continue;
                chunks.push_back({lo, lo + len, g, 0, (int64_t)chunks.size()});
                lo += len;
            }
        }
    }
    return chunks;
}

// One ops_call: its arguments and what its steps (below, in the call's order) hand on.
struct OpsCall {
    const Switches& sw;
    const char* reads; const int64_t* offsets; int64_t n; bool upload;
    const Groups* groups; const PackedInput* pk; const Dual* dual;
    HostTimer ht;
    // per pass: the caller's outputs, the runs' running total
    nw_stat* st_p[2]; int64_t* oo_p[2]; uint32_t* ops_p[2]; int64_t cap_p[2], total_p[2] = {0, 0};
    int64_t err = 0;                  // the chunks' kCtlError, or-ed
    bool cap_short = false;
    int64_t chunk = 1;                // reads of a full chunk
    std::vector<Chunk> chunks;
    int64_t nchunks = 0;
    int ngroups = 1, nsets = 1;
    int64_t lag = 1;                  // chunk k's runs are copied once chunk k + lag is queued
    bool tail_split = false;
    int64_t base0 = 0, nbytes = 0;    // the batch's bytes [base0, base0 + nbytes) of the caller's array
    // packed input: the device copy of the packed stream starts at byte P0 (4-aligned: one
    // dword = 16 bases), the unpacked bytes at batch position base0 & ~15 (16-B stores)
    int64_t P0 = 0, pk_hi = 0;        // (pk_hi: end of the caller's packed bytes)
    bool lens_on = false;             // the reads' lengths cross instead of their offsets
    int64_t ngroups_len = 0, h2d_bytes = 0;
    int32_t lb_max = 1;
    int64_t n_short = 0;              // reads the 16-diagonal band cannot hold (Lb <= La - 16): the seeded band's
    std::vector<AmpConfig> gcfg;      // per group: what configure() decided (size_sets)
    int configured = -1;              // the group c->ref / c->cur / c->ac hold
    bool packed_resident = false, direct_out = false;   // (direct_out: the last chunk's compaction writes the caller's buffers)
    std::vector<char> direct_done, one_level;   // per chunk: it did; it ran the 32-diagonal level alone
    bool skip16 = false, any_diag = false;
    int64_t runs_queued = 0;          // chunks [0, runs_queued) had their runs copies queued early (the last iteration)
    // chunk k's predecessor of its own pass, the newest chunk of its pass the host has read back
    // lag chunks behind it, and its index within its pass (a dual call's passes alternate)
    int64_t prev_same(int64_t j) const { return dual ? j - 2 : j - 1; }
    int64_t newest_same(int64_t k, int64_t back) const {
        int64_t j = k - back;
        if (dual && j >= 0 && chunks[(size_t)j].pass != chunks[(size_t)k].pass) --j;
        return j;
    }
    int64_t in_pass(int64_t k) const { return dual ? k >> 1 : k; }
};

// Every exit of ops_call, the HIP_TRY ones too, leaves no per-call state behind.
struct CallReset {
    nw_ctx* c;
    ~CallReset() {
        c->call = CallState{};
        c->n = 0;   // the per-batch getters describe nw_batch_upload batches only; the call used its buffers
        c->batch_pk = nw::KernelArgs{};
    }
};

// an error after uploads were queued: they read the caller's arrays
int drain(nw_ctx* c, int rc) {
    (void)hipStreamSynchronize(c->s_in);
    return rc;
}

// Every upload queued up front on s_in: the copy engine streams the batch while chunks compute.
int queue_uploads(nw_ctx* c, OpsCall& o) {
    const PackedInput* pk = o.pk;
    const int64_t* offsets = o.offsets;
    const int64_t n = o.n;
    HIP_TRY(c, hipEventRecord(c->ev_h0, c->s_in));
    if (pk && o.upload && pk->n_exc > 0) {
        HIP_TRY(c, hipMemcpyAsync(c->d_exc_pos.p, pk->exc_pos, sizeof(int64_t) * (size_t)pk->n_exc,
                                  hipMemcpyHostToDevice, c->s_in));
        HIP_TRY(c, hipMemcpyAsync(c->d_exc_byte.p, pk->exc_byte, (size_t)pk->n_exc, hipMemcpyHostToDevice, c->s_in));
        o.h2d_bytes += 9 * pk->n_exc;
    }
    // Packed input with the reads' lengths (nw_align_ops_packed_lens): per read its uint16
    // length crosses PCIe instead of its int64 offset (plus every kLenGroup-th offset, once):
    // 2 B instead of 8, 70.5 -> 64.5 MB per 1M C2 reads.  The call is PCIe-bound at the
    // margin (8 MB more upload measured +0.15 ms).  Each chunk's unpack launch rebuilds its
    // offsets (nw::LenSeg); the scan (scan_lengths) checks the lengths against the group offsets
    // before any kernel runs.
    o.lens_on = pk && pk->lens && o.upload && n > 0;
    const int64_t ngroups_len = o.ngroups_len = o.lens_on ? n / nw::kLenGroup + 1 : 0;
    if (o.lens_on) {
        // the group bases and chunk 0's lengths in one copy (the device layout is [bases][lengths])
        const int64_t n0 = o.nchunks > 0 ? o.chunks[0].hi - o.chunks[0].lo : 0;
        const int64_t need = 8 * ngroups_len + 2 * n0;
        if (need > c->h_lens_cap) {
            if (c->h_lens) (void)hipHostFree(c->h_lens);
            c->h_lens = nullptr;
            c->h_lens_cap = 0;
            HIP_TRY(c, hipHostMalloc((void**)&c->h_lens, (size_t)need, hipHostMallocDefault));
            c->h_lens_cap = need;
        }
        if (c->d_lens.reserve((size_t)(8 * ngroups_len + 2 * n + 64)) != hipSuccess)
            return fail(c, NW_E_NOMEM, "device allocation failed for %lld reads", (long long)n);
        int64_t* gb = (int64_t*)c->h_lens;
        for (int64_t g = 0; g < ngroups_len; ++g) gb[g] = offsets[g * nw::kLenGroup];
        std::memcpy(c->h_lens + 8 * ngroups_len, pk->lens + o.chunks[0].lo, 2 * (size_t)n0);
        HIP_TRY(c, hipMemcpyAsync(c->d_lens.p, c->h_lens, (size_t)need, hipMemcpyHostToDevice, c->s_in));
        o.h2d_bytes += need;
    }
    for (int64_t k = 0; o.upload && k < o.nchunks; ++k) {
        if (o.chunks[(size_t)k].pass) continue;   // its twin's upload holds its reads
        const int64_t lo = o.chunks[(size_t)k].lo, hi = o.chunks[(size_t)k].hi;
        const int64_t b0 = offsets[lo], b1 = offsets[hi];
        // chunk 0's lengths went with the group bases; every later chunk's in one copy queued
        // ahead of chunk 1's bases: fewer copies, fewer gaps on the engine (C4 16.9 -> 16.4 ms,
        // C5 17.2 -> 17.0 ms against one lengths copy per chunk)
        if (o.lens_on && k == (o.dual ? 2 : 1)) {
            HIP_TRY(c, hipMemcpyAsync(c->d_lens.p + 8 * ngroups_len + 2 * lo, pk->lens + lo, 2 * (size_t)(n - lo),
                                      hipMemcpyHostToDevice, c->s_in));
            o.h2d_bytes += 2 * (n - lo);
        }
        if (pk) {
            // the chunk's packed dwords (the caller's bytes only; edge bases are masked)
            const int64_t q0 = std::max((b0 / 16) * 4, o.base0 / 4), q1 = std::min((b1 + 15) / 16 * 4, o.pk_hi);
            if (b1 > b0 && q1 > q0) {
                HIP_TRY(c, hipMemcpyAsync(c->d_packed.p + (q0 - o.P0), pk->packed + q0, (size_t)(q1 - q0),
                                          hipMemcpyHostToDevice, c->s_in));
                o.h2d_bytes += q1 - q0;
            }
        } else if (b1 > b0) {
            HIP_TRY(c, hipMemcpyAsync(c->d_reads.p + (b0 - o.base0), o.reads + b0, (size_t)(b1 - b0),
                                      hipMemcpyHostToDevice, c->s_in));
            o.h2d_bytes += b1 - b0;
        }
        if (!o.lens_on) {
            HIP_TRY(c, hipMemcpyAsync(c->d_offsets.p + lo, offsets + lo, sizeof(int64_t) * (size_t)(hi - lo + 1),
                                      hipMemcpyHostToDevice, c->s_in));
            o.h2d_bytes += (int64_t)sizeof(int64_t) * (hi - lo + 1);
        }
        HIP_TRY(c, hipEventRecord(c->ev_in[(size_t)k], c->s_in));
    }
    if (o.upload) HIP_TRY(c, hipEventRecord(c->ev_h1, c->s_in));
    return NW_OK;
}

// The reads' lengths while the uploads stream: the longest (o.lb_max), how many the 16-diagonal
// band cannot hold (o.n_short), and that each is valid.
int scan_lengths(nw_ctx* c, OpsCall& o) {
    const int64_t* offsets = o.offsets;
    const int64_t n = o.n;
    nw_host::Pool& pool = nw_host::Pool::get();
    int64_t mx = 1, mn = 0;
    const int64_t short_la = o.ngroups == 1 ? (int64_t)c->ref.size() : 0;
    // a vectorisable pass, split over the host pool for large batches (memory-bound; the exact
    // read is found only on error)
    const int parts = (int)std::min<int64_t>(pool.threads(), std::max<int64_t>(1, n >> (o.lens_on ? 16 : 15)));
    std::vector<int64_t> pmx((size_t)parts, 1), pmn((size_t)parts, 0), pbad((size_t)parts, -1), psh((size_t)parts, 0);
    // lengths given: the longest read, and every length must equal its offsets' difference
    // (the device rebuilds the offsets from the lengths and the group bases, the host expands
    // the rows from the offsets: a mismatch would make them refer to different bytes)
    if (o.lens_on)
        pool.run(parts, [&](int q) {
            int64_t g0, g1;
            nw_host::Pool::range(o.ngroups_len, parts, q, &g0, &g1);
            unsigned a = 1;
            int64_t sh = 0;
            for (int64_t g = g0; g < g1 && pbad[(size_t)q] < 0; ++g) {
                const int64_t r0 = g * nw::kLenGroup, r1 = std::min(n, r0 + nw::kLenGroup);
                int64_t diff = 0;
                for (int64_t r = r0; r < r1; ++r) {
                    const unsigned l = o.pk->lens[r];
                    a = l > a ? l : a;
                    sh += (int64_t)l + 16 <= short_la;
                    diff |= (int64_t)l ^ (offsets[r + 1] - offsets[r]);
                }
                if (diff) pbad[(size_t)q] = g;
            }
            pmx[(size_t)q] = a;
            psh[(size_t)q] = sh;
        });
    else   // longest / shortest read
        pool.run(parts, [&](int q) {
            int64_t lo, hi, a = 1, b = 0, sh = 0;
            nw_host::Pool::range(n, parts, q, &lo, &hi);
            for (int64_t r = lo; r < hi; ++r) {
                const int64_t len = offsets[r + 1] - offsets[r];
                a = len > a ? len : a;
                b = len < b ? len : b;
                sh += len + 16 <= short_la;
            }
            pmx[(size_t)q] = a;
            pmn[(size_t)q] = b;
            psh[(size_t)q] = sh;
        });
    for (int q = 0; q < parts; ++q) {
        mx = std::max(mx, pmx[(size_t)q]);
        mn = std::min(mn, pmn[(size_t)q]);
        o.n_short += psh[(size_t)q];
        if (pbad[(size_t)q] >= 0)
            return drain(c, fail(c, NW_E_INVALID, "lens differ from the offsets in reads %lld ..",
                                 (long long)(pbad[(size_t)q] * nw::kLenGroup)));
    }
    if (mn < 0 || mx > (1 << 20))
        for (int64_t r = 0; r < n; ++r) {
            const int64_t len = offsets[r + 1] - offsets[r];
            if (len < 0 || len > (1 << 20))
                return drain(c, fail(c, NW_E_INVALID, "read %lld has length %lld", (long long)r, (long long)len));
        }
    o.lb_max = (int32_t)mx;
    return NW_OK;
}

// c->ref / c->cur / c->ac become group g's (a pooled call: assigned from the sizing pass's
// decisions, not re-derived: configure's occupancy queries are host API calls).
void use_group(nw_ctx* c, OpsCall& o, int g) {
    if (g == o.configured) return;
    if (o.groups) {
        c->ref = (*o.groups->refs)[(size_t)g];
        c->cur = (*o.groups->profs)[(size_t)g];
    }
    c->ac = o.gcfg[(size_t)g];
    o.configured = g;
}

// Launch configuration of the chunks: configure() for every amplicon group on every scratch set
// the call uses, once up front (grids sized for a full chunk also serve a shorter last chunk:
// the kernels clamp to the counts): the buffers reach their largest size before anything is
// queued (no allocation inside the pipeline).
// (A resident pass -- the C3 HDR pass -- in 524288- / 1048576-read chunks measured 8.95 / 10.77
// vs 5.85 ms per C3 step: the wide level's region per chunk overflows to the exact kernel and the
// last chunk's records go over PCIe unoverlapped; without the tail stream 5.78 vs 5.70.)
int size_sets(nw_ctx* c, OpsCall& o) {
    const int64_t n = o.n, chunk = o.chunk;
    o.gcfg.assign((size_t)o.ngroups, AmpConfig{});
    int rc = NW_OK;
    for (int si = 0; si < o.nsets && !rc; ++si) {
        Scratch& S = c->sc[si];
        for (int g = 0; g < o.ngroups && !rc; ++g) {
            const int64_t gn = o.groups ? (*o.groups->first)[(size_t)g + 1] - (*o.groups->first)[(size_t)g] : n;
            if (gn <= 0 && o.ngroups != 1) continue;
            if (o.groups) {
                c->ref = (*o.groups->refs)[(size_t)g];
                c->cur = (*o.groups->profs)[(size_t)g];
            }
            rc = configure(c, o.sw, S, std::max(std::max<int64_t>(1, std::min(chunk, gn)), std::min(chunk, n)));
            if (!rc) o.gcfg[(size_t)g] = c->ac;   // (every set's buffers sized: the last set's decisions, as each set's)
        }
        if (!rc) rc = ops_reserve(c, o.sw, S, chunk, o.dual ? 2 * n + 1 : n);
        // the fallback lists are indexed by the call's read (d_fallback + chunk base)
        if (!rc && (S.d_fallback.reserve((size_t)std::max<int64_t>(n, 1)) != hipSuccess ||
                    S.d_fallback2.reserve((size_t)std::max<int64_t>(n, 1)) != hipSuccess))
            rc = fail(c, NW_E_NOMEM, "device allocation failed for %lld reads", (long long)n);
    }
    o.configured = !rc && o.ngroups == 1 ? 0 : -1;   // (several groups: the pipeline assigns each chunk's)
    return rc;
}

// Copies of a known sequence from one alignment (packed classify): the caller's (nw_set_known),
// or in a resident pass against a new amplicon the one the batch was last aligned against.  The
// alignment runs on the upload stream of a resident pass (idle), else on the tail stream (its
// first tail packet comes a chunk's chain later); every compaction waits for it
int prepare_known(nw_ctx* c, OpsCall& o) {
    int rc = NW_OK;
    c->kset[0].on = c->kset[1].on = false;
    if (o.dual) {   // each pass's copies of the other pass's amplicon
        for (int q = 0; q < 2 && o.n > 0; ++q) {
            use_group(c, o, q);
            if (c->ac.use_diag && (rc = known_prepare(c, (*o.groups->refs)[(size_t)(1 - q)], c->cstream[2], q))) return rc;
        }
        return NW_OK;
    }
    const std::string& K = (!c->known_seq.empty() && c->known_seq != c->ref) ? c->known_seq
                           : (!o.upload && c->resident_ref != c->ref) ? c->resident_ref : c->known_seq;
    const bool packed_classify = (o.pk != nullptr && o.upload) || (!o.upload && c->resident_packed);
    if (!o.groups && packed_classify && c->ac.use_diag && o.n > 0 && !K.empty() && K != c->ref)
        rc = known_prepare(c, K, o.upload ? c->cstream[2] : c->s_in);
    return rc;
}

// Chunk k's runs go back once the host has read its total.  (Copying an estimate of them as soon
// as the chunk is done measured no gain on the 1M-read call and a loss on the pooled call's 96
// small chunks: not kept.)
int copy_runs(nw_ctx* c, OpsCall& o, int64_t k) {
    o.ht.lap(4);
    HIP_TRY(c, hipEventSynchronize(c->ev_ce[(size_t)k]));
    o.ht.lap(5);
    const int64_t* h = c->h_ctl + nw::kOpsCtl * k;
    o.err |= h[nw::kCtlError];
    const int64_t cb = h[nw::kCtlBase], tot = h[nw::kCtlChunkTotal];
    const int pass = o.chunks[(size_t)k].pass;
    uint32_t* po = o.ops_p[pass];
    if (!po) {   // records only (a scores-only pass, CORE:1740-1741): the runs stay on the device
    } else if (cb + tot > o.cap_p[pass]) o.cap_short = true;
    else if (tot > 0 && !o.direct_done[(size_t)k])
        HIP_TRY(c, hipMemcpyAsync(po + cb, c->sc[k % o.nsets].d_staging.p, sizeof(uint32_t) * (size_t)tot,
                                  hipMemcpyDeviceToHost, c->s_out));
    HIP_TRY(c, hipEventRecord(c->ev_out[(size_t)k], c->s_out));
    o.total_p[pass] = cb + tot;
    if (po) c->ops_d2h_bytes += 4 * tot;
    return NW_OK;
}

// Chunk k of the pipeline: its plan, its kernels and compaction, its outputs' copies.
int run_chunk(nw_ctx* c, OpsCall& o, int64_t k) {
    const Chunk& ch = o.chunks[(size_t)k];
    const int64_t lo = ch.lo, hi = ch.hi, nchunks = o.nchunks;
    const int nsets = o.nsets, pass = ch.pass;
    const PackedInput* pk = o.pk;
    const int64_t* offsets = o.offsets;
    int rc = NW_OK;
    ChunkPlan p(o.sw, &c->sc[k % nsets], c->cstream[k % std::min(nsets, kComputeStreams)], hi - lo, true);
    if (o.tail_split) {
        p.cs = c->cstream[k % 2];
        // the last chunks keep their tail on their own compute stream (no later chunk's bulk
        // queues behind it there): their tails overlap instead of queueing on the tail stream
        // (a one-amplicon call keeps each chunk's tail on its compute stream: in-process A/Bs,
        // C1 shape 5.05 -> 4.49 ms, C2 1.977 -> 1.958 ms; the pooled call's many small chunks and the
        // dual call keep the tail stream: 16.35 vs 19.14 ms, 5.34 vs 5.46 ms)
        p.split_to = o.groups ? c->cstream[2] : nullptr;
        p.split_ev = c->ev_bulk[(size_t)k];
        // the set's previous chunk (k - 3) must be through its tail
        if (k >= nsets) HIP_TRY(c, hipStreamWaitEvent(p.cs, c->ev_ce[(size_t)(k - nsets)], 0));
    }
    if (o.upload) HIP_TRY(c, hipStreamWaitEvent(p.cs, c->ev_in[(size_t)ch.up], 0));
    // (a timing event here sat in every chunk's chain: only with the host timing on)
    if (o.ht.on) HIP_TRY(c, hipEventRecord(c->ev_cs[(size_t)k], p.cs));
    use_group(c, o, ch.g);
    p.out_off = pass ? o.n + 1 : 0;   // a dual call's pass 1: its records and run offsets after pass 0's
    p.ctl_pass = pass;
    p.known = c->kset[o.dual ? pass : 0].on ? &c->kset[o.dual ? pass : 0] : nullptr;
    // the first level's lane walk + stop summary on chunks of >= 65536 reads of one
    // amplicon (in-process A/Bs, wave walk vs lane walk on every such chunk: C2 1.954 vs 1.961 ms,
    // C3 5.578 vs 5.570, C1 7.082 vs 7.070 -- the same -- while the kernel-resident pass of the
    // same kernels runs 0.81 -> 0.69 ms; the pooled call's 96 small chunks lost: 16.61 vs 17.15 ms)
    p.lane = (!o.groups || o.dual) && hi - lo >= 65536;
    p.wide_first_ok = nchunks == 1 && !o.groups && !o.dual;   // (a one-chunk call: the other compute stream is idle)
    // A dual call unpacks each read range once, in its pass-0 chunk, when either pass runs the exact
    // kernels on bytes: the unpack stores a decoded 'A' at every exception's place before its second
    // launch corrects it, and no kernel of the other pass may see that (across the passes
    // only a byte's final value is ever stored).  The pass-1 twin waits for the unpacked bytes (and the
    // offsets rebuilt with them) instead of writing them again; a band-path pass beside it stores final
    // values only (classify's write_read_bytes).
    const bool dual_unpack = pk && o.upload && o.dual && !(o.gcfg[0].use_diag && o.gcfg[1].use_diag);
    if (dual_unpack && pass == 1) {
        HIP_TRY(c, hipStreamWaitEvent(p.cs, c->ev_up[(size_t)ch.up], 0));
    } else if (pk && o.upload && (!c->ac.use_diag || dual_unpack)) {
        // the exact kernels read bytes: the chunk's bases -> bytes + exceptions
        const int64_t b0 = offsets[lo], b1 = offsets[hi];
        const int64_t e0 = std::lower_bound(pk->exc_pos, pk->exc_pos + pk->n_exc, b0) - pk->exc_pos;
        const int64_t e1 = std::lower_bound(pk->exc_pos, pk->exc_pos + pk->n_exc, b1) - pk->exc_pos;
        nw::LenSeg lsk{};
        if (o.lens_on)
            lsk = nw::LenSeg{(const uint16_t*)(c->d_lens.p + 8 * o.ngroups_len), (const int64_t*)c->d_lens.p,
                             lo / nw::kLenGroup, hi / nw::kLenGroup - lo / nw::kLenGroup + 1, lo, hi, c->d_offsets.p};
        const nw::LenSeg* ls = o.lens_on ? &lsk : nullptr;
        HIP_TRY(c, nw::launch_unpack((const uint32_t*)c->d_packed.p, o.P0, b0, b1, c->d_exc_pos.p, c->d_exc_byte.p,
                                     e0, e1, c->d_reads.p, c->reads_bias, p.cs, ls));
        if (dual_unpack) HIP_TRY(c, hipEventRecord(c->ev_up[(size_t)k], p.cs));
    }
    if (c->ac.use_diag && ((pk && o.upload) || o.packed_resident)) {
        // band path: classify decodes the chunk from the 2-bit stream itself (rebuilding its
        // offsets from the lengths) and writes only the bytes of the reads that need the DP --
        // no unpack launch, and 2 bits per base read instead of a byte written and re-read
        p.pk.pk_words = (const uint32_t*)c->d_packed.p;
        p.pk.pk_pos0 = 4 * o.P0;
        p.pk.pk_exc_pos = c->d_exc_pos.p;
        p.pk.pk_exc_byte = c->d_exc_byte.p;
        if (o.upload) {
            p.pk.pk_e0 = std::lower_bound(pk->exc_pos, pk->exc_pos + pk->n_exc, offsets[lo]) - pk->exc_pos;
            p.pk.pk_e1 = std::lower_bound(pk->exc_pos, pk->exc_pos + pk->n_exc, offsets[hi]) - pk->exc_pos;
        } else {
            p.pk.pk_e0 = 0;
            p.pk.pk_e1 = c->resident_n_exc;
        }
        if (o.lens_on) {
            p.pk.pk_len = (const uint16_t*)(c->d_lens.p + 8 * o.ngroups_len);
            p.pk.pk_gbase = (const int64_t*)c->d_lens.p;
        }
        p.pk.pk_call_lo = lo;
    }
    o.any_diag = o.any_diag || c->ac.use_diag;
    // adaptive first level: when most of the DP reads of the chunks done so far needed the
    // 32-diagonal level (e.g. the HDR pass: a 10-bp block substitution costs two 10-bp gaps
    // or 10 mismatches, beyond what 16 diagonals certify), the next chunks skip the
    // 16-diagonal level (its fill and walk would be spent on reads it hands on).  (The
    // converse -- sending the first level's give-ups straight to the exact kernel when few
    // reach the second level -- measured 3 % on C2 but is not safe to choose from earlier
    // chunks: with the HDR reads last (synth.c3_workload), the last chunks sent tens of
    // thousands of reads to the exact kernel, 15 -> 24 ms per C3 step.  The same choice
    // made on the device from the chunk's own count measured no gain: the skipped
    // level's launches remain.)
    // The newest chunk the host has read back (k - lag - 1, synchronised in copy_runs)
    // decides from its own counts when it ran both levels; while the level is skipped
    // every 4th chunk runs both again, so input that changes back is noticed.
    // (a dual call: its pass's own chunks; the passes' counts accumulate apart)
    static const int64_t zero[nw::kOpsCtl] = {};
    const int64_t jn = o.newest_same(k, o.lag + 1);
    const int64_t* hn = jn >= 0 ? c->h_ctl + nw::kOpsCtl * jn : zero;
    const int64_t* hpn = jn >= 0 && o.prev_same(jn) >= 0 ? c->h_ctl + nw::kOpsCtl * o.prev_same(jn) : zero;
    if (o.dual) o.skip16 = false;   // (each chunk decides for its own pass)
    if (o.sw.adapt && jn >= 0) {   // pooled calls too: one library's amplicons, one read source
        if (!o.one_level[(size_t)jn]) {
            const int64_t dp = (hn[nw::kCtlDp] - hn[nw::kCtlDpOneLevel]) - (hpn[nw::kCtlDp] - hpn[nw::kCtlDpOneLevel]);
            const int64_t l2 = hn[nw::kCtlL2] - hpn[nw::kCtlL2];
            o.skip16 = dp >= 2048 && 2 * l2 > dp;
        } else {
            o.skip16 = (o.in_pass(k) & 3) != 0;
        }
    }
    p.skip16 = o.skip16;
    o.one_level[(size_t)k] = o.skip16 && c->ac.diag16_fill.grid > 0;
    // (No second-level launches while the newest chunk read back needed none -- the wide level
    // taking the whole redo list -- measured 1.926 vs 1.939 ms per C2 call but is not safe to
    // choose from earlier chunks: the C3 amplicon pass, whose HDR reads come last, sent ~30k of
    // them past the wide level's region to the exact kernel, 5.96 -> 14.5 ms per C3 step.  Lost
    // on C2 and not kept either: spinning on the chunk events, the last chunks' tails on their
    // own compute streams, explicit chunk ramps ending in small chunks, the last chunk's DP
    // reads straight to the wide level, the lane walk in the chunks (1.975 vs 1.959 ms; C3 14.50
    // vs 14.56), the 32-diagonal level's lane walk, the last chunk alone
    // on a high-priority stream, each chunk's upload split over two streams: +0.01 to +0.58 ms.)
    // the exact kernel's grid: small while the newest chunk read back sent it few reads
    // (after the wide level it gets the rare read no band certifies)
    p.exact_small = jn < 0 || hn[nw::kCtlReachedExact] - hpn[nw::kCtlReachedExact] < 256;
    // diagnostics: the last chunks' launches
    p.trace = o.sw.trace > 0 && k >= nchunks - o.sw.trace;
    p.chunk = (int)k;
    // the compaction writes the chunk's ctl into h_ctl[k] itself
    nw::OpsHostOut ho{};
    const bool direct_k = o.direct_out && k == nchunks - 1;
    if (direct_k) ho = nw::OpsHostOut{(const int4*)(c->d_stats.p + p.out_off + lo), (int4*)(o.st_p[pass] + lo),
                                      o.oo_p[pass] + lo, o.ops_p[pass], o.ops_p[pass] ? o.cap_p[pass] : 0};
    // the compaction after its pass's previous one (the running base of the pass's ctl block)
    if ((rc = launch_range_ops(c, p, lo, &c->last_launch, k >= nsets ? c->ev_out[(size_t)(k - nsets)] : nullptr,
                               o.prev_same(k) >= 0 ? c->ev_ce[(size_t)o.prev_same(k)] : nullptr,
                               c->h_ctl + nw::kOpsCtl * k, (int)(o.in_pass(k) & 1), direct_k ? &ho : nullptr)))
        return rc;
    o.direct_done[(size_t)k] = direct_k;
    HIP_TRY(c, hipEventRecord(c->ev_ce[(size_t)k], c->last_launch.cs));
    // s_out order: chunk k - lag's runs (their size is known once that chunk is done:
    // the host waits for it, so lag = nsets - 1 chunks stay queued ahead), then chunk
    // k's records and offsets
    if (k >= o.lag && (rc = copy_runs(c, o, k - o.lag))) return rc;
    // the last chunk: every earlier chunk's runs are queued ahead of its records, so they
    // copy while it computes (otherwise s_out would hold them behind the last chunk's end)
    if (k == nchunks - 1)
        for (int64_t j = std::max<int64_t>(0, k - o.lag + 1); j < k; ++j) {
            if ((rc = copy_runs(c, o, j))) return rc;
            o.runs_queued = j + 1;
        }
    if (!direct_k) {
        HIP_TRY(c, hipStreamWaitEvent(c->s_out, c->ev_ce[(size_t)k], 0));
        HIP_TRY(c, hipMemcpyAsync(o.st_p[pass] + lo, c->d_stats.p + p.out_off + lo,
                                  sizeof(nw::Stat) * (size_t)(hi - lo), hipMemcpyDeviceToHost, c->s_out));
        HIP_TRY(c, hipMemcpyAsync(o.oo_p[pass] + lo, c->d_opsoff.p + p.out_off + lo,
                                  sizeof(int64_t) * (size_t)(hi - lo), hipMemcpyDeviceToHost, c->s_out));
    }
    c->ops_d2h_bytes += (int64_t)(sizeof(nw::Stat) + sizeof(int64_t)) * (hi - lo);
    return NW_OK;
}

// After the last copy: the call's counters, device times, diagnostics, and what stays resident.
int finish_call(nw_ctx* c, OpsCall& o) {
    const int64_t n = o.n, nchunks = o.nchunks;
    if (nchunks > 0) {   // the call's reads by path (nw_batch_path_counts / nw_batch_fallbacks; a dual call: pass 0's)
        int64_t kl = nchunks - 1;   // the last chunk of pass 0 (a dual call interleaves the passes)
        while (kl > 0 && o.chunks[(size_t)kl].pass != 0) --kl;
        const int64_t* h = c->h_ctl + nw::kOpsCtl * kl;
        const bool two = o.any_diag && c->ac.diag16_fill.grid > 0;
        c->call_counts[0] = o.any_diag ? n - h[nw::kCtlDp] : 0;
        c->call_counts[1] = two ? h[nw::kCtlDp] - h[nw::kCtlDpOneLevel] : 0;                // first level: two-level chunks' DP reads
        c->call_counts[2] = o.any_diag ? (two ? h[nw::kCtlL2] + h[nw::kCtlDpOneLevel] : h[nw::kCtlDp]) : 0;
        c->call_counts[3] = h[nw::kCtlExact];
        c->call_exact = h[nw::kCtlReachedExact];
        c->call_wide_first = h[nw::kCtlWideFirst];
    }
    c->call_done = true;
    // device times: the upload span on s_in, the chunks' compute spans summed
    c->ops_h2d_ms = 0.0f;
    c->ops_compute_ms = 0.0f;
    c->ops_h2d_bytes = o.upload ? o.h2d_bytes : 0;
    if (nchunks > 0) {
        if (o.upload)
            HIP_TRY(c, hipEventElapsedTime(&c->ops_h2d_ms, c->ev_h0, c->ev_h1));
        // the chunks' compute spans summed (host timing on: their start events), else the call's device
        // span, first upload to the last chunk's end
        for (int64_t k = 0; k < nchunks; ++k) {
            float ms = 0.0f;
            if (o.ht.on) HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_cs[(size_t)k], c->ev_ce[(size_t)k]));
            c->ops_compute_ms += ms;
        }
        if (!o.ht.on) HIP_TRY(c, hipEventElapsedTime(&c->ops_compute_ms, c->ev_h0, c->ev_ce[(size_t)nchunks - 1]));
        for (size_t i = 0; i < c->call.trace_used; ++i) {
            float t = 0;
            (void)hipEventElapsedTime(&t, c->ev_h0, c->trace_ev[i].second);
            std::fprintf(stderr, "  trace chunk %s: %.1f us\n", c->trace_ev[i].first.c_str(), 1e3 * t);
        }
        if (o.ht.on)   // per chunk (ms from the first upload): upload done, compute start, compute end
            for (int64_t k = 0; k < nchunks; ++k) {
                const float a = 0;   // (the uploads' events do not time: ev_h1 is the last one's end)
                float b = 0, e = 0;
                (void)hipEventElapsedTime(&b, c->ev_h0, c->ev_cs[(size_t)k]);
                (void)hipEventElapsedTime(&e, c->ev_h0, c->ev_ce[(size_t)k]);
                std::fprintf(stderr, "  chunk %lld [%lld reads]: in %.3f start %.3f end %.3f\n", (long long)k,
                             (long long)(o.chunks[(size_t)k].hi - o.chunks[(size_t)k].lo), a, b, e);
            }
    }
    c->resident_ok = true;   // the batch stays in HBM for nw_align_ops_resident
    if (o.upload) {
        c->resident_packed = o.pk != nullptr;
        c->resident_n_exc = o.pk ? o.pk->n_exc : 0;
    }
    c->resident_n = n;
    c->resident_lo = o.base0;
    c->resident_hi = o.base0 + o.nbytes;
    c->resident_ref = o.groups ? std::string() : c->ref;   // a later resident pass's known sequence
    int rc = ops_error(c, o.err);
    if (rc) return rc;
    if (o.cap_short)
        return fail(c, NW_E_CAPACITY, "ops_cap %lld < %lld runs (ops_off holds the offsets)",
                    (long long)(o.total_p[0] > o.cap_p[0] ? o.cap_p[0] : o.cap_p[1]),
                    (long long)(o.total_p[0] > o.cap_p[0] ? o.total_p[0] : o.total_p[1]));
    return NW_OK;
}

// nw_align_ops (upload = true), nw_align_ops_resident (the batch the last call
// uploaded, still in HBM: no upload) and nw_align_multi_ops (groups: chunks never
// straddle two amplicons; each chunk's kernels use its amplicon's tables).
int ops_call(nw_ctx* c, const Switches& sw, const char* reads, const int64_t* offsets, int64_t n, uint32_t* ops_out,
             int64_t ops_cap, int64_t* ops_off, nw_stat* stats, bool upload, const Groups* groups = nullptr,
             const PackedInput* pk = nullptr, const Dual* dual = nullptr) {
    if (!c) return NW_E_INVALID;
    if (dual && (!groups || groups->refs->size() != 2 || !upload || !pk || !dual->stats2 || !dual->ops_off2))
        return fail(c, NW_E_INVALID, "bad dual call");
    OpsCall o{sw, reads, offsets, n, upload, groups, pk, dual,
              HostTimer(sw.host_timing, "scan configure setup uploads launch wait sync"),
              {stats, dual ? dual->stats2 : nullptr}, {ops_off, dual ? dual->ops_off2 : nullptr},
              {ops_out, dual ? dual->ops_out2 : nullptr}, {ops_cap, dual ? dual->ops_cap2 : 0}};
    if (!groups && c->ref.empty()) return fail(c, NW_E_STATE, "nw_set_reference must come first");
    if (n < 0 || (n > 0 && (!offsets || (upload && !reads && !(pk && pk->packed)) || !stats)) || !ops_off)
        return fail(c, NW_E_INVALID, "bad batch");
    if (pk && pk->n_exc > 0 && (!pk->exc_pos || !pk->exc_byte)) return fail(c, NW_E_INVALID, "bad exception list");
    if (!upload && !(c->resident_ok && c->resident_n == n && (n == 0 || (c->resident_lo == offsets[0] &&
                                                                          c->resident_hi == offsets[n]))))
        return fail(c, NW_E_STATE, "no resident batch of these %lld reads (nw_align_ops uploads one)", (long long)n);
    if (upload) c->resident_ok = false;
    (void)hipSetDevice(c->device);
    const int64_t chunk = o.chunk = std::max<int64_t>(1, std::min<int64_t>(sw.chunk, n));
    o.chunks = plan_chunks(n, chunk, groups, dual != nullptr);
    o.ngroups = groups ? (int)groups->refs->size() : 1;
    const int64_t nchunks = o.nchunks = (int64_t)o.chunks.size();
    o.base0 = n ? offsets[0] : 0;
    o.nbytes = n ? offsets[n] - o.base0 : 0;
    int rc = NW_OK;
    // the chunks' edges must be in order before anything is copied (the scan below checks
    // every read, after the uploads are queued: the copy engine starts streaming at once)
    for (const Chunk& ch : o.chunks)
        if (offsets[ch.lo] > offsets[ch.hi] || offsets[ch.lo] < o.base0 || offsets[ch.hi] > offsets[n])
            return fail(c, NW_E_INVALID, "offsets out of order at read %lld", (long long)ch.lo);
    CallReset reset{c};
    o.P0 = (o.base0 / 16) * 4;
    o.pk_hi = n ? (offsets[n] + 3) / 4 : 0;
    if (pk && upload &&
        (c->d_packed.reserve((size_t)std::max<int64_t>(o.pk_hi - o.P0, 0) + 64) != hipSuccess ||
         c->d_exc_pos.reserve((size_t)std::max<int64_t>(pk->n_exc, 1)) != hipSuccess ||
         c->d_exc_byte.reserve((size_t)std::max<int64_t>(pk->n_exc, 1)) != hipSuccess))
        return fail(c, NW_E_NOMEM, "device allocation failed for the packed batch");
    if (c->d_reads.reserve((size_t)o.nbytes + 512 + 16) != hipSuccess || c->d_offsets.reserve((size_t)n + 1) != hipSuccess ||
        c->d_stats.reserve((size_t)std::max<int64_t>(dual ? 2 * n + 2 : n, 1)) != hipSuccess)
        return fail(c, NW_E_NOMEM, "device allocation failed for %lld reads", (long long)n);
    if ((rc = ops_events(c, (size_t)std::max<int64_t>(nchunks, 1)))) return rc;
    o.ht.lap(2);
    if (upload) c->reads_bias = pk ? (o.base0 & ~(int64_t)15) : o.base0;
    if ((rc = queue_uploads(c, o))) return rc;
    o.ht.lap(3);
    if ((rc = scan_lengths(c, o))) return rc;
    // the seeded band: a one-amplicon call whose classify decodes a packed batch
    // (an upload, or the resident batch of one), with reads the 16-diagonal band cannot hold; its
    // sort keys must fit the segment sort (11 key bits, LDS)
    {
        const int La = (int)c->ref.size();
        const int keys = La / 2 + 2, cap = La + nw::kBandDiags - 1;
        // (a few such reads -- C2's long deletions -- the 32-diagonal level holds: not worth the keys)
        c->call.seed_on = o.ngroups == 1 && o.n_short > 0 && 64 * o.n_short >= n &&
                          (pk != nullptr || (!upload && c->resident_packed)) && !c->end_weight && La <= 1024 &&
                          cap + 3 + keys <= 2048 &&
                          4 * 17 * (cap + keys + 3) + 128 <= 64 * 1024;   // segsort_lds_bytes (default LDS limit)
        c->call.seed_keys = c->call.seed_on ? keys : 0;
        c->call.seed_l2 = sw.seed32;
        c->call.seed_pairs = c->call.seed_on ? std::min<int64_t>(chunk, o.n_short) / 2 + 1 : 0;
    }
    o.ht.lap(0);
    c->ran = false;
    c->call_done = false;
    c->lb_max = o.lb_max;
    c->cells = 0;
    // two sets overlap a chunk's tail with the next chunk's bulk; a third measured slower
    // (328M vs 306M reads/s at 262144-read chunks, scripts/gpu_sets_sweep.sh)
    const bool several = (n + chunk - 1) / std::max<int64_t>(chunk, 1) > 1 || o.ngroups > 1;
    // tail split: a chunk's bulk kernels (unpack, classify, sort, first band level) on compute
    // stream k mod 2, its latency-bound rest (second level, wide level, exact kernel,
    // compaction) on one tail stream in chunk order, three scratch sets: chunk k + 2's bulk no
    // longer queues behind chunk k's tail (C5 pooled call 24.7 -> 21.6 ms, C2 unchanged).
    // (Chunk k's compaction waits for the copy of the runs a set back, ev_out[k - nsets],
    // recorded once the host has read that chunk's total: one set cannot pipeline chunks.)
    static_assert(kScratchSets >= 6 && kComputeStreams == 3, "the tail split needs three scratch sets (a dual call six)");
    o.tail_split = several;
    // a dual call: three sets per pass (set k % 6 keeps a pass's chunks on its own sets), so a slow
    // pass-1 chunk never holds back the set a pass-0 chunk needs
    o.nsets = dual ? 6 : several ? 3 : 1;
    rc = size_sets(c, o);
    o.ht.lap(1);
    o.one_level.assign((size_t)std::max<int64_t>(nchunks, 1), 0);
    // (Rounds 3-5 ran a score-only diagonal pass over the reads of the amplicon's length ahead of
    // the first level's traceback fill in all but a call's last chunk, switched off per chunk when it
    // handed most reads on.  With round 6's classify certificates taking nearly all of those reads its
    // sweep only lengthened each chain: removed, in-process A/Bs C2 call 1.894 -> 1.833 ms, resident
    // pass 0.536 -> 0.484 ms, dual call 5.28 -> 5.12 ms, C1 shape 3.03 -> 2.98 ms)
    if (rc) return drain(c, rc);
    HIP_TRY(c, hipMemsetAsync(c->d_ctl64.p, 0, 2 * nw::kOpsCtlAll * sizeof(int64_t), c->stream));
    if ((rc = prepare_known(c, o))) return rc;
    // The last chunk's records, offsets and runs are written by its compaction kernel straight
    // into the caller's buffers when they are page-locked: no copies and no host round trip
    // after the call's last kernel (2.31 -> 2.27 ms per 1M-read call)
    const int last_pass = nchunks >= 1 ? o.chunks[(size_t)nchunks - 1].pass : 0;
    o.direct_out = nchunks >= 1 && host_mapped(o.st_p[last_pass]) && host_mapped(o.oo_p[last_pass]) &&
                   (!o.ops_p[last_pass] || host_mapped(o.ops_p[last_pass]));
    // (The last two / three chunks writing their outputs the same way measured 1.968 vs 2.002 / 2.015 vs
    // 2.392 ms per C2 call in round 6: the PCIe writes then sit in those chunks' chains.  Not kept.)
    o.direct_done.assign((size_t)std::max<int64_t>(nchunks, 1), 0);
    c->ops_d2h_bytes = 0;
    // (a dual call: its pass's chunk two back -- the host never waits for the other pass's chunks)
    o.lag = dual ? 4 : std::max(1, o.nsets - 1);
    // chunk k waits on ev_out[k - nsets], recorded by copy_runs(k - nsets) once k - nsets <= k' - lag for
    // an earlier k': every wait needs lag < nsets
    if (nchunks > o.nsets && o.lag >= o.nsets)
        return fail(c, NW_E_INVALID, "ops call: run-copy lag must be below the scratch sets");
    // a resident packed batch (nw_align_ops_resident after nw_align_ops_packed): the band path's
    // classify decodes it again; the exact kernels alone (-endweight, amplicons over 1024 bp)
    // need its bytes, unpacked once here before any chunk
    o.packed_resident = !upload && c->resident_packed && c->ac.use_diag;
    if (!upload && c->resident_packed && !c->ac.use_diag && n > 0)
        HIP_TRY(c, nw::launch_unpack((const uint32_t*)c->d_packed.p, o.P0, o.base0, o.base0 + o.nbytes, c->d_exc_pos.p,
                                     c->d_exc_byte.p, 0, c->resident_n_exc, c->d_reads.p, c->reads_bias, c->stream));
    // the ctl reset and the exceptions' upload are on the first compute stream and s_in:
    // both compute streams start after them
    HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    for (int k = 1; k < std::min(o.nsets, kComputeStreams); ++k)
        HIP_TRY(c, hipStreamWaitEvent(c->cstream[k], c->ev_start, 0));
    for (int64_t k = 0; k < nchunks; ++k)
        if ((rc = run_chunk(c, o, k))) return rc;
    for (int64_t k = std::max<int64_t>(o.runs_queued, nchunks - o.lag); k < nchunks; ++k)
        if ((rc = copy_runs(c, o, k))) return rc;
    o.ht.lap(4);
    HIP_TRY(c, hipStreamSynchronize(c->s_out));
    o.ht.lap(6);
    ops_off[n] = o.total_p[0];
    if (dual) dual->ops_off2[n] = o.total_p[1];
    return finish_call(c, o);
}

}  // namespace

extern "C" {

int nw_align_ops(nw_ctx* c, const char* reads, const int64_t* offsets, int64_t n, uint32_t* ops_out, int64_t ops_cap,
                 int64_t* ops_off, nw_stat* stats) {
    return ops_call(c, read_switches(), reads, offsets, n, ops_out, ops_cap, ops_off, stats, true);
}

int nw_align_ops_packed(nw_ctx* c, const uint8_t* packed, const int64_t* offsets, int64_t n, const int64_t* exc_pos,
                        const uint8_t* exc_byte, int64_t n_exc, uint32_t* ops_out, int64_t ops_cap, int64_t* ops_off,
                        nw_stat* stats) {
    if (n_exc < 0) return fail(c, NW_E_INVALID, "bad exception count");
    const PackedInput pk{packed, exc_pos, exc_byte, n_exc};
    return ops_call(c, read_switches(), nullptr, offsets, n, ops_out, ops_cap, ops_off, stats, true, nullptr, &pk);
}

int nw_align_ops_packed_lens(nw_ctx* c, const uint8_t* packed, const int64_t* offsets, const uint16_t* lens, int64_t n,
                             const int64_t* exc_pos, const uint8_t* exc_byte, int64_t n_exc, uint32_t* ops_out,
                             int64_t ops_cap, int64_t* ops_off, nw_stat* stats) {
    if (n_exc < 0) return fail(c, NW_E_INVALID, "bad exception count");
    if (n > 0 && !lens) return fail(c, NW_E_INVALID, "no lengths");
    const PackedInput pk{packed, exc_pos, exc_byte, n_exc, lens};
    return ops_call(c, read_switches(), nullptr, offsets, n, ops_out, ops_cap, ops_off, stats, true, nullptr, &pk);
}

int nw_align_ops_resident(nw_ctx* c, const int64_t* offsets, int64_t n, uint32_t* ops_out, int64_t ops_cap,
                          int64_t* ops_off, nw_stat* stats) {
    return ops_call(c, read_switches(), nullptr, offsets, n, ops_out, ops_cap, ops_off, stats, false);
}

// Pooled batch, ops output (CRISPRessoPooled.py:882-908 runs one CRISPResso -- one
// needle per pass -- per amplicon): one call, every amplicon's tables uploaded once,
// chunks of one amplicon each pipelined as in nw_align_ops.  Reads grouped by
// amplicon (ref_of_read non-decreasing, as the demultiplexed per-amplicon read sets
// arrive) are used in place; otherwise they are grouped on the host first and the
// outputs put back in the caller's order.
}  // extern "C"

namespace {

int multi_ops(nw_ctx* c, const char* refs, const int64_t* ref_offsets, int32_t n_refs, const char* reads,
              const int64_t* offsets, const int32_t* ref_of_read, int64_t n, uint32_t* ops_out, int64_t ops_cap,
              int64_t* ops_off, nw_stat* stats, const PackedInput* pk) {
    if (!c) return NW_E_INVALID;
    const Switches sw = read_switches();
    HostTimer ht(sw.host_timing, "index-scan tables");
    if (n_refs <= 0 || !refs || !ref_offsets) return fail(c, NW_E_INVALID, "no amplicons");
    if (n < 0 || (n > 0 && (!(reads || pk) || !offsets || !ref_of_read || !stats)) || !ops_off)
        return fail(c, NW_E_INVALID, "bad batch");
    std::vector<std::string> amps((size_t)n_refs);
    for (int32_t g = 0; g < n_refs; ++g) {
        const int64_t L = ref_offsets[g + 1] - ref_offsets[g];
        if (L <= 0 || L > kMaxRef) return fail(c, NW_E_UNSUPPORTED, "amplicon %d has length %lld", g, (long long)L);
        amps[(size_t)g].assign(refs + ref_offsets[g], refs + ref_offsets[g + 1]);
    }
    (void)hipSetDevice(c->device);
    // reads per amplicon and whether the reads come grouped: per part of the host pool
    // (memory-bound), a bad index located afterwards
    std::vector<int64_t> first((size_t)n_refs + 1, 0);
    bool grouped = true;
    {
        nw_host::Pool& pool = nw_host::Pool::get();
        const int parts = (int)std::min<int64_t>(pool.threads(), std::max<int64_t>(1, n >> 17));
        std::vector<std::vector<int64_t>> cnt((size_t)parts);
        std::vector<char> pbad((size_t)parts, 0), psorted((size_t)parts, 1);
        pool.run(parts, [&](int q) {
            int64_t lo, hi;
            nw_host::Pool::range(n, parts, q, &lo, &hi);
            std::vector<int64_t>& h = cnt[(size_t)q];
            h.assign((size_t)n_refs + 1, 0);
            uint32_t bad = 0, desc = 0;
            for (int64_t r = lo; r < hi; ++r) {
                const int32_t g = ref_of_read[r];
                const bool out = (uint32_t)g >= (uint32_t)n_refs;
                bad |= out;
                ++h[out ? (size_t)n_refs : (size_t)g];
                desc |= r > lo && g < ref_of_read[r - 1];
            }
            pbad[(size_t)q] = bad != 0;
            psorted[(size_t)q] = desc == 0 && (lo == 0 || hi == lo || ref_of_read[lo] >= ref_of_read[lo - 1]);
        });
        for (int q = 0; q < parts; ++q)
            if (pbad[(size_t)q])
                for (int64_t r = 0; r < n; ++r)
                    if ((uint32_t)ref_of_read[r] >= (uint32_t)n_refs)
                        return fail(c, NW_E_INVALID, "read %lld has amplicon index %d", (long long)r, ref_of_read[r]);
        for (int q = 0; q < parts; ++q) {
            grouped = grouped && psorted[(size_t)q];
            for (int32_t g = 0; g < n_refs; ++g) first[(size_t)g + 1] += cnt[(size_t)q][(size_t)g];
        }
    }
    for (int32_t g = 0; g < n_refs; ++g) first[(size_t)g + 1] += first[(size_t)g];
    ht.lap(0);
    int rc = upload_shared(c);
    std::vector<Profile> profs;
    if (!rc) rc = upload_profiles(c, amps, &profs);
    if (rc) return rc;
    ht.lap(1);
    c->ref.clear();   // the context has no single amplicon afterwards (nw_set_reference again)
    c->cur = Profile{};
    Groups grp{&amps, &profs, &first};
    if (grouped) {
        rc = ops_call(c, sw, reads, offsets, n, ops_out, ops_cap, ops_off, stats, true, &grp, pk);
        c->ref.clear();
        c->cur = Profile{};
        return rc;
    }
    if (pk) return fail(c, NW_E_INVALID, "packed pooled batches must be grouped by amplicon (ref_of_read ascending)");
    // group on the host (stable), align, then back to the caller's order
    std::vector<int64_t> order((size_t)n), fill(first.begin(), first.end() - 1);
    for (int64_t r = 0; r < n; ++r) order[(size_t)fill[(size_t)ref_of_read[r]]++] = r;
    std::vector<int64_t> soff((size_t)n + 1, 0);
    for (int64_t s2 = 0; s2 < n; ++s2)
        soff[(size_t)s2 + 1] = soff[(size_t)s2] + (offsets[order[(size_t)s2] + 1] - offsets[order[(size_t)s2]]);
    std::vector<char> sreads((size_t)std::max<int64_t>(soff[(size_t)n], 1));
    for (int64_t s2 = 0; s2 < n; ++s2) {
        const int64_t r = order[(size_t)s2];
        std::memcpy(sreads.data() + soff[(size_t)s2], reads + offsets[r], (size_t)(offsets[r + 1] - offsets[r]));
    }
    std::vector<nw::Stat> sst((size_t)std::max<int64_t>(n, 1));
    std::vector<int64_t> sopo((size_t)n + 1);
    std::vector<uint32_t> sops((size_t)std::max<int64_t>(ops_out ? std::max<int64_t>(ops_cap, 0) : 0, 1));
    rc = ops_call(c, sw, sreads.data(), soff.data(), n, ops_out ? sops.data() : nullptr, ops_out ? ops_cap : 0,
                  sopo.data(), (nw_stat*)sst.data(), true, &grp);
    c->ref.clear();
    c->cur = Profile{};
    if (rc && rc != NW_E_CAPACITY) return rc;
    // caller order: records, run counts -> offsets, runs
    std::vector<int64_t> cnt((size_t)n);
    for (int64_t s2 = 0; s2 < n; ++s2) {
        const int64_t r = order[(size_t)s2];
        std::memcpy(&stats[r], &sst[(size_t)s2], sizeof(nw::Stat));
        cnt[(size_t)r] = sopo[(size_t)s2 + 1] - sopo[(size_t)s2];
    }
    ops_off[0] = 0;
    for (int64_t r = 0; r < n; ++r) ops_off[r + 1] = ops_off[r] + cnt[(size_t)r];
    if (rc == NW_E_CAPACITY) return rc;
    if (ops_out)
        for (int64_t s2 = 0; s2 < n; ++s2) {
            const int64_t r = order[(size_t)s2];
            std::memcpy(ops_out + ops_off[r], sops.data() + sopo[(size_t)s2], sizeof(uint32_t) * (size_t)cnt[(size_t)r]);
        }
    return NW_OK;
}

}  // namespace

extern "C" {

int nw_align_multi_ops(nw_ctx* c, const char* refs, const int64_t* ref_offsets, int32_t n_refs, const char* reads,
                       const int64_t* offsets, const int32_t* ref_of_read, int64_t n, uint32_t* ops_out, int64_t ops_cap,
                       int64_t* ops_off, nw_stat* stats) {
    return multi_ops(c, refs, ref_offsets, n_refs, reads, offsets, ref_of_read, n, ops_out, ops_cap, ops_off, stats,
                     nullptr);
}

int nw_align_multi_ops_packed(nw_ctx* c, const char* refs, const int64_t* ref_offsets, int32_t n_refs,
                              const uint8_t* packed, const int64_t* offsets, const int32_t* ref_of_read, int64_t n,
                              const int64_t* exc_pos, const uint8_t* exc_byte, int64_t n_exc, uint32_t* ops_out,
                              int64_t ops_cap, int64_t* ops_off, nw_stat* stats) {
    if (!c) return NW_E_INVALID;
    if (n_exc < 0 || (n > 0 && !packed)) return fail(c, NW_E_INVALID, "bad packed batch");
    const PackedInput pk{packed, exc_pos, exc_byte, n_exc};
    return multi_ops(c, refs, ref_offsets, n_refs, nullptr, offsets, ref_of_read, n, ops_out, ops_cap, ops_off, stats,
                     &pk);
}

int nw_align_multi_ops_packed_lens(nw_ctx* c, const char* refs, const int64_t* ref_offsets, int32_t n_refs,
                                   const uint8_t* packed, const int64_t* offsets, const uint16_t* lens,
                                   const int32_t* ref_of_read, int64_t n, const int64_t* exc_pos, const uint8_t* exc_byte,
                                   int64_t n_exc, uint32_t* ops_out, int64_t ops_cap, int64_t* ops_off, nw_stat* stats) {
    if (!c) return NW_E_INVALID;
    if (n_exc < 0 || (n > 0 && (!packed || !lens))) return fail(c, NW_E_INVALID, "bad packed batch");
    const PackedInput pk{packed, exc_pos, exc_byte, n_exc, lens};
    return multi_ops(c, refs, ref_offsets, n_refs, nullptr, offsets, ref_of_read, n, ops_out, ops_cap, ops_off, stats,
                     &pk);
}

int nw_align_dual_ops_packed_lens(nw_ctx* c, const char* ref2, int32_t ref2_len, const uint8_t* packed,
                                  const int64_t* offsets, const uint16_t* lens, int64_t n, const int64_t* exc_pos,
                                  const uint8_t* exc_byte, int64_t n_exc, uint32_t* ops_out, int64_t ops_cap,
                                  int64_t* ops_off, nw_stat* stats, uint32_t* ops_out2, int64_t ops_cap2,
                                  int64_t* ops_off2, nw_stat* stats2) {
    if (!c) return NW_E_INVALID;
    if (c->ref.empty()) return fail(c, NW_E_STATE, "nw_set_reference must come first");
    if (!ref2 || ref2_len <= 0) return fail(c, NW_E_INVALID, "empty second amplicon");
    if (ref2_len > kMaxRef) return fail(c, NW_E_UNSUPPORTED, "amplicon length %d exceeds %d", ref2_len, kMaxRef);
    if (n_exc < 0 || (n > 0 && (!packed || !lens || !stats2 || !ops_off2))) return fail(c, NW_E_INVALID, "bad packed batch");
    (void)hipSetDevice(c->device);
    const PackedInput pk{packed, exc_pos, exc_byte, n_exc, lens};
    const std::string ref0 = c->ref;
    std::vector<std::string> amps{ref0, std::string(ref2, ref2 + ref2_len)};
    std::vector<Profile> profs;
    int rc = upload_shared(c);
    if (!rc) rc = upload_profiles(c, amps, &profs);
    if (rc) return rc;
    const std::vector<int64_t> first{0, n, 2 * n};
    Groups grp{&amps, &profs, &first};
    const Dual d{ops_out2, ops_cap2, ops_off2, stats2};
    rc = ops_call(c, read_switches(), nullptr, offsets, n, ops_out, ops_cap, ops_off, stats, true, &grp, &pk, &d);
    c->ref = ref0;   // the context keeps its amplicon (the arena holds both tables)
    c->cur = profs[0];
    return rc;
}

int nw_ops_times(const nw_ctx* c, float* h2d_ms, float* compute_ms, int64_t* h2d_bytes, int64_t* d2h_bytes) {
    if (!c) return NW_E_INVALID;
    if (h2d_ms) *h2d_ms = c->ops_h2d_ms;
    if (compute_ms) *compute_ms = c->ops_compute_ms;
    if (h2d_bytes) *h2d_bytes = c->ops_h2d_bytes;
    if (d2h_bytes) *d2h_bytes = c->ops_d2h_bytes;
    return NW_OK;
}

int nw_host_threads(void) { return nw_host::Pool::get().threads(); }

int nw_set_known(nw_ctx* c, const char* seq, int32_t len) {
    if (!c || len < 0 || (len > 0 && !seq)) return NW_E_INVALID;
    c->known_seq.assign(seq ? seq : "", (size_t)len);
    return NW_OK;
}

int nw_batch_set_phase_events(nw_ctx* c, int on) {
    if (!c) return NW_E_INVALID;
    c->phase_events = on != 0;
    return NW_OK;
}

int nw_batch_set_lane_walk(nw_ctx* c, int on) {
    if (!c) return NW_E_INVALID;
    c->lane_walk = on != 0;
    return NW_OK;
}

int nw_host_alloc(int64_t bytes, void** out) {
    if (!out || bytes < 0) return NW_E_INVALID;
    *out = nullptr;
    return hipHostMalloc(out, (size_t)std::max<int64_t>(bytes, 1), hipHostMallocDefault) == hipSuccess ? NW_OK
                                                                                                     : NW_E_NOMEM;
}

void nw_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int nw_host_register(void* p, int64_t bytes) {
    if (!p || bytes <= 0) return NW_E_INVALID;
    return hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault) == hipSuccess ? NW_OK : NW_E_HIP;
}

int nw_host_unregister(void* p) {
    if (!p) return NW_E_INVALID;
    return hipHostUnregister(p) == hipSuccess ? NW_OK : NW_E_HIP;
}

int nw_batch_phase_times(nw_ctx* c, float* ms5) {
    if (!c || !ms5) return NW_E_INVALID;
    if (!c->ran) return fail(c, NW_E_STATE, "nothing has run");
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 5; ++k) ms5[k] = 0.0f;
    if (!c->phases_recorded) return fail(c, NW_E_STATE, "the last run recorded no phase events (nw_batch_set_phase_events)");
    if (!c->ac.use_diag || c->n <= 0) {
        HIP_TRY(c, hipEventElapsedTime(&ms5[4], c->ev0, c->ev1));
        return NW_OK;
    }
    const bool two = c->ac.diag16_fill.grid > 0;
    HIP_TRY(c, hipEventElapsedTime(&ms5[0], c->ev0, c->ev_sort));
    HIP_TRY(c, hipEventElapsedTime(&ms5[1], c->ev_sort, c->ev_fill));
    HIP_TRY(c, hipEventElapsedTime(&ms5[2], c->ev_fill, c->ev_walk));
    HIP_TRY(c, hipEventElapsedTime(&ms5[3], c->ev_walk, c->ev_l2));
    HIP_TRY(c, hipEventElapsedTime(&ms5[4], c->ev_l2, c->ev1));
    if (!two) {   // one level: ms5[1..2] are the 32-diagonal level's, ms5[3] is empty
        ms5[3] = 0.0f;
    }
    return NW_OK;
}

int nw_batch_path_counts(nw_ctx* c, int64_t* counts4) {
    if (!c || !counts4) return NW_E_INVALID;
    if (c->call_done) {
        for (int k = 0; k < 4; ++k) counts4[k] = c->call_counts[k];
        return NW_OK;
    }
    if (!c->ran) return fail(c, NW_E_STATE, "nothing has run");
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 4; ++k) counts4[k] = 0;
    if (!c->ac.use_diag) {
        counts4[3] = nw_batch_fallbacks(c);
        return NW_OK;
    }
    int32_t fb[nw::kChunkCounters] = {}, need = 0;
    HIP_TRY(c, hipMemcpy(fb, c->sc[0].d_fallback_count.p, sizeof fb, hipMemcpyDeviceToHost));
    need = fb[nw::kCntDp];
    const bool two = c->ac.diag16_fill.grid > 0;
    counts4[0] = c->n - need;             // exact copies (no DP)
    counts4[1] = two ? need : 0;          // first level (16 diagonals)
    // a skipped second level (KernelArgs::redo_direct) sent its reads to the exact kernel
    const bool direct = two && c->last_launch.redo_direct > 0 && fb[nw::kCntRedo] <= c->last_launch.redo_direct;
    counts4[2] = two ? (direct ? 0 : fb[nw::kCntRedo]) : need;   // second level (32 diagonals)
    // the 16 / 32 levels' give-ups and the wide-first launch's reads (wide level + exact kernel)
    counts4[3] = fb[nw::kCntExact] + (direct ? fb[nw::kCntRedo] : 0) + fb[nw::kCntWfTaken];
    return NW_OK;
}

int64_t nw_batch_wide_first_reads(nw_ctx* c) {
    if (c && c->call_done) return c->call_wide_first;
    if (!c || !c->ran) return -1;
    if (!c->ac.use_diag) return 0;
    int32_t fb[nw::kChunkCounters];
    return run_counts(c, fb) ? fb[nw::kCntWfTaken] : -1;
}

int64_t nw_batch_exact_reads(nw_ctx* c) {
    if (c && c->call_done) return c->call_exact;
    if (!c || !c->ran) return -1;
    if (!c->ac.use_diag || c->ac.wide_fill.grid <= 0) return nw_batch_fallbacks(c);
    int32_t fb[nw::kChunkCounters];
    return run_counts(c, fb) ? fb[nw::kCntWideGiveUp] : -1;
}

}  // extern "C"
