// nw_bam.cpp -- the BAM reader of include/crispr_regions.h (host only, no GPU call): BGZF blocks
// inflated in parallel (zlib, host_pool.h), the header parsed, every record indexed and
// validated.  What passes here may be trusted by the kernels of nw_regions.hip: a record's fixed
// fields, name, CIGAR, sequence and qualities all lie inside its block, and the block inside
// the stream.
#include <zlib.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/crispr_nw.h"
#include "../../include/crispr_regions.h"
#include "host_pool.h"
#include "nw_bam.h"

namespace {

int fail(char* err, int64_t cap, int code, const char* fmt, ...) {
    if (err && cap > 0) {
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(err, (size_t)cap, fmt, ap);
        va_end(ap);
    }
    return code;
}

inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

struct Block {
    size_t in, clen;      // the deflate bytes
    size_t out;           // where the block's bytes go
    uint32_t isize, crc;
};

// The BGZF blocks of [p, p + n): every block whole, with its BC field.
int scan_blocks(const uint8_t* p, size_t n, std::vector<Block>* blocks, size_t* total, char* err, int64_t cap) {
    size_t at = 0, out = 0;
    while (at < n) {
        const long long k = (long long)blocks->size();
        if (n - at < 18) return fail(err, cap, NW_E_INVALID, "BGZF block %lld is truncated (header)", k);
        const uint8_t* h = p + at;
        if (h[0] != 31 || h[1] != 139 || h[2] != 8) return fail(err, cap, NW_E_INVALID, "BGZF block %lld: bad gzip magic", k);
        if (h[3] != 4) return fail(err, cap, NW_E_INVALID, "BGZF block %lld: gzip flags %d, not a BGZF block", k, (int)h[3]);
        const size_t xlen = le16(h + 10);
        if (n - at < 12 + xlen) return fail(err, cap, NW_E_INVALID, "BGZF block %lld is truncated (extra field)", k);
        size_t bsize = 0;
        for (size_t x = 0; x + 4 <= xlen;) {
            const uint8_t* s = h + 12 + x;
            const size_t slen = le16(s + 2);
            if (x + 4 + slen > xlen) break;
            if (s[0] == 'B' && s[1] == 'C' && slen == 2) bsize = (size_t)le16(s + 4) + 1;
            x += 4 + slen;
        }
        if (bsize == 0) return fail(err, cap, NW_E_INVALID, "BGZF block %lld has no BC field", k);
        if (bsize < 12 + xlen + 8) return fail(err, cap, NW_E_INVALID, "BGZF block %lld: size %zu is too small", k, bsize);
        if (n - at < bsize) return fail(err, cap, NW_E_INVALID, "BGZF block %lld is truncated (%zu of %zu bytes)", k, n - at, bsize);
        Block b;
        b.in = at + 12 + xlen;
        b.clen = bsize - 12 - xlen - 8;
        b.out = out;
        b.crc = le32(h + bsize - 8);
        b.isize = le32(h + bsize - 4);
        if (b.isize > 65536) return fail(err, cap, NW_E_INVALID, "BGZF block %lld: %u bytes, more than 64 KiB", k, b.isize);
        blocks->push_back(b);
        out += b.isize;
        at += bsize;
    }
    *total = out;
    return NW_OK;
}

int inflate_blocks(const uint8_t* p, const std::vector<Block>& blocks, uint8_t* out, char* err, int64_t cap) {
    const int64_t nb = (int64_t)blocks.size();
    std::atomic<int64_t> bad{-1};
    std::atomic<int> why{0};
    nw_host::Pool& pool = nw_host::Pool::get();
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(pool.threads(), nb / 16));
    pool.run(parts, [&](int q) {
        int64_t lo, hi;
        nw_host::Pool::range(nb, parts, q, &lo, &hi);
        z_stream z;
        std::memset(&z, 0, sizeof z);
        if (inflateInit2(&z, -15) != Z_OK) {
            bad = lo;
            why = 3;
            return;
        }
        for (int64_t k = lo; k < hi && bad.load(std::memory_order_relaxed) < 0; ++k) {
            const Block& b = blocks[(size_t)k];
            uint8_t dummy = 0;
            inflateReset(&z);
            z.next_in = const_cast<Bytef*>(p + b.in);
            z.avail_in = (uInt)b.clen;
            z.next_out = b.isize ? out + b.out : &dummy;
            z.avail_out = b.isize ? b.isize : 1;      // (an empty block still needs room to end in)
            const int rc = inflate(&z, Z_FINISH);
            int w = 0;
            if (rc != Z_STREAM_END || z.total_out != b.isize) w = 1;
            else if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), out + b.out, b.isize) != b.crc) w = 2;
            if (w) {
                bad = k;
                why = w;
            }
        }
        inflateEnd(&z);
    });
    if (bad >= 0) {
        const char* what = why == 1 ? "the deflate data does not give the block's size" : why == 2 ? "CRC-32 mismatch" : "zlib failed";
        return fail(err, cap, NW_E_INVALID, "BGZF block %lld: %s", (long long)bad.load(), what);
    }
    return NW_OK;
}

int parse(nwr_bam* b, char* err, int64_t cap) {
    const uint8_t* d = b->data.data();
    const int64_t n = (int64_t)b->data.size();
    if (n < 12 || std::memcmp(d, "BAM\1", 4) != 0) return fail(err, cap, NW_E_INVALID, "bad BAM magic");
    int64_t at = 4;
    const int64_t l_text = (int32_t)le32(d + at);
    at += 4;
    if (l_text < 0 || l_text > n - at - 4) return fail(err, cap, NW_E_INVALID, "the header text (%lld bytes) passes the end", (long long)l_text);
    b->text.assign((const char*)d + at, (size_t)l_text);
    at += l_text;
    const int64_t n_ref = (int32_t)le32(d + at);
    at += 4;
    if (n_ref < 0) return fail(err, cap, NW_E_INVALID, "%lld references", (long long)n_ref);
    for (int64_t r = 0; r < n_ref; ++r) {
        if (n - at < 4) return fail(err, cap, NW_E_INVALID, "reference %lld passes the end", (long long)r);
        const int64_t l_name = (int32_t)le32(d + at);
        at += 4;
        if (l_name < 1 || l_name > n - at - 4) return fail(err, cap, NW_E_INVALID, "reference %lld: name of %lld bytes", (long long)r, (long long)l_name);
        const char* nm = (const char*)d + at;
        b->ref_names.append(nm, strnlen(nm, (size_t)l_name - 1));
        b->ref_names.push_back('\0');
        at += l_name;
        b->ref_len.push_back((int32_t)le32(d + at));
        at += 4;
    }
    while (at < n) {
        const long long k = (long long)b->off.size();
        if (n - at < 4) return fail(err, cap, NW_E_INVALID, "record %lld is truncated (%lld bytes left)", k, (long long)(n - at));
        const int64_t bs = (int32_t)le32(d + at);
        if (bs < 32) return fail(err, cap, NW_E_INVALID, "record %lld: block_size %lld", k, (long long)bs);
        if (bs > n - at - 4) return fail(err, cap, NW_E_INVALID, "record %lld passes the end (block_size %lld, %lld bytes left)", k, (long long)bs, (long long)(n - at - 4));
        const uint8_t* r = d + at;
        const int64_t ref_id = (int32_t)le32(r + nw_bam::kRefId), pos = (int32_t)le32(r + nw_bam::kPos);
        const int64_t l_name = r[nw_bam::kLReadName], n_op = le16(r + nw_bam::kNCigar), l_seq = (int32_t)le32(r + nw_bam::kLSeq);
        if (l_seq < 0) return fail(err, cap, NW_E_INVALID, "record %lld: l_seq %lld", k, (long long)l_seq);
        if (bs < 32 + l_name + 4 * n_op + (l_seq + 1) / 2 + l_seq)
            return fail(err, cap, NW_E_INVALID, "record %lld: block_size %lld is smaller than its fields", k, (long long)bs);
        if (ref_id < -1 || ref_id >= n_ref) return fail(err, cap, NW_E_INVALID, "record %lld: reference %lld of %lld", k, (long long)ref_id, (long long)n_ref);
        if (pos < -1) return fail(err, cap, NW_E_INVALID, "record %lld: pos %lld", k, (long long)pos);
        b->off.push_back(at);
        at += 4 + bs;
    }
    b->off.push_back(at);
    return NW_OK;
}

}  // namespace

extern "C" {

int nwr_read_bam(const char* path, const uint8_t* mem, int64_t mem_len, nwr_bam** out, char* err, int64_t err_cap) {
    if (!out) return NW_E_INVALID;
    *out = nullptr;
    if (err && err_cap > 0) err[0] = 0;
    std::vector<uint8_t> file;
    if (path) {
        FILE* f = std::fopen(path, "rb");
        if (!f) return fail(err, err_cap, NW_E_STATE, "cannot open %s", path);
        uint8_t buf[1 << 16];
        size_t got;
        while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + got);
        const bool bad = std::ferror(f) != 0;
        std::fclose(f);
        if (bad) return fail(err, err_cap, NW_E_STATE, "cannot read %s", path);
        mem = file.data();
        mem_len = (int64_t)file.size();
    }
    if (mem_len < 0 || (mem_len > 0 && !mem)) return fail(err, err_cap, NW_E_INVALID, "null input");
    nwr_bam* b = new nwr_bam();
    int rc = NW_OK;
    if (mem_len >= 2 && mem[0] == 31 && mem[1] == 139) {
        std::vector<Block> blocks;
        size_t total = 0;
        rc = scan_blocks(mem, (size_t)mem_len, &blocks, &total, err, err_cap);
        if (rc == NW_OK) {
            b->data.resize(total);
            rc = inflate_blocks(mem, blocks, b->data.data(), err, err_cap);
        }
    } else if (path) {
        b->data.swap(file);
    } else {
        b->data.assign(mem, mem + mem_len);
    }
    if (rc == NW_OK) rc = parse(b, err, err_cap);
    if (rc != NW_OK) {
        delete b;
        return rc;
    }
    *out = b;
    return NW_OK;
}

void nwr_bam_free(nwr_bam* b) { delete b; }

int64_t nwr_bam_count(const nwr_bam* b) { return b ? (int64_t)b->off.size() - 1 : 0; }

const uint8_t* nwr_bam_data(const nwr_bam* b, int64_t* nbytes) {
    if (nbytes) *nbytes = b ? (int64_t)b->data.size() : 0;
    return b ? b->data.data() : nullptr;
}

const int64_t* nwr_bam_offsets(const nwr_bam* b) { return b ? b->off.data() : nullptr; }

int32_t nwr_bam_n_ref(const nwr_bam* b) { return b ? (int32_t)b->ref_len.size() : 0; }

const char* nwr_bam_ref_names(const nwr_bam* b, int64_t* nbytes) {
    if (nbytes) *nbytes = b ? (int64_t)b->ref_names.size() : 0;
    return b ? b->ref_names.data() : nullptr;
}

const int32_t* nwr_bam_ref_lens(const nwr_bam* b) { return b ? b->ref_len.data() : nullptr; }

const char* nwr_bam_text(const nwr_bam* b, int64_t* nbytes) {
    if (nbytes) *nbytes = b ? (int64_t)b->text.size() : 0;
    return b ? b->text.data() : nullptr;
}

}  // extern "C"
