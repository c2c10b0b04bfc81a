// What fastq_parse.hip (the ingest, include/crispr_ingest.h) and front_pack.hip (the front end,
// which reads the records where they lie) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/crispr_ingest.h"

// One parsed text.  Streams: 0 bases, 1 qualities, 2 names; stream[q] is padded by 16 readable
// bytes past bytes[q], off[q] has n + 1 entries from 0.  n == 0: no device array at all.
struct nwi_records {
    int device = 0;
    nwi_summary info{};
    uint8_t* stream[3] = {nullptr, nullptr, nullptr};
    int64_t* off[3] = {nullptr, nullptr, nullptr};
    uint8_t* flags = nullptr;
    std::vector<void*> bufs;
};

namespace nwi {

// the first reason among a record's flags, for a refusal's message
inline const char* flag_reason(int f) {
    if (f & NWI_BAD_HEADER) return "the header line is empty or does not start with '@'";
    if (f & NWI_BAD_PLUS) return "the third line is empty or does not start with '+'";
    if (f & NWI_LEN_MISMATCH) return "the sequence and its quality line differ in length";
    if (f & NWI_BAD_QUAL) return "a quality byte outside 33..126 (phred 33)";
    return "no flag";
}

}  // namespace nwi
