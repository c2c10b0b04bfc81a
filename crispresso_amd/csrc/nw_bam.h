// nw_bam.h -- a BAM held in host memory, validated (nw_bam.cpp); what nw_regions.hip uploads.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

// BAM's record layout from the block_size field on (SAM specification, section 4.2).
namespace nw_bam {
constexpr int kRefId = 4, kPos = 8, kLReadName = 12, kNCigar = 16, kFlag = 18, kLSeq = 20, kName = 36;
}

struct nwr_bam {
    std::vector<uint8_t> data;       // the uncompressed stream
    std::vector<int64_t> off;        // [count + 1] record starts (the block_size field), then the end
    std::vector<int32_t> ref_len;
    std::string ref_names;           // each name ended by a NUL
    std::string text;
};
