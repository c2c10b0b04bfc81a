// bam_check.cpp -- the BAM reader (nw_bam.cpp) as a stand-alone program, for host sanitizer
// builds (`make bam_check SAN=-fsanitize=address,undefined`): reads every file named on the
// command line and prints its record count, or the reader's error.  No GPU, no Python.
#include <cstdio>

#include "../../include/crispr_regions.h"

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        nwr_bam* b = nullptr;
        char err[256];
        const int rc = nwr_read_bam(argv[i], nullptr, 0, &b, err, sizeof err);
        if (rc != 0) {
            std::printf("%s\terror %d\t%s\n", argv[i], rc, err);
            continue;
        }
        int64_t nbytes = 0, sum = 0;
        const uint8_t* d = nwr_bam_data(b, &nbytes);
        const int64_t* off = nwr_bam_offsets(b);
        for (int64_t r = 0; r < nwr_bam_count(b); ++r)      // touch every record's bytes
            for (int64_t k = off[r]; k < off[r + 1]; ++k) sum += d[k];
        std::printf("%s\tok\t%lld records\t%d references\t%lld bytes\tsum %lld\n", argv[i], (long long)nwr_bam_count(b),
                    (int)nwr_bam_n_ref(b), (long long)nbytes, (long long)sum);
        nwr_bam_free(b);
    }
    return 0;
}
