/*
 * out_range_table.cpp -- the verdicts of csrc/bnf_out_range.h, the rule that keeps a decoded
 * frame inside the caller's output, as a stand-alone program (tests/test_out_placement_host.py
 * builds it with UBSan and compares every verdict with the rule in unbounded integers).
 *
 * stdin: one row per line, four unsigned decimal numbers: out_sample blocksize stride out_bytes.
 * stdout: per row "limit verdict", verdict 1 when the frame lies inside the output, then
 * "out_range_table: N rows".  A line that is not four numbers ends the program with status 2.
 *
 *   c++ -std=c++17 -g -fsanitize=undefined -fno-sanitize-recover=all \
 *       -I birdnest/audio_amd/csrc tools/out_range_table.cpp -o out_range_table
 */
#include <cinttypes>
#include <cstdint>
#include <cstdio>

#include "bnf_out_range.h"

int main() {
    char line[256];
    unsigned long long rows = 0;
    while (fgets(line, sizeof line, stdin)) {
        uint64_t p, bs, stride, out_bytes;
        if (sscanf(line, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &p, &bs, &stride, &out_bytes) != 4 ||
            bs > 0xffffffffull) {
            fprintf(stderr, "out_range_table: bad row %llu: %s", rows, line);
            return 2;
        }
        const uint64_t limit = bnf_out_limit(out_bytes, stride);
        printf("%" PRIu64 " %d\n", limit, bnf_out_in_range(p, (uint32_t)bs, limit) ? 1 : 0);
        rows++;
    }
    printf("out_range_table: %llu rows\n", rows);
    return 0;
}
