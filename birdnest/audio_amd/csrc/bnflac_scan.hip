/*
 * bnflac_scan.hip -- k_scan_streams: the metadata of every stream of a batch, read where the
 * streams lie.  The first link of the batched chain: it fills the two words of each
 * bnflac_stream_desc that bnflac_index_streams needs (first_offset, total_samples) and the
 * STREAMINFO sums bnflac_md5_streams compares against, all in device memory.
 *
 * The walk (bnf_metadata.h) is a chain of dependent steps per stream, a few bytes each, so the
 * only parallelism is across streams: one lane owns one stream, 64-thread workgroups (one wave),
 * a grid of ceil(nstreams / 64), as k_md5_streams.  A typical stream (marker, STREAMINFO, a few
 * more blocks) is 3 + blocks round trips to memory; nothing else in the kernel takes time.  The
 * loads are plain byte loads at their own addresses: begin needs no alignment and no byte
 * outside [begin, end) is touched.  No LDS, no tables.  A wave counts its streams by kind with
 * ballots and its first lane adds the counts to the status words: at most four atomics per wave.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bnf_metadata.h"
#include "bnflac_launch.h"

#define SCAN_LANES 64

__global__ __launch_bounds__(SCAN_LANES) void k_scan_streams(const uint8_t *__restrict__ bytes, uint64_t nbytes,
                                                             bnf_stream_desc *sd, uint32_t nstreams,
                                                             bnf_stream_params expect, uint32_t has_expect,
                                                             bnf_stream_meta *__restrict__ meta, uint8_t *__restrict__ md5,
                                                             uint32_t *__restrict__ status) {
    const uint32_t s = blockIdx.x * SCAN_LANES + threadIdx.x;
    const bool live = s < nstreams;
    uint32_t kind = BNF_SCAN_KEPT;
    bool bad = false;
    if (live) {
        const uint64_t begin = sd[s].begin, end = sd[s].end;
        const uint64_t prev_end = s ? sd[s - 1].end : 0; /* begin and end are never written: no race with lane s - 1 */
        bad = begin > end || end > nbytes || begin < prev_end;
        bnf_stream_meta m;
        uint64_t first, total;
        uint32_t sum[4];
        kind = bnf_metadata_scan(bnf_bytes{bytes + (bad ? 0 : begin)}, begin, end, bad, has_expect ? &expect : nullptr, m,
                                 first, total, sum);
        sd[s].first_offset = first;
        sd[s].total_samples = total;
        if (meta) meta[s] = m;
        if (md5) {
#pragma unroll
            for (int i = 0; i < 16; i++) md5[16ull * s + i] = (uint8_t)(sum[i >> 2] >> (8 * (i & 3)));
        }
    }
    /* [0] bit 0 some stream not OK, bit 1 some stream differs, bit 2 some BAD_RANGE; [1] kept, [2] not OK, [3] differing */
    const uint32_t kept = (uint32_t)__popcll(__ballot(live && kind == BNF_SCAN_KEPT));
    const uint32_t failed = (uint32_t)__popcll(__ballot(live && kind == BNF_SCAN_FAILED));
    const uint32_t differ = (uint32_t)__popcll(__ballot(live && kind == BNF_SCAN_DIFFERENT));
    const bool any_bad = __ballot(live && bad) != 0;
    if (threadIdx.x == 0) {
        const uint32_t bits = (failed ? 1u : 0u) | (differ ? 2u : 0u) | (any_bad ? 4u : 0u);
        if (bits) atomicOr(&status[0], bits);
        if (kept) atomicAdd(&status[1], kept);
        if (failed) atomicAdd(&status[2], failed);
        if (differ) atomicAdd(&status[3], differ);
    }
}

extern "C" hipError_t bnf_launch_scan_streams(const uint8_t *bytes, uint64_t nbytes, bnf_stream_desc *sd, uint32_t nstreams,
                                              const bnf_stream_params *expect, bnf_stream_meta *meta, uint8_t *md5,
                                              uint32_t *status, hipStream_t s) {
    hipError_t e = hipMemsetAsync(status, 0, 4 * sizeof(uint32_t), s);
    if (e != hipSuccess || !nstreams) return e;
    bnf_stream_params x = {};
    if (expect) x = *expect;
    const dim3 grid((nstreams + SCAN_LANES - 1) / SCAN_LANES), block(SCAN_LANES);
    hipLaunchKernelGGL(k_scan_streams, grid, block, 0, s, bytes, nbytes, sd, nstreams, x, expect ? 1u : 0u, meta, md5, status);
    return hipGetLastError();
}
