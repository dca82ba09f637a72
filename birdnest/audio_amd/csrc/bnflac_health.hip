/*
 * bnflac_health.hip -- which windows of a decoded selection hold damaged or missing audio:
 * k_hl_prefix / k_hl_scan / k_hl_windows (bnflac_window_health).  No CRC tables, no g_stats, no
 * ablate word.
 *
 * The rule is bnf_health.h's.  A window's run of records is [first, first + nframes) of the
 * selection; no loop walks it.  Prefixes over the record positions, then one lane per window, as
 * k_shr_rank / k_shr_windows do for the shared selection; launch boundaries are the only ordering
 * between workgroups (no workgroup waits on another):
 *   k_hl_prefix   one lane per position of [0, sel_cap), 1,024 per workgroup: status, crc_ok and
 *                 blocksize of the record (three dword loads), its terms (bad | crc << 32, blocksize,
 *                 bad ? blocksize : 0), their exclusive scan inside the workgroup (wave64 shuffle scan,
 *                 then the 16 wave sums through LDS).  Writes the three prefixes per position and the
 *                 workgroup's sums.
 *   k_hl_scan     one workgroup: the exclusive scan of the workgroup sums, in place, sel_cap / 2^20
 *                 rounds; entry nwg gets the totals, which are the prefixes at sel_cap.
 *   k_hl_windows  one lane per window: the prefixes at the clamped run ends and next to them (at most
 *                 four positions, each a workgroup base plus a position entry), the request rule, the
 *                 32-byte record.  Three ballots and integer atomics per wave give the status words.
 * Grids, loop bounds and the scratch depend on sel_cap and nwindows only.  A position is read only
 * below sel_cap, a window, first or request entry only below nwindows, a stream entry only for a
 * stream id below nstreams.  Atomics are integer adds and ors: no result depends on their order.
 * Scratch: 24 bytes per position of [0, sel_cap) and 24 per 1,024 positions plus 24.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bnf_health.h"
#include "bnflac_launch.h"

#define HL_BLOCK 1024
#define HL_WAVES (HL_BLOCK / 64)
#define HL_WIN_THREADS 256

static_assert(sizeof(bnf_window_health) == 32 && sizeof(bnf_health_sums) == 24, "record sizes");
static_assert(sizeof(bnf_frame_info) == 128 && sizeof(bnf_window) == 32 && sizeof(bnf_window_request) == 24 &&
                  sizeof(bnf_stream_desc) == 32,
              "table record sizes");

/* Exclusive scan of v over the workgroup's HL_BLOCK lanes -> e; t: the workgroup's sums. */
__device__ __forceinline__ void hl_block_scan(const bnf_health_sums &v, bnf_health_sums &e, bnf_health_sums &t) {
    __shared__ uint64_t wsum[3][HL_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t c0 = v.counts, c1 = v.all, c2 = v.bad;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t u0 = __shfl_up(c0, d), u1 = __shfl_up(c1, d), u2 = __shfl_up(c2, d);
        if (lane >= d) {
            c0 += u0;
            c1 += u1;
            c2 += u2;
        }
    }
    __syncthreads(); /* a second scan by the same workgroup: the sums of the first one are read */
    if (lane == 63u) {
        wsum[0][wave] = c0;
        wsum[1][wave] = c1;
        wsum[2][wave] = c2;
    }
    __syncthreads();
    /* every wave scans the 16 wave sums itself, in each of its four groups of 16 lanes: three LDS reads per
     * lane and four shuffle steps instead of 48 reads, and the registers they would hold */
    const uint32_t g = lane & (HL_WAVES - 1u);
    uint64_t s0 = wsum[0][g], s1 = wsum[1][g], s2 = wsum[2][g];
#pragma unroll
    for (uint32_t d = 1; d < HL_WAVES; d <<= 1) {
        const uint64_t u0 = __shfl_up(s0, d, HL_WAVES), u1 = __shfl_up(s1, d, HL_WAVES), u2 = __shfl_up(s2, d, HL_WAVES);
        if (g >= d) {
            s0 += u0;
            s1 += u1;
            s2 += u2;
        }
    }
    t.counts = __shfl(s0, HL_WAVES - 1, HL_WAVES);
    t.all = __shfl(s1, HL_WAVES - 1, HL_WAVES);
    t.bad = __shfl(s2, HL_WAVES - 1, HL_WAVES);
    const uint32_t prev = (wave + HL_WAVES - 1u) & (HL_WAVES - 1u); /* the waves below this one end there */
    const uint64_t b0 = __shfl(s0, prev, HL_WAVES), b1 = __shfl(s1, prev, HL_WAVES), b2 = __shfl(s2, prev, HL_WAVES);
    e.counts = (wave ? b0 : 0u) + c0 - v.counts;
    e.all = (wave ? b1 : 0u) + c1 - v.all;
    e.bad = (wave ? b2 : 0u) + c2 - v.bad;
}

/* rel: each position's prefix inside its workgroup; wg: the workgroup sums (nwg + 1 entries, the last one
 * written by k_hl_scan). */
__global__ __launch_bounds__(HL_BLOCK) void k_hl_prefix(const bnf_frame_info *__restrict__ info, uint32_t sel_cap,
                                                        bnf_health_sums *__restrict__ rel, bnf_health_sums *__restrict__ wg) {
    const uint32_t p = blockIdx.x * HL_BLOCK + threadIdx.x;
    bnf_health_sums v = {0, 0, 0};
    if (p < sel_cap) v = bnf_health_terms(info[p].status, info[p].crc_ok, info[p].blocksize);
    bnf_health_sums e, t;
    hl_block_scan(v, e, t);
    if (p < sel_cap) rel[p] = e;
    if (threadIdx.x == 0) wg[blockIdx.x] = t;
}

/* One workgroup: the workgroup sums become their exclusive prefixes, entry nwg the totals. */
__global__ __launch_bounds__(HL_BLOCK) void k_hl_scan(bnf_health_sums *__restrict__ wg, uint32_t nwg) {
    bnf_health_sums carry = {0, 0, 0};
    for (uint32_t base = 0; base < nwg; base += HL_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        bnf_health_sums v = {0, 0, 0};
        if (i < nwg) v = wg[i];
        bnf_health_sums e, t;
        hl_block_scan(v, e, t);
        if (i < nwg) {
            e.counts += carry.counts;
            e.all += carry.all;
            e.bad += carry.bad;
            wg[i] = e;
        }
        carry.counts += t.counts;
        carry.all += t.all;
        carry.bad += t.bad;
    }
    if (threadIdx.x == 0) wg[nwg] = carry;
}

/* P(p) for p in [0, sel_cap]: the workgroup's base plus the position's entry, or the totals at sel_cap. */
struct hl_prefix {
    const bnf_health_sums *rel, *wg;
    uint32_t sel_cap, nwg;
    __host__ __device__ __forceinline__ bnf_health_sums operator()(uint32_t p) const {
        if (p >= sel_cap) return wg[nwg];
        bnf_health_sums a = wg[p / HL_BLOCK];
        const bnf_health_sums b = rel[p];
        a.counts += b.counts;
        a.all += b.all;
        a.bad += b.bad;
        return a;
    }
};

__global__ __launch_bounds__(HL_WIN_THREADS) void k_hl_windows(const bnf_health_sums *__restrict__ rel,
                                                               const bnf_health_sums *__restrict__ wg, uint32_t sel_cap,
                                                               uint32_t nwg, const bnf_window *__restrict__ windows,
                                                               const uint32_t *__restrict__ first, uint32_t nwindows,
                                                               const bnf_window_request *__restrict__ requests,
                                                               const bnf_stream_desc *__restrict__ streams,
                                                               const uint64_t *__restrict__ stream_samples, uint32_t nstreams,
                                                               bnf_window_health *__restrict__ health,
                                                               uint32_t *__restrict__ status) {
    const uint32_t w = blockIdx.x * HL_WIN_THREADS + threadIdx.x;
    uint32_t flags = 0;
    if (w < nwindows) {
        bnf_window_health h;
        hl_prefix prefix = {rel, wg, sel_cap, nwg};
        bnf_health_window(windows[w], first[w], sel_cap, prefix, h);
        if (requests) bnf_health_request(requests[w], streams, stream_samples, nstreams, h);
        health[w] = h;
        flags = h.flags;
    }
    const uint32_t damaged = (uint32_t)__popcll(__ballot(flags & BNF_HEALTH_DAMAGED));
    const uint32_t brief = (uint32_t)__popcll(__ballot(flags & BNF_HEALTH_SHORT));
    const uint32_t unknown = (uint32_t)__popcll(__ballot(flags & BNF_HEALTH_UNKNOWN));
    if ((threadIdx.x & 63u) == 0) {
        const uint32_t bits = (damaged ? BNF_HEALTH_DAMAGED : 0u) | (brief ? BNF_HEALTH_SHORT : 0u) |
                              (unknown ? BNF_HEALTH_UNKNOWN : 0u);
        if (bits) atomicOr(&status[0], bits);
        if (damaged) atomicAdd(&status[1], damaged);
        if (brief) atomicAdd(&status[2], brief);
        if (unknown) atomicAdd(&status[3], unknown);
    }
}

/* Scratch: the position prefixes, then the workgroup sums and the totals; 24 bytes per entry, the first
 * table rounded up to 16 bytes.  Without windows no position is looked at. */
static uint64_t hl_rel_bytes(uint32_t npos) { return (24u * (uint64_t)npos + 15u) & ~(uint64_t)15; }

extern "C" uint64_t bnf_window_health_scratch_bytes(uint32_t sel_cap, uint32_t nwindows) {
    const uint32_t npos = nwindows ? sel_cap : 0u;
    const uint64_t nwg = ((uint64_t)npos + HL_BLOCK - 1) / HL_BLOCK;
    return hl_rel_bytes(npos) + 24u * (nwg + 1);
}

extern "C" hipError_t bnf_launch_window_health(const bnf_frame_info *sel_info, uint32_t sel_cap, const bnf_window *windows,
                                               const uint32_t *first, uint32_t nwindows, const bnf_window_request *requests,
                                               const bnf_stream_desc *streams, const uint64_t *stream_samples,
                                               uint32_t nstreams, bnf_window_health *health, uint32_t *status, void *scratch,
                                               hipStream_t s) {
    hipError_t e = hipMemsetAsync(status, 0, 4 * sizeof(uint32_t), s);
    if (e != hipSuccess || !nwindows) return e;
    const uint32_t nwg = (uint32_t)(((uint64_t)sel_cap + HL_BLOCK - 1) / HL_BLOCK);
    bnf_health_sums *rel = (bnf_health_sums *)scratch;
    bnf_health_sums *wg = (bnf_health_sums *)((uint8_t *)scratch + hl_rel_bytes(sel_cap));
    if (nwg) hipLaunchKernelGGL(k_hl_prefix, dim3(nwg), dim3(HL_BLOCK), 0, s, sel_info, sel_cap, rel, wg);
    hipLaunchKernelGGL(k_hl_scan, dim3(1), dim3(HL_BLOCK), 0, s, wg, nwg);
    hipLaunchKernelGGL(k_hl_windows, dim3((nwindows + HL_WIN_THREADS - 1) / HL_WIN_THREADS), dim3(HL_WIN_THREADS), 0, s, rel,
                       wg, sel_cap, nwg, windows, first, nwindows, requests, streams, stream_samples, nstreams, health,
                       status);
    return hipGetLastError();
}
