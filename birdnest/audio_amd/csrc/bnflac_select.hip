/*
 * bnflac_select.hip -- sample windows of a batch: k_sel_streams / k_sel_scan / k_sel_apply /
 * k_sel_emit (bnflac_select_ranges), k_win_select / k_win_scan / k_win_apply
 * (bnflac_select_windows) and k_shr_* (bnflac_select_windows_shared) cut the index of
 * bnflac_index_streams down to the frames the windows need, k_gather_ranges (bnflac_gather_ranges) copies the decoded windows into rows of
 * one shape.  No CRC tables, no g_stats, no ablate word.
 *
 * Selection.  The rule is bnf_select.h's.  Four launches, and launch boundaries are the only
 * ordering between workgroups (no workgroup waits on another, as in the batched indexer):
 *   k_sel_streams  one lane per stream, 1,024 streams per workgroup: the two binary searches, then
 *                  the workgroup's exclusive scan of (frames, hull samples).  Writes the prefixes
 *                  and the window records relative to the workgroup, and the workgroup's sums.
 *                  A lane whose slice of the tables descends or passes cap searches nothing and
 *                  raises the call's bad flag.
 *   k_sel_scan     one workgroup: the exclusive scan of the workgroup sums, the two totals and
 *                  the status words (zeros, empty and bit 1 when the bad flag is up).
 *   k_sel_apply    adds each workgroup's base to its prefixes and windows (or empties them).
 *   k_sel_emit     8 lanes per position of [0, sel_cap): the position's stream by binary search
 *                  over the frame prefixes, then the 128-byte record as 8 x 16 bytes, so a wave
 *                  moves eight whole records, each a full 128-byte line in and out; the lane that
 *                  holds out_sample (bytes 64..71) patches it.  Positions at or past the total get
 *                  the filler record.  Nothing at or past sel_cap is written.
 * Loop bounds: the searches of bnf_select.h run over index intervals, the emit's search over
 * [0, nstreams]; no trip count is a table value.  A source position is checked against cap.
 *
 * Selection per window request (bnflac_select_windows): the same four launches with one lane per
 * window, k_win_select / k_win_scan / k_win_apply and k_sel_emit itself.  A lane loads its request,
 * checks the stream it names against nstreams and reads that stream's four table entries; no grid,
 * loop bound or scratch size depends on nstreams.  Windows may share frames, so frame counts are
 * scanned in 64 bits: k_win_select leaves each window's prefix inside its workgroup in the scratch,
 * k_win_apply adds the workgroup's base and writes min(prefix, UINT32_MAX).  The emit compares a
 * position below sel_cap with prefix entries only, and a saturated entry is above every position.
 *
 * Shared selection (bnflac_select_windows_shared): the same requests, every frame selected once.  A
 * mark / scan / compact over the index positions [0, cap), launch boundaries again the only ordering:
 *   k_shr_mark     one lane per window: bnf_select_request, the window record with pcm_first = skip,
 *                  +1 / -1 into a difference array delta[cap + 1] (integer atomics), the ballots of
 *                  k_win_select and the highest position any run ends at (atomicMax).
 *   k_shr_cover    1,024 positions per workgroup: the running sum of delta inside the workgroup, in
 *                  place, and the workgroup's sum.
 *   k_shr_scan<0>  one workgroup: the exclusive scan of those sums.
 *   k_shr_rank     covered = base + running sum > 0; the workgroup's exclusive scan of (covered,
 *                  covered ? blocksize : 0) to rank / pos, the sums per workgroup.  d_info is read at
 *                  covered positions only.
 *   k_shr_scan<1>  one workgroup: the exclusive scan of those sums, the totals and the status words.
 *   k_shr_emit     8 lanes per position, as k_sel_emit: a covered position copies its record to its
 *                  rank (below sel_cap) with out_sample = pos; output positions at or past the total
 *                  get the filler.
 *   k_shr_windows  one lane per window: pcm_first += pos of its first frame, win_sel_first = its rank;
 *                  under the bad flag the emptied records.
 * Grids and loop bounds are cap, nwindows and sel_cap.  A position workgroup at or past the highest
 * marked position (clamped to cap) writes zero sums and leaves.  Scratch: 32 bytes, 16 per position
 * (delta 4, rank 4, pos 8) and 16 per 1,024 positions; nothing per window.
 *
 * Gather.  Row s = min(nsamples, row_samples) sample frames from pcm_first, then zeros up to
 * row_samples.  Source offset (pcm_first * stride) and destination offset (s * row_bytes) have
 * independent phases modulo 16, constant along a row.  A workgroup belongs to one row
 * (blockIdx.x) and walks chunks of 1,024 aligned 16-byte destination slots (blockIdx.y, grid
 * strided): each slot is one 16-byte store, built from the two aligned 16-byte source blocks its
 * bytes lie in, shifted together with v_alignbyte_b32 (the dword part of the shift is uniform
 * over the row and chosen once, outside the loop).  The slot the data ends in is masked, the
 * slots behind it are zero stores.  The up to 15 bytes in front of the first aligned slot and
 * behind the last one go out bytewise from the row's first workgroup.  Reads stay inside
 * [0, round_up(pcm_bytes, 16)): a block's address is never above the buffer's last block, and a
 * window that is not inside pcm_bytes is not read at all (zero row, counted).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bnf_select.h"
#include "bnflac_launch.h"

#define SEL_BLOCK 1024
#define SEL_WAVES (SEL_BLOCK / 64)

static_assert(sizeof(bnf_frame_info) == 128 && sizeof(bnf_window) == 32 && sizeof(bnf_sample_range) == 16, "record sizes");
static_assert(sizeof(bnf_window_request) == 24, "request size");

/* Exclusive scan of (f, s) over the workgroup's SEL_BLOCK lanes; tf / ts: the workgroup's sums.
 * F: uint32_t for frames per stream (bounded by cap), uint64_t for frames per window (not bounded). */
template <typename F>
__device__ __forceinline__ void sel_block_scan(F f, uint64_t s, F &ef, uint64_t &es, F &tf, uint64_t &ts) {
    __shared__ F wf[SEL_WAVES];
    __shared__ uint64_t ws[SEL_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    F cf = f;
    uint64_t cs = s;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const F uf = __shfl_up(cf, d);
        const uint64_t us = __shfl_up(cs, d);
        if (lane >= d) {
            cf += uf;
            cs += us;
        }
    }
    __syncthreads(); /* a second scan by the same workgroup: the sums of the first one are read */
    if (lane == 63u) {
        wf[wave] = cf;
        ws[wave] = cs;
    }
    __syncthreads();
    F bf = 0;
    uint64_t bs = 0;
    tf = 0;
    ts = 0;
#pragma unroll
    for (uint32_t w = 0; w < SEL_WAVES; w++) {
        if (w < wave) {
            bf += wf[w];
            bs += ws[w];
        }
        tf += wf[w];
        ts += ws[w];
    }
    ef = bf + cf - f;
    es = bs + cs - s;
}

/* ctl: [0] bad flag, [1] streams with a window, [2] streams clipped */
__global__ __launch_bounds__(SEL_BLOCK) void k_sel_streams(const bnf_frame_info *__restrict__ info, uint32_t cap,
                                                           const uint32_t *__restrict__ sf, const uint64_t *__restrict__ ss,
                                                           uint32_t nstreams, const bnf_sample_range *__restrict__ ranges,
                                                           uint32_t *__restrict__ sel_frames, uint64_t *__restrict__ sel_samples,
                                                           bnf_window *__restrict__ windows, uint32_t *__restrict__ ctl,
                                                           uint32_t *__restrict__ wg_frames, uint64_t *__restrict__ wg_samples) {
    const uint32_t s = blockIdx.x * SEL_BLOCK + threadIdx.x;
    const bool live = s < nstreams;
    bnf_sel_stream o;
    o.nsamples = o.hull = 0;
    o.skip = o.first_frame = o.nframes = 0;
    o.flags = BNF_WIN_EMPTY;
    bool bad = false;
    if (live) {
        const uint32_t f0 = sf[s], f1 = sf[s + 1];
        const uint64_t s0 = ss[s], s1 = ss[s + 1];
        bad = !bnf_select_tables_ok(f0, f1, s0, s1, cap);
        if (!bad) bnf_select_stream(info, f0, f1, s0, s1, ranges[s], o);
    }
    uint32_t ef, tf;
    uint64_t es, ts;
    sel_block_scan(o.nframes, o.hull, ef, es, tf, ts);
    if (live) {
        sel_frames[s] = ef;
        sel_samples[s] = es;
        windows[s] = bnf_select_window(o, es);
    }
    if (threadIdx.x == 0) {
        wg_frames[blockIdx.x] = tf;
        wg_samples[blockIdx.x] = ts;
    }
    const bool any_bad = __ballot(bad) != 0;
    const uint32_t nonempty = (uint32_t)__popcll(__ballot(live && !bad && !(o.flags & BNF_WIN_EMPTY)));
    const uint32_t clipped = (uint32_t)__popcll(__ballot(live && !bad && (o.flags & BNF_WIN_CLIPPED)));
    if ((threadIdx.x & 63u) == 0) {
        if (any_bad) atomicOr(&ctl[0], 1u);
        if (nonempty) atomicAdd(&ctl[1], nonempty);
        if (clipped) atomicAdd(&ctl[2], clipped);
    }
}

/* One workgroup: the workgroup sums become their exclusive prefixes; totals and status. */
__global__ __launch_bounds__(SEL_BLOCK) void k_sel_scan(uint32_t *__restrict__ wg_frames, uint64_t *__restrict__ wg_samples,
                                                        uint32_t nwg, uint32_t nstreams, uint32_t sel_cap,
                                                        const uint32_t *__restrict__ ctl, uint32_t *__restrict__ sel_frames,
                                                        uint64_t *__restrict__ sel_samples, uint32_t *__restrict__ status) {
    uint32_t carry_f = 0;
    uint64_t carry_s = 0;
    for (uint32_t base = 0; base < nwg; base += SEL_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t f = i < nwg ? wg_frames[i] : 0u;
        const uint64_t s = i < nwg ? wg_samples[i] : 0u;
        uint32_t ef, tf;
        uint64_t es, ts;
        sel_block_scan(f, s, ef, es, tf, ts);
        if (i < nwg) {
            wg_frames[i] = carry_f + ef;
            wg_samples[i] = carry_s + es;
        }
        carry_f += tf;
        carry_s += ts;
    }
    if (threadIdx.x == 0) {
        const bool bad = ctl[0] != 0;
        sel_frames[nstreams] = bad ? 0u : carry_f;
        sel_samples[nstreams] = bad ? 0u : carry_s;
        status[0] = bad ? BNF_SEL_BAD_TABLES : carry_f > sel_cap ? BNF_SEL_OVERFLOW : 0u;
        status[1] = bad ? 0u : carry_f;
        status[2] = bad ? 0u : ctl[1];
        status[3] = bad ? 0u : ctl[2];
    }
}

__global__ __launch_bounds__(SEL_BLOCK) void k_sel_apply(const uint32_t *__restrict__ sf, uint32_t nstreams,
                                                         const uint32_t *__restrict__ wg_frames,
                                                         const uint64_t *__restrict__ wg_samples, const uint32_t *__restrict__ ctl,
                                                         uint32_t *__restrict__ sel_frames, uint64_t *__restrict__ sel_samples,
                                                         bnf_window *__restrict__ windows) {
    const uint32_t s = blockIdx.x * SEL_BLOCK + threadIdx.x;
    if (s >= nstreams) return;
    if (ctl[0]) {
        sel_frames[s] = 0;
        sel_samples[s] = 0;
        windows[s] = bnf_select_no_window(sf[s]);
    } else if (blockIdx.x) {
        sel_frames[s] += wg_frames[blockIdx.x];
        sel_samples[s] += wg_samples[blockIdx.x];
        windows[s].pcm_first += wg_samples[blockIdx.x];
    }
}

#define EMIT_THREADS 256

__global__ __launch_bounds__(EMIT_THREADS) void k_sel_emit(const uint64_t *__restrict__ offsets,
                                                           const bnf_frame_info *__restrict__ info, uint32_t cap,
                                                           const uint32_t *__restrict__ sel_frames,
                                                           const uint64_t *__restrict__ sel_samples, uint32_t nstreams,
                                                           const bnf_window *__restrict__ windows, uint64_t *__restrict__ sel_offsets,
                                                           bnf_frame_info *__restrict__ sel_info, uint32_t sel_cap) {
    const uint64_t gid = (uint64_t)blockIdx.x * EMIT_THREADS + threadIdx.x;
    const uint64_t p64 = gid >> 3;
    const uint32_t part = (uint32_t)gid & 7u; /* bytes [16 part, 16 part + 16) of the record */
    if (p64 >= sel_cap) return;
    const uint32_t p = (uint32_t)p64;
    uint4 v = make_uint4(0u, 0u, 0u, 0u); /* the filler: zeros, status 3 (skipped), err -1 */
    if (part == 0) {
        v.x = BNF_ST_SKIPPED;
        v.y = 0xffffffffu;
    }
    uint64_t off = 0;
    if (p < sel_frames[nstreams]) {
        /* sel_frames[a] <= p < sel_frames[b] holds from (0, nstreams) on: sel_frames[0] is 0 */
        uint32_t a = 0, b = nstreams;
        while (b - a > 1u) {
            const uint32_t m = a + ((b - a) >> 1);
            if (sel_frames[m] <= p)
                a = m;
            else
                b = m;
        }
        const uint32_t first = windows[a].first_frame;
        const uint64_t src = (uint64_t)first + (p - sel_frames[a]);
        if (src < cap) {
            v = ((const uint4 *)(info + src))[part];
            if (part == 4) { /* out_sample: bytes 64..71 */
                const uint64_t os = ((uint64_t)v.y << 32 | v.x) - info[first].out_sample + sel_samples[a];
                v.x = (uint32_t)os;
                v.y = (uint32_t)(os >> 32);
            }
            if (part == 0 && offsets) off = offsets[src];
        }
    }
    ((uint4 *)(sel_info + p))[part] = v;
    if (part == 0 && sel_offsets) sel_offsets[p] = off;
}

extern "C" uint64_t bnf_select_scratch_bytes(uint32_t nstreams) {
    const uint64_t nwg = ((uint64_t)nstreams + SEL_BLOCK - 1) / SEL_BLOCK;
    return 16u + ((4u * nwg + 15u) & ~(uint64_t)15) + 8u * nwg;
}

extern "C" hipError_t bnf_launch_select_ranges(const uint64_t *offsets, const bnf_frame_info *info, uint32_t cap,
                                               const uint32_t *sf, const uint64_t *ss, uint32_t nstreams,
                                               const bnf_sample_range *ranges, uint64_t *sel_offsets, bnf_frame_info *sel_info,
                                               uint32_t sel_cap, uint32_t *sel_frames, uint64_t *sel_samples,
                                               bnf_window *windows, uint32_t *status, void *scratch, hipStream_t s) {
    const uint32_t nwg = (uint32_t)(((uint64_t)nstreams + SEL_BLOCK - 1) / SEL_BLOCK);
    uint32_t *ctl = (uint32_t *)scratch;
    uint32_t *wg_frames = ctl + 4;
    uint64_t *wg_samples = (uint64_t *)((uint8_t *)scratch + 16u + ((4u * (uint64_t)nwg + 15u) & ~(uint64_t)15));
    hipError_t e = hipMemsetAsync(ctl, 0, 16, s);
    if (e != hipSuccess) return e;
    if (nwg)
        hipLaunchKernelGGL(k_sel_streams, dim3(nwg), dim3(SEL_BLOCK), 0, s, info, cap, sf, ss, nstreams, ranges, sel_frames,
                           sel_samples, windows, ctl, wg_frames, wg_samples);
    hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(SEL_BLOCK), 0, s, wg_frames, wg_samples, nwg, nstreams, sel_cap, ctl,
                       sel_frames, sel_samples, status);
    if (nwg)
        hipLaunchKernelGGL(k_sel_apply, dim3(nwg), dim3(SEL_BLOCK), 0, s, sf, nstreams, wg_frames, wg_samples, ctl, sel_frames,
                           sel_samples, windows);
    if (sel_cap) {
        const uint64_t threads = 8ull * sel_cap;
        hipLaunchKernelGGL(k_sel_emit, dim3((uint32_t)((threads + EMIT_THREADS - 1) / EMIT_THREADS)), dim3(EMIT_THREADS), 0, s,
                           offsets, info, cap, sel_frames, sel_samples, nstreams, windows, sel_offsets, sel_info, sel_cap);
    }
    return hipGetLastError();
}

/* ------------------------------------------------------------------ selection per window request */
/* ctl: [0] bad flag, [1] windows that are not empty, [2] windows clipped, [3] a request names no stream.
 * rel_frames: the window's frame prefix inside its workgroup, in 64 bits (k_win_apply saturates). */
__global__ __launch_bounds__(SEL_BLOCK) void k_win_select(const bnf_frame_info *__restrict__ info, uint32_t cap,
                                                          const uint32_t *__restrict__ sf, const uint64_t *__restrict__ ss,
                                                          uint32_t nstreams, const bnf_window_request *__restrict__ requests,
                                                          uint32_t nwindows, uint64_t *__restrict__ rel_frames,
                                                          uint64_t *__restrict__ sel_samples, bnf_window *__restrict__ windows,
                                                          uint32_t *__restrict__ ctl, uint64_t *__restrict__ wg_frames,
                                                          uint64_t *__restrict__ wg_samples) {
    const uint32_t w = blockIdx.x * SEL_BLOCK + threadIdx.x;
    const bool live = w < nwindows;
    bnf_sel_stream o;
    o.nsamples = o.hull = 0;
    o.skip = o.first_frame = o.nframes = 0;
    o.flags = BNF_WIN_EMPTY;
    uint32_t verdict = BNF_REQ_OK;
    if (live) verdict = bnf_select_request(info, cap, sf, ss, nstreams, requests[w], o);
    uint64_t ef, tf, es, ts;
    sel_block_scan<uint64_t>(o.nframes, o.hull, ef, es, tf, ts);
    if (live) {
        rel_frames[w] = ef;
        sel_samples[w] = es;
        windows[w] = bnf_select_window(o, es);
    }
    if (threadIdx.x == 0) {
        wg_frames[blockIdx.x] = tf;
        wg_samples[blockIdx.x] = ts;
    }
    const bool any_bad = __ballot(verdict == BNF_REQ_BAD_SLICE) != 0;
    const bool any_none = __ballot(verdict == BNF_REQ_NO_STREAM) != 0;
    const uint32_t nonempty = (uint32_t)__popcll(__ballot(live && !(o.flags & BNF_WIN_EMPTY)));
    const uint32_t clipped = (uint32_t)__popcll(__ballot(live && (o.flags & BNF_WIN_CLIPPED)));
    if ((threadIdx.x & 63u) == 0) {
        if (any_bad) atomicOr(&ctl[0], 1u);
        if (nonempty) atomicAdd(&ctl[1], nonempty);
        if (clipped) atomicAdd(&ctl[2], clipped);
        if (any_none) atomicOr(&ctl[3], 1u);
    }
}

/* One workgroup: the workgroup sums become their exclusive prefixes; totals (frames saturating) and status. */
__global__ __launch_bounds__(SEL_BLOCK) void k_win_scan(uint64_t *__restrict__ wg_frames, uint64_t *__restrict__ wg_samples,
                                                        uint32_t nwg, uint32_t nwindows, uint32_t sel_cap,
                                                        const uint32_t *__restrict__ ctl, uint32_t *__restrict__ sel_frames,
                                                        uint64_t *__restrict__ sel_samples, uint32_t *__restrict__ status) {
    uint64_t carry_f = 0, carry_s = 0;
    for (uint32_t base = 0; base < nwg; base += SEL_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t f = i < nwg ? wg_frames[i] : 0u;
        const uint64_t s = i < nwg ? wg_samples[i] : 0u;
        uint64_t ef, tf, es, ts;
        sel_block_scan<uint64_t>(f, s, ef, es, tf, ts);
        if (i < nwg) {
            wg_frames[i] = carry_f + ef;
            wg_samples[i] = carry_s + es;
        }
        carry_f += tf;
        carry_s += ts;
    }
    if (threadIdx.x == 0) {
        const bool bad = ctl[0] != 0;
        const uint32_t none = ctl[3] ? BNF_SEL_NO_STREAM : 0u;
        sel_frames[nwindows] = bad ? 0u : bnf_sel_sat32(carry_f);
        sel_samples[nwindows] = bad ? 0u : carry_s;
        status[0] = (bad ? BNF_SEL_BAD_TABLES : carry_f > sel_cap ? BNF_SEL_OVERFLOW : 0u) | none;
        status[1] = bad ? 0u : bnf_sel_sat32(carry_f);
        status[2] = bad ? 0u : ctl[1];
        status[3] = bad ? 0u : ctl[2];
    }
}

__global__ __launch_bounds__(SEL_BLOCK) void k_win_apply(const uint32_t *__restrict__ sf, uint32_t nstreams,
                                                         const bnf_window_request *__restrict__ requests, uint32_t nwindows,
                                                         const uint64_t *__restrict__ rel_frames,
                                                         const uint64_t *__restrict__ wg_frames,
                                                         const uint64_t *__restrict__ wg_samples, const uint32_t *__restrict__ ctl,
                                                         uint32_t *__restrict__ sel_frames, uint64_t *__restrict__ sel_samples,
                                                         bnf_window *__restrict__ windows) {
    const uint32_t w = blockIdx.x * SEL_BLOCK + threadIdx.x;
    if (w >= nwindows) return;
    if (ctl[0]) {
        sel_frames[w] = 0;
        sel_samples[w] = 0;
        windows[w] = bnf_select_no_request(sf, nstreams, requests[w].stream);
    } else {
        sel_frames[w] = bnf_sel_sat32(wg_frames[blockIdx.x] + rel_frames[w]);
        sel_samples[w] += wg_samples[blockIdx.x];
        windows[w].pcm_first += wg_samples[blockIdx.x];
    }
}

extern "C" uint64_t bnf_select_windows_scratch_bytes(uint32_t nwindows) {
    const uint64_t nwg = ((uint64_t)nwindows + SEL_BLOCK - 1) / SEL_BLOCK;
    return 16u + 16u * nwg + 8u * (uint64_t)nwindows;
}

/* The emit is k_sel_emit: its inputs mean the same with a window in a stream's place, and it only
 * compares positions below sel_cap with prefix entries, which saturation leaves in order. */
extern "C" hipError_t bnf_launch_select_windows(const uint64_t *offsets, const bnf_frame_info *info, uint32_t cap,
                                                const uint32_t *sf, const uint64_t *ss, uint32_t nstreams,
                                                const bnf_window_request *requests, uint32_t nwindows, uint64_t *sel_offsets,
                                                bnf_frame_info *sel_info, uint32_t sel_cap, uint32_t *sel_frames,
                                                uint64_t *sel_samples, bnf_window *windows, uint32_t *status, void *scratch,
                                                hipStream_t s) {
    const uint32_t nwg = (uint32_t)(((uint64_t)nwindows + SEL_BLOCK - 1) / SEL_BLOCK);
    uint32_t *ctl = (uint32_t *)scratch;
    uint64_t *wg_frames = (uint64_t *)((uint8_t *)scratch + 16u);
    uint64_t *wg_samples = wg_frames + nwg;
    uint64_t *rel_frames = wg_samples + nwg;
    hipError_t e = hipMemsetAsync(ctl, 0, 16, s);
    if (e != hipSuccess) return e;
    if (nwg)
        hipLaunchKernelGGL(k_win_select, dim3(nwg), dim3(SEL_BLOCK), 0, s, info, cap, sf, ss, nstreams, requests, nwindows,
                           rel_frames, sel_samples, windows, ctl, wg_frames, wg_samples);
    hipLaunchKernelGGL(k_win_scan, dim3(1), dim3(SEL_BLOCK), 0, s, wg_frames, wg_samples, nwg, nwindows, sel_cap, ctl,
                       sel_frames, sel_samples, status);
    if (nwg)
        hipLaunchKernelGGL(k_win_apply, dim3(nwg), dim3(SEL_BLOCK), 0, s, sf, nstreams, requests, nwindows, rel_frames,
                           wg_frames, wg_samples, ctl, sel_frames, sel_samples, windows);
    if (sel_cap) {
        const uint64_t threads = 8ull * sel_cap;
        hipLaunchKernelGGL(k_sel_emit, dim3((uint32_t)((threads + EMIT_THREADS - 1) / EMIT_THREADS)), dim3(EMIT_THREADS), 0, s,
                           offsets, info, cap, sel_frames, sel_samples, nwindows, windows, sel_offsets, sel_info, sel_cap);
    }
    return hipGetLastError();
}

/* ------------------------------------------------------------------ shared selection: every frame once
 * ctl: [0] bad flag, [1] windows that are not empty, [2] windows clipped, [3] a request names no stream,
 * [4] one past the last position a window covers (never above cap), [5] frames selected, 0 under the
 * bad flag (written by the final k_shr_scan for the emit), [6], [7] unused. */
#define SHR_CTL_WORDS 8

__global__ __launch_bounds__(SEL_BLOCK) void k_shr_mark(const bnf_frame_info *__restrict__ info, uint32_t cap,
                                                        const uint32_t *__restrict__ sf, const uint64_t *__restrict__ ss,
                                                        uint32_t nstreams, const bnf_window_request *__restrict__ requests,
                                                        uint32_t nwindows, bnf_window *__restrict__ windows,
                                                        uint32_t *__restrict__ ctl, int32_t *__restrict__ delta) {
    const uint32_t w = blockIdx.x * SEL_BLOCK + threadIdx.x;
    const bool live = w < nwindows;
    bnf_sel_stream o;
    o.nsamples = o.hull = 0;
    o.skip = o.first_frame = o.nframes = 0;
    o.flags = BNF_WIN_EMPTY;
    uint32_t verdict = BNF_REQ_OK;
    if (live) {
        verdict = bnf_select_request(info, cap, sf, ss, nstreams, requests[w], o);
        windows[w] = bnf_select_shared_window(o);
    }
    uint32_t end = 0; /* a run lies inside its stream's slice: first_frame + nframes <= cap, delta has cap + 1 entries */
    if (o.nframes) {
        end = o.first_frame + o.nframes;
        atomicAdd(&delta[o.first_frame], 1);
        atomicAdd(&delta[end], -1);
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        const uint32_t other = __shfl_xor(end, d);
        end = other > end ? other : end;
    }
    const bool any_bad = __ballot(verdict == BNF_REQ_BAD_SLICE) != 0;
    const bool any_none = __ballot(verdict == BNF_REQ_NO_STREAM) != 0;
    const uint32_t nonempty = (uint32_t)__popcll(__ballot(live && !(o.flags & BNF_WIN_EMPTY)));
    const uint32_t clipped = (uint32_t)__popcll(__ballot(live && (o.flags & BNF_WIN_CLIPPED)));
    if ((threadIdx.x & 63u) == 0) {
        if (any_bad) atomicOr(&ctl[0], 1u);
        if (nonempty) atomicAdd(&ctl[1], nonempty);
        if (clipped) atomicAdd(&ctl[2], clipped);
        if (any_none) atomicOr(&ctl[3], 1u);
        if (end) atomicMax(&ctl[4], end);
    }
}

/* The running sum of delta inside each workgroup's 1,024 positions, in place, and the workgroup's sum.
 * A workgroup at or past ctl[4] holds zeros only: it writes a zero sum and leaves. */
__global__ __launch_bounds__(SEL_BLOCK) void k_shr_cover(int32_t *__restrict__ delta, uint32_t cap,
                                                         const uint32_t *__restrict__ ctl, uint32_t *__restrict__ wg_cover) {
    const uint32_t high = ctl[4] < cap ? ctl[4] : cap;
    if (blockIdx.x * SEL_BLOCK >= high) {
        if (threadIdx.x == 0) wg_cover[blockIdx.x] = 0;
        return;
    }
    const uint32_t i = blockIdx.x * SEL_BLOCK + threadIdx.x;
    const uint32_t d = i < cap ? (uint32_t)delta[i] : 0u; /* sums modulo 2^32 are the signed sums */
    uint32_t ef, tf;
    uint64_t es, ts;
    sel_block_scan<uint32_t>(d, 0, ef, es, tf, ts);
    if (i < cap) delta[i] = (int32_t)(ef + d);
    if (threadIdx.x == 0) wg_cover[blockIdx.x] = tf;
}

/* One workgroup: the workgroup sums become their exclusive prefixes.  LAST: frames and samples of the
 * covered positions, then the totals and the status words; else the cover sums alone. */
template <bool LAST>
__global__ __launch_bounds__(SEL_BLOCK) void k_shr_scan(uint32_t *__restrict__ wg_frames, uint64_t *__restrict__ wg_samples,
                                                        uint32_t nwg, uint32_t sel_cap, uint32_t *__restrict__ ctl,
                                                        uint64_t *__restrict__ totals, uint32_t *__restrict__ status) {
    uint32_t carry_f = 0;
    uint64_t carry_s = 0;
    for (uint32_t base = 0; base < nwg; base += SEL_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t f = i < nwg ? wg_frames[i] : 0u;
        const uint64_t s = LAST && i < nwg ? wg_samples[i] : 0u;
        uint32_t ef, tf;
        uint64_t es, ts;
        sel_block_scan<uint32_t>(f, s, ef, es, tf, ts);
        if (i < nwg) {
            wg_frames[i] = carry_f + ef;
            if (LAST) wg_samples[i] = carry_s + es;
        }
        carry_f += tf;
        carry_s += ts;
    }
    if (LAST && threadIdx.x == 0) {
        const bool bad = ctl[0] != 0;
        const uint32_t none = ctl[3] ? BNF_SEL_NO_STREAM : 0u;
        ctl[5] = bad ? 0u : carry_f;
        totals[0] = bad ? 0u : carry_f;
        totals[1] = bad ? 0u : carry_s;
        status[0] = (bad ? BNF_SEL_BAD_TABLES : carry_f > sel_cap ? BNF_SEL_OVERFLOW : 0u) | none;
        status[1] = bad ? 0u : carry_f;
        status[2] = bad ? 0u : ctl[1];
        status[3] = bad ? 0u : ctl[2];
    }
}

/* Position i is covered when its workgroup's base plus its running sum is positive.  The exclusive scan
 * of (covered, covered ? blocksize : 0) inside the workgroup goes to rank / pos, covered itself replaces
 * the running sum in delta.  info is read at covered positions only. */
__global__ __launch_bounds__(SEL_BLOCK) void k_shr_rank(const bnf_frame_info *__restrict__ info, uint32_t cap,
                                                        const uint32_t *__restrict__ ctl, const uint32_t *__restrict__ wg_cover,
                                                        int32_t *__restrict__ delta, uint32_t *__restrict__ rank,
                                                        uint64_t *__restrict__ pos, uint32_t *__restrict__ wg_frames,
                                                        uint64_t *__restrict__ wg_samples) {
    const uint32_t high = ctl[4] < cap ? ctl[4] : cap;
    if (blockIdx.x * SEL_BLOCK >= high) {
        if (threadIdx.x == 0) {
            wg_frames[blockIdx.x] = 0;
            wg_samples[blockIdx.x] = 0;
        }
        return;
    }
    const uint32_t i = blockIdx.x * SEL_BLOCK + threadIdx.x;
    const bool covered = i < cap && (int32_t)(wg_cover[blockIdx.x] + (uint32_t)delta[i]) > 0;
    const uint32_t bs = covered ? info[i].blocksize : 0u;
    uint32_t ef, tf;
    uint64_t es, ts;
    sel_block_scan<uint32_t>(covered ? 1u : 0u, bs, ef, es, tf, ts);
    if (i < cap) {
        delta[i] = covered ? 1 : 0;
        rank[i] = ef;
        pos[i] = es;
    }
    if (threadIdx.x == 0) {
        wg_frames[blockIdx.x] = tf;
        wg_samples[blockIdx.x] = ts;
    }
}

/* 8 lanes per position q, as in k_sel_emit.  As an index position (q below ctl[4]): a covered one copies
 * its record to its rank, if that is below sel_cap, with out_sample = its pos.  As a position of the
 * output (q below sel_cap): at or past the frame total it gets the filler.  The two sets of output
 * positions are disjoint (rank < total <= filler). */
__global__ __launch_bounds__(EMIT_THREADS) void k_shr_emit(const uint64_t *__restrict__ offsets,
                                                           const bnf_frame_info *__restrict__ info, uint32_t cap,
                                                           const uint32_t *__restrict__ ctl, const int32_t *__restrict__ delta,
                                                           const uint32_t *__restrict__ rank, const uint64_t *__restrict__ pos,
                                                           const uint32_t *__restrict__ wg_frames,
                                                           const uint64_t *__restrict__ wg_samples,
                                                           uint64_t *__restrict__ sel_offsets,
                                                           bnf_frame_info *__restrict__ sel_info, uint32_t sel_cap) {
    const uint64_t gid = (uint64_t)blockIdx.x * EMIT_THREADS + threadIdx.x;
    const uint64_t q64 = gid >> 3;
    const uint32_t part = (uint32_t)gid & 7u; /* bytes [16 part, 16 part + 16) of the record */
    const uint32_t high = ctl[0] ? 0u : ctl[4] < cap ? ctl[4] : cap;
    if (q64 >= high && q64 >= sel_cap) return;
    const uint32_t q = (uint32_t)q64;
    if (q < sel_cap && q >= ctl[5]) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u); /* the filler: zeros, status 3 (skipped), err -1 */
        if (part == 0) {
            v.x = BNF_ST_SKIPPED;
            v.y = 0xffffffffu;
        }
        ((uint4 *)(sel_info + q))[part] = v;
        if (part == 0 && sel_offsets) sel_offsets[q] = 0;
    }
    if (q < high && delta[q]) {
        const uint32_t r = wg_frames[q / SEL_BLOCK] + rank[q];
        if (r < sel_cap) {
            uint4 v = ((const uint4 *)(info + q))[part];
            if (part == 4) { /* out_sample: bytes 64..71 */
                const uint64_t os = wg_samples[q / SEL_BLOCK] + pos[q];
                v.x = (uint32_t)os;
                v.y = (uint32_t)(os >> 32);
            }
            ((uint4 *)(sel_info + r))[part] = v;
            if (part == 0 && sel_offsets) sel_offsets[r] = offsets ? offsets[q] : 0u;
        }
    }
}

/* One lane per window: pcm_first gains the pos of the window's first frame, win_sel_first its rank; under
 * the bad flag every window is emptied. */
__global__ __launch_bounds__(SEL_BLOCK) void k_shr_windows(const uint32_t *__restrict__ sf, uint32_t nstreams,
                                                           const bnf_window_request *__restrict__ requests, uint32_t nwindows,
                                                           uint32_t cap, const uint32_t *__restrict__ ctl,
                                                           const uint32_t *__restrict__ rank, const uint64_t *__restrict__ pos,
                                                           const uint32_t *__restrict__ wg_frames,
                                                           const uint64_t *__restrict__ wg_samples,
                                                           bnf_window *__restrict__ windows, uint32_t *__restrict__ win_sel_first) {
    const uint32_t w = blockIdx.x * SEL_BLOCK + threadIdx.x;
    if (w >= nwindows) return;
    uint32_t first = 0;
    if (ctl[0]) {
        windows[w] = bnf_select_no_request(sf, nstreams, requests[w].stream);
    } else {
        const uint32_t a = windows[w].first_frame;
        if (windows[w].nframes && a < cap) { /* a < cap holds for every run k_shr_mark wrote */
            windows[w].pcm_first += wg_samples[a / SEL_BLOCK] + pos[a];
            first = wg_frames[a / SEL_BLOCK] + rank[a];
        }
    }
    if (win_sel_first) win_sel_first[w] = first;
}

/* Scratch: 32 bytes of ctl, then 16 bytes per position (delta 4, rank 4, pos 8; delta has one entry more)
 * and 16 bytes per 1,024 positions (the three workgroup sums), each table rounded up to 16 bytes.
 * Nothing per window: the window records are written in place.  npos = cap, or 0 without windows. */
struct shr_scratch {
    uint32_t *ctl;
    int32_t *delta;
    uint32_t *rank, *wg_cover, *wg_frames;
    uint64_t *pos, *wg_samples;
    uint64_t bytes;
};

static shr_scratch shr_layout(void *scratch, uint32_t npos) {
    const uint64_t nwg = ((uint64_t)npos + SEL_BLOCK - 1) / SEL_BLOCK;
    auto up16 = [](uint64_t n) { return (n + 15u) & ~(uint64_t)15; };
    uint8_t *p = (uint8_t *)scratch;
    shr_scratch x;
    x.ctl = (uint32_t *)p; /* ctl and delta are zeroed by one memset */
    x.delta = (int32_t *)(p + 4u * SHR_CTL_WORDS);
    p += up16(4u * SHR_CTL_WORDS + 4u * ((uint64_t)npos + 1));
    x.pos = (uint64_t *)p;
    p += up16(8u * (uint64_t)npos);
    x.wg_samples = (uint64_t *)p;
    p += up16(8u * nwg);
    x.rank = (uint32_t *)p;
    p += up16(4u * (uint64_t)npos);
    x.wg_cover = (uint32_t *)p;
    p += up16(4u * nwg);
    x.wg_frames = (uint32_t *)p;
    p += up16(4u * nwg);
    x.bytes = (uint64_t)(p - (uint8_t *)scratch);
    return x;
}

extern "C" uint64_t bnf_select_shared_scratch_bytes(uint32_t cap, uint32_t nwindows) {
    return shr_layout(nullptr, nwindows ? cap : 0u).bytes;
}

extern "C" hipError_t bnf_launch_select_windows_shared(const uint64_t *offsets, const bnf_frame_info *info, uint32_t cap,
                                                       const uint32_t *sf, const uint64_t *ss, uint32_t nstreams,
                                                       const bnf_window_request *requests, uint32_t nwindows,
                                                       uint64_t *sel_offsets, bnf_frame_info *sel_info, uint32_t sel_cap,
                                                       bnf_window *windows, uint32_t *win_sel_first, uint64_t *totals,
                                                       uint32_t *status, void *scratch, hipStream_t s) {
    const uint32_t npos = nwindows ? cap : 0u; /* without windows no position is looked at */
    const uint32_t nwg = (uint32_t)(((uint64_t)nwindows + SEL_BLOCK - 1) / SEL_BLOCK);
    const uint32_t npwg = (uint32_t)(((uint64_t)npos + SEL_BLOCK - 1) / SEL_BLOCK);
    const shr_scratch x = shr_layout(scratch, npos);
    hipError_t e = hipMemsetAsync(x.ctl, 0, 4u * SHR_CTL_WORDS + 4u * ((size_t)npos + 1), s);
    if (e != hipSuccess) return e;
    if (nwg)
        hipLaunchKernelGGL(k_shr_mark, dim3(nwg), dim3(SEL_BLOCK), 0, s, info, cap, sf, ss, nstreams, requests, nwindows, windows,
                           x.ctl, x.delta);
    if (npwg) {
        hipLaunchKernelGGL(k_shr_cover, dim3(npwg), dim3(SEL_BLOCK), 0, s, x.delta, cap, x.ctl, x.wg_cover);
        hipLaunchKernelGGL(k_shr_scan<false>, dim3(1), dim3(SEL_BLOCK), 0, s, x.wg_cover, (uint64_t *)nullptr, npwg, sel_cap,
                           x.ctl, (uint64_t *)nullptr, (uint32_t *)nullptr);
        hipLaunchKernelGGL(k_shr_rank, dim3(npwg), dim3(SEL_BLOCK), 0, s, info, cap, x.ctl, x.wg_cover, x.delta, x.rank, x.pos,
                           x.wg_frames, x.wg_samples);
    }
    hipLaunchKernelGGL(k_shr_scan<true>, dim3(1), dim3(SEL_BLOCK), 0, s, x.wg_frames, x.wg_samples, npwg, sel_cap, x.ctl, totals,
                       status);
    const uint64_t threads = 8ull * (npos > sel_cap ? npos : sel_cap);
    if (threads)
        hipLaunchKernelGGL(k_shr_emit, dim3((uint32_t)((threads + EMIT_THREADS - 1) / EMIT_THREADS)), dim3(EMIT_THREADS), 0, s,
                           offsets, info, cap, x.ctl, x.delta, x.rank, x.pos, x.wg_frames, x.wg_samples, sel_offsets, sel_info,
                           sel_cap);
    if (nwg)
        hipLaunchKernelGGL(k_shr_windows, dim3(nwg), dim3(SEL_BLOCK), 0, s, sf, nstreams, requests, nwindows, cap, x.ctl, x.rank,
                           x.pos, x.wg_frames, x.wg_samples, windows, win_sel_first);
    return hipGetLastError();
}

/* ------------------------------------------------------------------ gather */
#define GATHER_THREADS 256
#define GATHER_UNROLL 4
#define GATHER_SLOTS (GATHER_THREADS * GATHER_UNROLL)

/* The 16 bytes that start sh = 4 DW + b bytes into the 32 bytes lo | hi. */
template <int DW>
__device__ __forceinline__ uint4 gather_realign(const uint4 lo, const uint4 hi, uint32_t b) {
    const uint32_t c[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return make_uint4(__builtin_amdgcn_alignbyte(c[DW + 1], c[DW], b), __builtin_amdgcn_alignbyte(c[DW + 2], c[DW + 1], b),
                      __builtin_amdgcn_alignbyte(c[DW + 3], c[DW + 2], b),
                      __builtin_amdgcn_alignbyte(c[DW + 4 > 7 ? 7 : DW + 4], c[DW + 3], b));
}

/* keep the first m bytes (m < 16) of v */
__device__ __forceinline__ uint4 gather_mask(uint4 v, uint32_t m) {
    auto word = [m](uint32_t x, uint32_t j) {
        const uint32_t k = m > 4u * j ? m - 4u * j : 0u;
        return k >= 4u ? x : x & ((1u << (8u * k)) - 1u);
    };
    return make_uint4(word(v.x, 0), word(v.y, 1), word(v.z, 2), word(v.w, 3));
}

/* The aligned slots of one row: slot q is dst[hb + 16 q, + 16), its data src[src0 + hb + 16 q, ...)
 * while below n bytes of the row. */
template <int DW>
__device__ __forceinline__ void gather_body(const uint8_t *__restrict__ pcm, uint64_t src0, uint64_t last_blk, uint32_t b,
                                            uint8_t *__restrict__ dst, uint32_t hb, uint64_t nslots, uint64_t n) {
    for (uint64_t chunk = blockIdx.y; chunk * GATHER_SLOTS < nslots; chunk += gridDim.y) {
        uint4 v[GATHER_UNROLL];
#pragma unroll
        for (int u = 0; u < GATHER_UNROLL; u++) {
            const uint64_t q = chunk * GATHER_SLOTS + (uint32_t)u * GATHER_THREADS + threadIdx.x;
            const uint64_t o = hb + 16u * q;
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            if (q < nslots && o < n) {
                const uint64_t a = (src0 + o) & ~(uint64_t)15;
                const uint64_t a1 = a + 16u < last_blk ? a + 16u : last_blk;
                const uint4 lo = *(const uint4 *)(pcm + a), hi = *(const uint4 *)(pcm + a1);
                v[u] = gather_realign<DW>(lo, hi, b);
                if (n - o < 16u) v[u] = gather_mask(v[u], (uint32_t)(n - o));
            }
        }
#pragma unroll
        for (int u = 0; u < GATHER_UNROLL; u++) {
            const uint64_t q = chunk * GATHER_SLOTS + (uint32_t)u * GATHER_THREADS + threadIdx.x;
            if (q < nslots) *(uint4 *)(dst + hb + 16u * q) = v[u];
        }
    }
}

/* status: [0] bit 0 a window outside pcm_bytes, [1] such windows, [2] rows cut at row_samples */
__global__ __launch_bounds__(GATHER_THREADS) void k_gather_ranges(const uint8_t *__restrict__ pcm, uint64_t pcm_bytes,
                                                                  uint32_t stride, const bnf_window *__restrict__ windows,
                                                                  uint32_t row_samples, uint64_t row_bytes,
                                                                  uint8_t *__restrict__ rows, uint32_t *__restrict__ status) {
    const uint32_t s = blockIdx.x;
    const uint64_t first = windows[s].pcm_first, want = windows[s].nsamples;
    const uint64_t limit = pcm_bytes / stride; /* whole sample frames of the PCM */
    const bool bad = want != 0 && (first > limit || want > limit - first);
    const uint64_t ncopy = bad ? 0u : want < row_samples ? want : row_samples;
    const uint64_t W = (uint64_t)row_samples * stride, n = ncopy * stride; /* bytes written, bytes of them copied */
    const uint64_t src0 = n ? first * stride : 0u;
    uint8_t *const dst = rows + (uint64_t)s * row_bytes;
    const uint32_t to16 = (16u - ((uint32_t)(uintptr_t)dst & 15u)) & 15u;
    const uint32_t hb = to16 < W ? to16 : (uint32_t)W; /* bytes in front of the first aligned slot */
    const uint64_t nslots = (W - hb) >> 4;
    const uint32_t tb = (uint32_t)(W - hb) & 15u; /* bytes behind the last one */
    if (blockIdx.y == 0) {
        if (threadIdx.x == 0) {
            if (bad) {
                atomicOr(&status[0], 1u);
                atomicAdd(&status[1], 1u);
            } else if (want > row_samples) {
                atomicAdd(&status[2], 1u);
            }
        }
        const uint32_t t = threadIdx.x & 15u;
        if (threadIdx.x < 16u) {
            if (t < hb) dst[t] = t < n ? pcm[src0 + t] : (uint8_t)0;
        } else if (threadIdx.x < 32u) {
            const uint64_t o = hb + 16u * nslots + t;
            if (t < tb) dst[o] = o < n ? pcm[src0 + o] : (uint8_t)0;
        }
    }
    if (!nslots) return;
    const uint64_t last_blk = pcm_bytes ? ((pcm_bytes + 15u) & ~(uint64_t)15) - 16u : 0u;
    const uint32_t sh = (uint32_t)(src0 + hb) & 15u;
    switch (sh >> 2) { /* uniform over the row */
    case 0: gather_body<0>(pcm, src0, last_blk, sh & 3u, dst, hb, nslots, n); break;
    case 1: gather_body<1>(pcm, src0, last_blk, sh & 3u, dst, hb, nslots, n); break;
    case 2: gather_body<2>(pcm, src0, last_blk, sh & 3u, dst, hb, nslots, n); break;
    default: gather_body<3>(pcm, src0, last_blk, sh & 3u, dst, hb, nslots, n); break;
    }
}

extern "C" hipError_t bnf_launch_gather_ranges(const uint8_t *pcm, uint64_t pcm_bytes, uint32_t stride,
                                               const bnf_window *windows, uint32_t nstreams, uint32_t row_samples,
                                               uint64_t row_bytes, uint8_t *rows, uint32_t *status, hipStream_t s) {
    hipError_t e = hipMemsetAsync(status, 0, 4 * sizeof(uint32_t), s);
    if (e != hipSuccess || !nstreams) return e;
    if (!stride) return hipErrorInvalidValue;
    const uint64_t chunks = ((uint64_t)row_samples * stride / 16u + GATHER_SLOTS - 1) / GATHER_SLOTS;
    const dim3 grid(nstreams, (uint32_t)(chunks < 1 ? 1 : chunks > 65535u ? 65535u : chunks)), block(GATHER_THREADS);
    hipLaunchKernelGGL(k_gather_ranges, grid, block, 0, s, pcm, pcm_bytes, stride, windows, row_samples, row_bytes, rows, status);
    return hipGetLastError();
}
