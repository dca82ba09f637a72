/*
 * bnflac_f32.hip -- k_gather_f32 (bnflac_gather_ranges_f32): the windows of a decoded selection
 * as normalised float32 channel planes, optionally mixed down to mono.  The rule, and every
 * address and value the kernel computes, is bnf_pcm_f32.h's.  No CRC tables, no g_stats, no
 * ablate word.
 *
 * One workgroup per stream (blockIdx.x) walks the row's tiles (blockIdx.y, grid strided); a tile
 * is bnf_f32_tile_frames(channels) sample frames, at most 4,096 samples.  Three steps per tile:
 *   load    the tile's aligned 16-byte source blocks, one per lane and pass (a wave reads 1 KiB
 *           contiguous), all passes issued before the first is stored; each goes to LDS as it
 *           is (ds_write_b128 at consecutive slots).  A bad window loads nothing.
 *   unpack  lane <-> sample e = i * channels + c in source order: the dword(s) of the raw bytes
 *           the sample lies in (consecutive lanes read the same or consecutive dwords), then
 *           one int32 to the plane-major stage at c * pitch + i.  pitch modulo 32 is chosen per
 *           channel count so that the 32 lanes of a ds_write_b32 group hit 32 banks
 *           (bnf_f32_pitch).
 *   store   per plane, lane <-> 4 consecutive samples that make one aligned 16-byte global store
 *           (a wave writes 1 KiB contiguous).  The group's place in the stage row has any phase
 *           modulo 4 (the destination's phase differs between planes), so the lane reads the one
 *           or two aligned groups of 4 the samples lie in (ds_read_b128, consecutive slots over the
 *           lanes) and picks by the phase, which is uniform over the plane.  Up to 3 floats in
 *           front of the first aligned group and behind the last go out singly.  Samples past
 *           the window's data are zero stores of the same shape.
 * Trip counts: passes over blocks, samples and groups of a tile, all bounded by the tile's size;
 * tiles by row_samples.  A window's fields only enter through bnf_f32_window's check.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bnf_pcm_f32.h"
#include "bnflac_launch.h"

#define F32_THREADS 256
#define F32_LOAD_PASSES ((BNF_F32_RAW_BLOCKS + F32_THREADS - 1) / F32_THREADS)

static_assert(sizeof(bnf_f32_i4) == 16 && sizeof(bnf_window) == 32, "record sizes");

/* status: [0] bit 0 a window outside pcm_bytes, [1] such windows, [2] rows cut at row_samples */
__global__ __launch_bounds__(F32_THREADS) void k_gather_f32(const uint8_t *__restrict__ pcm, uint64_t pcm_bytes,
                                                            uint32_t stride, uint32_t unit, uint32_t bps, uint32_t channels,
                                                            uint32_t flags, const bnf_window *__restrict__ windows,
                                                            uint32_t row_samples, uint64_t plane_pitch,
                                                            float *__restrict__ out, uint32_t *__restrict__ status) {
    __shared__ uint4 raw4[BNF_F32_RAW_BLOCKS];
    __shared__ bnf_f32_i4 stage4[BNF_F32_STAGE_WORDS / 4];
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const bnf_f32_row row = bnf_f32_window(windows[s].pcm_first, windows[s].nsamples, pcm_bytes, stride, row_samples);
    if (blockIdx.y == 0 && t == 0) {
        if (row.bad) {
            atomicOr(&status[0], BNF_F32_BAD_WINDOW);
            atomicAdd(&status[1], 1u);
        } else if (row.cut) {
            atomicAdd(&status[2], 1u);
        }
    }
    const bnf_f32_conv cv = bnf_f32_conv_of(channels, bps, flags);
    const uint32_t frames = bnf_f32_tile_frames(channels), magic = bnf_f32_magic(channels);
    const uint32_t planes = cv.mono ? 1u : channels;
    const uint64_t last_blk = bnf_f32_last_block(pcm_bytes);
    const uint64_t ntiles = ((uint64_t)row_samples + frames - 1u) / frames;
    const uint32_t *const raw = (const uint32_t *)raw4;
    int32_t *const stage = (int32_t *)stage4;
    for (uint64_t tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
        const uint64_t t0 = tile * frames;
        const bnf_f32_tile tl = bnf_f32_tile_of(row, t0, frames, stride, row_samples);
        if (tl.ndata) { /* uniform over the workgroup */
            uint4 v[F32_LOAD_PASSES];
#pragma unroll
            for (int u = 0; u < (int)F32_LOAD_PASSES; u++) {
                const uint32_t j = (uint32_t)u * F32_THREADS + t;
                v[u] = make_uint4(0u, 0u, 0u, 0u);
                if (j < tl.nblk) v[u] = *(const uint4 *)(pcm + bnf_f32_block_addr(tl, j, last_blk));
            }
#pragma unroll
            for (int u = 0; u < (int)F32_LOAD_PASSES; u++) {
                const uint32_t j = (uint32_t)u * F32_THREADS + t;
                if (j < tl.nblk) raw4[j] = v[u];
            }
            __syncthreads(); /* also: the previous tile's stage has been read */
            const uint32_t nel = tl.ndata * channels;
            for (uint32_t e = t; e < nel; e += F32_THREADS) {
                const uint32_t i = bnf_f32_frame_of(e, magic), c = e - i * channels;
                stage[c * cv.pitch + i] = bnf_f32_fetch(raw, tl.phase + e * unit, unit);
            }
        }
        __syncthreads();
        for (uint32_t c = 0; c < planes; c++) {
            float *const D = out + ((uint64_t)s * planes + c) * plane_pitch + t0;
            uint32_t head, ngroups;
            bnf_f32_split((uint32_t)((uintptr_t)D >> 2), tl.nt, head, ngroups);
            for (uint32_t q = t; q < ngroups; q += F32_THREADS) {
                float f[4];
                bnf_f32_value4(stage4, cv, c, head + 4u * q, tl.ndata, f);
                *(float4 *)(D + head + 4u * q) = make_float4(f[0], f[1], f[2], f[3]);
            }
            const uint32_t behind = head + 4u * ngroups; /* the singles: lanes 0..2 and 64..66 */
            if (t < head) D[t] = bnf_f32_value1(stage4, cv, c, t, tl.ndata);
            if (t >= 64u && behind + (t - 64u) < tl.nt) D[behind + (t - 64u)] = bnf_f32_value1(stage4, cv, c, behind + (t - 64u), tl.ndata);
        }
    }
}

extern "C" hipError_t bnf_launch_gather_f32(const uint8_t *pcm, uint64_t pcm_bytes, uint32_t stride, uint32_t unit,
                                            uint32_t bps, uint32_t channels, uint32_t flags, const bnf_window *windows,
                                            uint32_t nstreams, uint32_t row_samples, uint64_t plane_pitch, float *out,
                                            uint32_t *status, hipStream_t s) {
    hipError_t e = hipMemsetAsync(status, 0, 4 * sizeof(uint32_t), s);
    if (e != hipSuccess || !nstreams) return e;
    if (!stride || channels < 1 || channels > 8 || unit * channels != stride || unit < 2 || unit > 4 || bps < 1 || bps > 32)
        return hipErrorInvalidValue;
    const uint64_t ntiles = ((uint64_t)row_samples + bnf_f32_tile_frames(channels) - 1u) / bnf_f32_tile_frames(channels);
    const dim3 grid(nstreams, (uint32_t)(ntiles < 1 ? 1 : ntiles > 65535u ? 65535u : ntiles)), block(F32_THREADS);
    hipLaunchKernelGGL(k_gather_f32, grid, block, 0, s, pcm, pcm_bytes, stride, unit, bps, channels, flags, windows,
                       row_samples, plane_pitch, out, status);
    return hipGetLastError();
}
