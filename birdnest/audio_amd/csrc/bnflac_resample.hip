/*
 * bnflac_resample.hip -- k_gather_f32_rs (bnflac_gather_ranges_f32_rs): the windows of a decoded
 * selection as float32 channel planes at another sample rate.  The rule, and every address and
 * value the kernel computes, is bnf_resample.h's (on top of bnf_pcm_f32.h's window check, block
 * loads, sample fetch and conversions).  No CRC tables, no g_stats, no ablate word.
 *
 * One workgroup per window (blockIdx.x) walks the row's tiles of BNF_RSMP_TILE outputs (blockIdx.y,
 * grid strided) and, inside a tile, the steps of bnf_rsmp_step_outputs() outputs.  All LDS is the
 * dynamic region, every part a multiple of 16 bytes: the raw blocks of a step (the two store
 * buffers reuse them), the plane-major float stage, and the whole taps table, loaded once per
 * workgroup with its rows bnf_rsmp_tap_pitch(K) floats apart.  Per step:
 *   load    the aligned 16-byte source blocks of the step's span, one per lane and pass, all passes
 *           issued before the first is stored (ds_write_b128 at consecutive slots).
 *   unpack  lane <-> stage slot in source order: the converted float, or +0.0f outside the window,
 *           to c * pitch + u (bnf_f32_pitch: 32 lanes, 32 banks).  Mono: lane <-> sample frame.
 *   filter  per plane, lane <-> consecutive outputs.  Neighbouring lanes read neighbouring x
 *           (ds_read_b32, stride M / L) and the tap rows of their phases (ds_read_b128; the phase
 *           advances by M mod L per lane and the row pitch / 4 is odd, so the lanes of a 16-lane
 *           group that differ in phase modulo 16 differ in bank group).  All K terms run for
 *           every lane; the value goes to a store buffer at the destination's phase modulo 4.
 *   store   per plane, lane <-> one aligned 16-byte group of the buffer (ds_read_b128) and one
 *           aligned 16-byte global store; up to 3 single floats at each end.  Two buffers
 *           alternate between planes, so one barrier per plane orders both hand-overs.
 * Trip counts: tiles by row_out, steps by BNF_RSMP_TILE, blocks and slots by the span (at most
 * BNF_F32_RAW_BLOCKS blocks, 4,096 slots), taps by K.  A window's fields only enter through
 * bnf_rsmp_window.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bnf_resample.h"
#include "bnflac_launch.h"

#define RS_THREADS 256
#define RS_LOAD_PASSES ((BNF_F32_RAW_BLOCKS + RS_THREADS - 1) / RS_THREADS)
#define RS_RAW_BYTES (16u * BNF_F32_RAW_BLOCKS)
#define RS_STAGE_BYTES (4u * BNF_F32_STAGE_WORDS)

static_assert(sizeof(bnf_rsmp_f4) == 16 && sizeof(bnf_window) == 32 && sizeof(bnf_rsmp_spec) == 16, "record sizes");
static_assert(RS_RAW_BYTES % 16 == 0 && RS_STAGE_BYTES % 16 == 0, "every part of the LDS starts on 16 bytes");
static_assert(2u * 4u * BNF_RSMP_YBUF <= RS_RAW_BYTES, "the two store buffers fit the raw blocks' place");
static_assert(BNF_RSMP_YBUF % 4 == 0, "the second store buffer is 16-byte aligned");

/* bytes of dynamic LDS for a spec */
static uint32_t rs_lds_bytes(const bnf_rsmp_spec &sp) {
    return RS_RAW_BYTES + RS_STAGE_BYTES + 4u * sp.up * bnf_rsmp_tap_pitch(sp.taps);
}

/* status: [0] bit 0 a window outside pcm_bytes, [1] such windows, [2] windows with more outputs than row_out */
__global__ __launch_bounds__(RS_THREADS) void k_gather_f32_rs(const uint8_t *__restrict__ pcm, uint64_t pcm_bytes,
                                                              uint32_t stride, uint32_t unit, uint32_t bps,
                                                              uint32_t channels, uint32_t flags,
                                                              const bnf_window *__restrict__ windows, bnf_rsmp_spec sp,
                                                              const float *__restrict__ taps, uint32_t row_out,
                                                              uint64_t plane_pitch, float *__restrict__ out,
                                                              uint32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint4 *const raw4 = (uint4 *)smem;
    float *const ybuf = (float *)smem; /* 2 x BNF_RSMP_YBUF floats, while the raw blocks are not needed */
    float *const stage = (float *)(smem + RS_RAW_BYTES);
    float *const ltaps = (float *)(smem + RS_RAW_BYTES + RS_STAGE_BYTES);
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const bnf_rsmp_row row = bnf_rsmp_window(windows[s].pcm_first, windows[s].nsamples, pcm_bytes, stride, sp, row_out);
    if (blockIdx.y == 0 && t == 0) {
        if (row.bad) {
            atomicOr(&status[0], BNF_F32_BAD_WINDOW);
            atomicAdd(&status[1], 1u);
        } else if (row.cut) {
            atomicAdd(&status[2], 1u);
        }
    }
    const bnf_f32_conv cv = bnf_f32_conv_of(channels, bps, flags);
    const uint32_t magic = bnf_f32_magic(channels), planes = cv.mono ? 1u : channels;
    const uint32_t so = bnf_rsmp_step_outputs(sp, channels), tap_pitch = bnf_rsmp_tap_pitch(sp.taps);
    const uint64_t last_blk = bnf_f32_last_block(pcm_bytes);
    const uint32_t ntiles = (row_out + BNF_RSMP_TILE - 1u) / BNF_RSMP_TILE;
    const uint32_t *const raw = (const uint32_t *)raw4;
    if (row.ncopy) { /* uniform over the workgroup: the table, 4 floats per lane and pass */
        const uint32_t k4 = sp.taps >> 2, ngr = sp.up * k4;
        for (uint32_t g = t; g < ngr; g += RS_THREADS) {
            const uint32_t ph = g / k4, col = g - ph * k4;
            *(bnf_rsmp_f4 *)(ltaps + ph * tap_pitch + 4u * col) = *(const bnf_rsmp_f4 *)(taps + 4u * g);
        }
    }
    for (uint32_t tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
        const uint32_t t0 = tile * BNF_RSMP_TILE;
        const uint32_t tend = row_out - t0 < BNF_RSMP_TILE ? row_out : t0 + BNF_RSMP_TILE;
        for (uint32_t r1 = t0; r1 < tend; r1 += so) {
            const uint32_t cnt = tend - r1 < so ? tend - r1 : so;
            const bnf_rsmp_step st = bnf_rsmp_step_of(row, sp, r1, cnt, stride);
            if (st.md) { /* uniform over the workgroup */
                uint4 v[RS_LOAD_PASSES];
#pragma unroll
                for (int u = 0; u < (int)RS_LOAD_PASSES; u++) {
                    const uint32_t j = (uint32_t)u * RS_THREADS + t;
                    v[u] = make_uint4(0u, 0u, 0u, 0u);
                    if (j < st.blk.nblk) v[u] = *(const uint4 *)(pcm + bnf_f32_block_addr(st.blk, j, last_blk));
                }
                __syncthreads(); /* the previous step's store buffers and stage have been read */
#pragma unroll
                for (int u = 0; u < (int)RS_LOAD_PASSES; u++) {
                    const uint32_t j = (uint32_t)u * RS_THREADS + t;
                    if (j < st.blk.nblk) raw4[j] = v[u];
                }
                __syncthreads();
                if (cv.mono) {
                    for (uint32_t u = t; u < st.span; u += RS_THREADS) stage[u] = bnf_rsmp_unpack(raw, st, cv, unit, u, 0);
                } else {
                    const uint32_t nel = st.span * channels;
                    for (uint32_t e = t; e < nel; e += RS_THREADS) {
                        const uint32_t u = bnf_f32_frame_of(e, magic), c = e - u * channels;
                        stage[c * cv.pitch + u] = bnf_rsmp_unpack(raw, st, cv, unit, u, c);
                    }
                }
            }
            __syncthreads(); /* the stage (and the table) is written, the raw blocks are read */
            for (uint32_t c = 0; c < planes; c++) {
                float *const D = out + ((uint64_t)s * planes + c) * plane_pitch + r1;
                const uint32_t a = (uint32_t)((uintptr_t)D >> 2) & 3u;
                float *const yb = ybuf + (c & 1u) * BNF_RSMP_YBUF;
                uint32_t head, ngroups;
                bnf_f32_split(a, cnt, head, ngroups);
                for (uint32_t p = t; p < cnt; p += RS_THREADS) yb[a + p] = bnf_rsmp_value(ltaps, tap_pitch, stage, st, sp, cv.pitch, c, p);
                __syncthreads(); /* also: the buffer the plane after this one writes has been read */
                const uint32_t first = a + head; /* a multiple of 4, or cnt < 4 and no group */
                for (uint32_t q = t; q < ngroups; q += RS_THREADS) {
                    const bnf_rsmp_f4 f = *(const bnf_rsmp_f4 *)(yb + first + 4u * q);
                    *(float4 *)(D + head + 4u * q) = make_float4(f[0], f[1], f[2], f[3]);
                }
                const uint32_t behind = head + 4u * ngroups; /* the singles: lanes 0..2 and 64..66 */
                if (t < head) D[t] = yb[a + t];
                if (t >= 64u && behind + (t - 64u) < cnt) D[behind + (t - 64u)] = yb[a + behind + (t - 64u)];
            }
        }
    }
}

extern "C" hipError_t bnf_launch_gather_f32_rs(const uint8_t *pcm, uint64_t pcm_bytes, uint32_t stride, uint32_t unit,
                                               uint32_t bps, uint32_t channels, uint32_t flags, const bnf_window *windows,
                                               uint32_t nstreams, const bnf_rsmp_spec *spec, const float *taps,
                                               uint32_t row_out, uint64_t plane_pitch, float *out, uint32_t *status,
                                               hipStream_t s) {
    if (!stride || channels < 1 || channels > 8 || unit * channels != stride || unit < 2 || unit > 4 || bps < 1 || bps > 32 ||
        bnf_rsmp_spec_refusal(*spec, row_out))
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(status, 0, 4 * sizeof(uint32_t), s);
    if (e != hipSuccess || !nstreams) return e;
    const uint32_t lds = rs_lds_bytes(*spec);
    if (lds > 64u * 1024u) { /* above the default limit of a launch's dynamic LDS */
        e = hipFuncSetAttribute((const void *)k_gather_f32_rs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    /* enough workgroups for every CU to hold several, few enough that each loads the table for many tiles */
    const uint32_t ntiles = (row_out + BNF_RSMP_TILE - 1u) / BNF_RSMP_TILE;
    const uint32_t want = (4096u + nstreams - 1u) / nstreams;
    const uint32_t gy = ntiles < 1 ? 1 : ntiles < want ? ntiles : want;
    const dim3 grid(nstreams, gy > 65535u ? 65535u : gy), block(RS_THREADS);
    hipLaunchKernelGGL(k_gather_f32_rs, grid, block, lds, s, pcm, pcm_bytes, stride, unit, bps, channels, flags, windows,
                       *spec, taps, row_out, plane_pitch, out, status);
    return hipGetLastError();
}
