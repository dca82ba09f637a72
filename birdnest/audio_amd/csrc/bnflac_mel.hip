/*
 * bnflac_mel.hip -- k_gather_mel (bnflac_gather_ranges_mel): the windows of a decoded selection as
 * mel (or power) spectrogram planes.  The rule, and every address and value the kernel computes, is
 * bnf_mel.h's (on top of bnf_pcm_f32.h's window check, block loads, sample fetch and conversions).
 * No CRC tables, no g_stats, no ablate word.
 *
 * One workgroup per window (blockIdx.x) walks the row's tiles of BNF_MEL_TF = 32 frames (blockIdx.y,
 * grid strided).  All LDS is the dynamic region, laid out by bnf_mel_plan_of, every part a multiple
 * of 16 bytes: the twiddles and the band weights (loaded once per workgroup), the checked bands
 * (first | nb << 16, woff), the raw blocks of a step, G work areas of N complex floats, and ybuf.
 * Per tile, pass of rows and plane:
 *   load    per step of sf frames, the aligned 16-byte source blocks of the step's span, one per lane
 *           and pass, four passes issued before the first is stored (ds_write_b128).
 *   frames  G frames at a time, tpf = 256 / G lanes each.  Lane <-> sample: fetched from the raw
 *           blocks, converted, weighted (the window comes from the table in global memory, an L1 hit)
 *           and stored at its bit-reversed slot.  Then the stages, two per pass over the work area
 *           (bnf_mel_pass2: lane <-> the four elements two stages couple; one stage alone first when
 *           log2 N is odd), a barrier after each.
 *   rows    with bands: P in place in the real slots, then lane <-> band, its fmaf chain to ybuf at
 *           (band, column).  Without: lane <-> bin, P straight to ybuf.  32 lanes at one column are
 *           32 rows 33 floats apart: 32 banks.
 *   store   lane <-> piece (row, j): the aligned 16-byte group 4j - a of the row's 32 floats out of
 *           ybuf (or +0.0f behind the tile's valid frames) as one 16-byte global store, the ragged
 *           pieces as single floats.  Nine consecutive lanes cover one row's run.
 * Trip counts: see bnf_mel.h.  A window's fields only enter through bnf_mel_window.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bnf_mel.h"
#include "bnflac_launch.h"

#define MEL_THREADS BNF_MEL_THREADS
#define MEL_LOAD_PASSES 4

static_assert(sizeof(bnf_window) == 32 && sizeof(bnf_mel_spec) == 32, "record sizes");

/* status: [0] bit 0 a window outside pcm_bytes, bit 1 a bad band, [1] such windows, [2] windows with
 * more frames than row_frames, [3] bad bands */
__global__ __launch_bounds__(MEL_THREADS) void k_gather_mel(const uint8_t *__restrict__ pcm, uint64_t pcm_bytes, uint32_t stride,
                                                            uint32_t unit, uint32_t bps, uint32_t channels, uint32_t flags,
                                                            const bnf_window *__restrict__ windows, bnf_mel_spec sp,
                                                            const float *__restrict__ tab, const uint32_t *__restrict__ bands,
                                                            uint32_t row_frames, uint64_t frame_pitch, float *__restrict__ out,
                                                            uint32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const bnf_f32_conv cv = bnf_f32_conv_of(channels, bps, flags);
    const uint32_t planes = cv.mono ? 1u : channels;
    const bnf_mel_plan pl = bnf_mel_plan_of(sp, stride, planes);
    const uint32_t N = pl.N;
    float *const ltw = (float *)smem;
    float *const lwt = (float *)(smem + pl.off_wt);
    uint32_t *const lb = (uint32_t *)(smem + pl.off_bands);
    uint4 *const raw4 = (uint4 *)(smem + pl.off_raw);
    const uint32_t *const raw = (const uint32_t *)raw4;
    float *const ybuf = (float *)(smem + pl.off_ybuf);
    const uint32_t g = t / pl.tpf, lt = t - g * pl.tpf;
    float *const v = (float *)(smem + pl.off_work) + 2u * N * g;
    const bnf_mel_row row = bnf_mel_window(windows[s].pcm_first, windows[s].nsamples, pcm_bytes, stride, sp, row_frames);
    if (blockIdx.y == 0 && t == 0) {
        if (row.bad) {
            atomicOr(&status[0], BNF_F32_BAD_WINDOW);
            atomicAdd(&status[1], 1u);
        } else if (row.cut) {
            atomicAdd(&status[2], 1u);
        }
    }
    const bool counts = blockIdx.x == 0 && blockIdx.y == 0; /* the bad bands, once per launch */
    if (row.ncopy || counts) {                               /* uniform over the workgroup: the tables */
        for (uint32_t m = t; m < sp.n_mels; m += MEL_THREADS) {
            uint32_t first, woff, nb;
            if (bnf_mel_band_of(bands, m, sp, first, woff, nb) && counts) {
                atomicOr(&status[0], BNF_MEL_BAD_BAND);
                atomicAdd(&status[3], 1u);
            }
            lb[2u * m] = first | (nb << 16);
            lb[2u * m + 1u] = woff;
        }
        for (uint32_t q = t; q < N / 4u; q += MEL_THREADS) ((float4 *)ltw)[q] = ((const float4 *)(tab + N))[q];
        for (uint32_t i = t; i < sp.n_weights; i += MEL_THREADS) lwt[i] = tab[2u * N + i];
    }
    const uint64_t last_blk = bnf_f32_last_block(pcm_bytes);
    const uint32_t ntiles = (row_frames + BNF_MEL_TF - 1u) / BNF_MEL_TF;
    for (uint32_t tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
        const uint32_t t0 = tile * BNF_MEL_TF;
        const uint32_t cnt = row_frames - t0 < BNF_MEL_TF ? row_frames - t0 : BNF_MEL_TF;
        const uint32_t mdt = row.ncopy > t0 ? (row.ncopy - t0 < cnt ? row.ncopy - t0 : cnt) : 0u;
        for (uint32_t r0 = 0; r0 < pl.rows; r0 += pl.pass_rows) {
            const uint32_t nrow = pl.rows - r0 < pl.pass_rows ? pl.rows - r0 : pl.pass_rows;
            for (uint32_t c = 0; c < planes; c++) {
                for (uint32_t r1 = t0; r1 < t0 + mdt; r1 += pl.sf) { /* uniform over the workgroup */
                    const uint32_t scnt = t0 + cnt - r1 < pl.sf ? t0 + cnt - r1 : pl.sf;
                    const bnf_mel_step st = bnf_mel_step_of(row, sp, r1, scnt, stride);
                    __syncthreads(); /* the previous step's frames have read the raw blocks (and the tables are written) */
                    for (uint32_t j0 = 0; j0 < st.blk.nblk; j0 += MEL_LOAD_PASSES * MEL_THREADS) {
                        uint4 ld[MEL_LOAD_PASSES];
#pragma unroll
                        for (int u = 0; u < MEL_LOAD_PASSES; u++) {
                            const uint32_t j = j0 + (uint32_t)u * MEL_THREADS + t;
                            ld[u] = make_uint4(0u, 0u, 0u, 0u);
                            if (j < st.blk.nblk) ld[u] = *(const uint4 *)(pcm + bnf_f32_block_addr(st.blk, j, last_blk));
                        }
#pragma unroll
                        for (int u = 0; u < MEL_LOAD_PASSES; u++) {
                            const uint32_t j = j0 + (uint32_t)u * MEL_THREADS + t;
                            if (j < st.blk.nblk) raw4[j] = ld[u];
                        }
                    }
                    __syncthreads();
                    for (uint32_t f0 = 0; f0 < st.md; f0 += pl.G) {
                        const uint32_t f = f0 + g;
                        const bool on = f < st.md;
                        if (on)
                            for (uint32_t i = lt; i < N; i += pl.tpf) {
                                const uint32_t d = bnf_mel_brev(i, pl.log2n);
                                const float u = bnf_mel_input(tab[i], bnf_mel_x(raw, st, cv, unit, f * sp.hop + i, c));
                                *(float2 *)(v + 2u * d) = make_float2(u, 0.0f);
                            }
                        __syncthreads();
                        uint32_t lh = 0;
                        if (pl.log2n & 1u) {
                            if (on)
                                for (uint32_t q = lt; q < N / 2u; q += pl.tpf) bnf_mel_pass1(v, ltw, pl.log2n, 0, q);
                            __syncthreads();
                            lh = 1;
                        }
                        for (; lh < pl.log2n; lh += 2u) {
                            if (on)
                                for (uint32_t q = lt; q < N / 4u; q += pl.tpf) bnf_mel_pass2(v, ltw, pl.log2n, lh, q);
                            __syncthreads();
                        }
                        const uint32_t col = r1 - t0 + f;
                        if (sp.n_mels) {
                            if (on)
                                for (uint32_t k = lt; k <= N / 2u; k += pl.tpf) v[2u * k] = bnf_mel_power(v[2u * k], v[2u * k + 1u]);
                            __syncthreads();
                            if (on)
                                for (uint32_t m = lt; m < nrow; m += pl.tpf) {
                                    const uint32_t w0 = lb[2u * m];
                                    ybuf[m * BNF_MEL_YPITCH + col] = bnf_mel_band(lwt + lb[2u * m + 1u], v, w0 & 0xffffu, w0 >> 16);
                                }
                        } else if (on) {
                            for (uint32_t k = r0 + lt; k < r0 + nrow; k += pl.tpf)
                                ybuf[(k - r0) * BNF_MEL_YPITCH + col] = bnf_mel_power(v[2u * k], v[2u * k + 1u]);
                        }
                        __syncthreads(); /* the work areas are free for the next frames */
                    }
                }
                __syncthreads(); /* ybuf is written */
                for (uint32_t it = t; it < nrow * BNF_MEL_PIECES; it += MEL_THREADS) {
                    const uint32_t r = it / BNF_MEL_PIECES, j = it - r * BNF_MEL_PIECES;
                    float *const D = out + (((uint64_t)s * planes + c) * pl.rows + r0 + r) * frame_pitch + t0;
                    const int32_t p0 = bnf_mel_piece((uint32_t)((uintptr_t)D >> 2), j);
                    float f[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int32_t p = p0 + e;
                        f[e] = p >= 0 && (uint32_t)p < mdt ? ybuf[r * BNF_MEL_YPITCH + (uint32_t)p] : 0.0f;
                    }
                    if (p0 >= 0 && (uint32_t)p0 + 3u < cnt) {
                        *(float4 *)(D + p0) = make_float4(f[0], f[1], f[2], f[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            if (p0 + e >= 0 && (uint32_t)(p0 + e) < cnt) D[p0 + e] = f[e];
                    }
                }
                __syncthreads(); /* ybuf has been read */
            }
        }
    }
}

extern "C" hipError_t bnf_launch_gather_mel(const uint8_t *pcm, uint64_t pcm_bytes, uint32_t stride, uint32_t unit,
                                            uint32_t bps, uint32_t channels, uint32_t flags, const bnf_window *windows,
                                            uint32_t nstreams, const bnf_mel_spec *spec, const float *tab, const uint32_t *bands,
                                            uint32_t row_frames, uint64_t frame_pitch, float *out, uint32_t *status,
                                            hipStream_t s) {
    if (!stride || channels < 1 || channels > 8 || unit * channels != stride || unit < 2 || unit > 4 || bps < 1 || bps > 32 ||
        bnf_mel_spec_refusal(*spec, row_frames, frame_pitch) || (spec->n_mels && !bands))
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(status, 0, 4 * sizeof(uint32_t), s);
    if (e != hipSuccess || !nstreams) return e;
    const bnf_mel_plan pl = bnf_mel_plan_of(*spec, stride, (flags & BNF_F32_MONO) ? 1u : channels);
    if (pl.lds_bytes > 64u * 1024u) { /* above the default limit of a launch's dynamic LDS */
        e = hipFuncSetAttribute((const void *)k_gather_mel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
        if (e != hipSuccess) return e;
    }
    /* enough workgroups for every CU to hold several, few enough that each loads the tables for many tiles */
    const uint32_t ntiles = (row_frames + BNF_MEL_TF - 1u) / BNF_MEL_TF;
    const uint32_t want = (4096u + nstreams - 1u) / nstreams;
    const uint32_t gy = ntiles < 1 ? 1 : ntiles < want ? ntiles : want;
    const dim3 grid(nstreams, gy > 65535u ? 65535u : gy), block(MEL_THREADS);
    hipLaunchKernelGGL(k_gather_mel, grid, block, pl.lds_bytes, s, pcm, pcm_bytes, stride, unit, bps, channels, flags, windows,
                       *spec, tab, bands, row_frames, frame_pitch, out, status);
    return hipGetLastError();
}
