/*
 * bnf_resample.h -- the rule of bnflac_gather_ranges_f32_rs: the windows of a decoded selection as
 * float32 channel planes at another sample rate, by a polyphase FIR whose taps the caller passes.
 * Everything k_gather_f32_rs (bnflac_resample.hip) computes is a function of this header, callable
 * from host and device; bnf_gather_f32_rs_host below walks the same tiles and steps with the same
 * functions, one "lane" after the other, so bnflac_gather_ranges_f32_rs_host and the kernel are
 * the same code, as bnf_pcm_f32.h is for the plain gather.  The header needs no HIP: a plain C++
 * compiler takes it too (tools/gather_rs_sanitize.cpp builds it with the sanitizers).  The design of
 * a table (bnf_rsmp_design) and the source window of a run of outputs (bnf_rsmp_request) are host code.
 *
 * The rule.  spec = {up = L, down = M, taps = K, out_first}, h = the table of L * K float32,
 * h[phase][k] at phase * K + k.  Window s passes bnf_f32_window's check or is bad (nothing read,
 * zero planes, counted).  n = nsamples of a good window, x[i] for 0 <= i < n the float
 * bnflac_gather_ranges_f32 specifies for sample frame i of the plane (bnf_f32_cvt, or
 * bnf_f32_cvt_mono with BNF_F32_MONO), x[i] = +0.0f elsewhere.
 *   n_out = max(0, ceil(n L / M) - out_first), ncopy = min(n_out, row_out)
 *   row position r < ncopy is output j = r + out_first: q = floor(j M / L), phase = (j M) mod L,
 *   c0 = K / 2 - 1; a[0..3] = +0.0f; for k = 0 .. K - 1 ascending
 *       a[k & 3] = fmaf(h[phase][k], x[q + k - c0], a[k & 3]);
 *   the value is (a[0] + a[1]) + (a[2] + a[3]); positions [ncopy, row_out) are +0.0f.
 * Output j exists (j < ceil(n L / M)) exactly when floor(j M / L) < n, which is how ncopy is found
 * here without the product n L.
 *
 * Terms outside the window.  For a finite tap, h * (+0.0f) is +0 or -0 exactly, and fmaf then
 * returns a + (+-0): a itself when a is not a zero, +0 when a is +0.  An accumulator starts at +0
 * and can only become -0 through a product so small that it underflows to -0 on a zero accumulator.
 * So with finite taps and no such underflow, skipping the terms whose x lies outside [0, n) gives
 * the same bits.  This code does not use the licence: it stages the +0.0f values and runs all K
 * terms for every output, so the value is the formula's for any table, NaNs included, and no lane
 * has a trip count of its own.
 *
 * Tiles and steps.  A row is cut into tiles of BNF_RSMP_TILE outputs (one workgroup takes a tile of
 * one window and writes it to every plane).  A tile is worked in steps of bnf_rsmp_step_outputs()
 * consecutive outputs: as many as keep the source span q_last - q_first + K of a step within
 * bnf_f32_tile_frames(channels) sample frames (at least K, so one output always fits; one step per
 * tile for the usual ratios, more when M / L is large), spread evenly over the tile.  Per step:
 *   span     sbase = q_first - c0 (may be negative), `span` sample frames from it; those inside
 *            [0, n) are [lo, hi), and their bytes lie in the aligned 16-byte blocks bnf_rsmp_step_of
 *            names, all below round_up(pcm_bytes, 16) for a checked window (bnf_f32_block_addr
 *            clamps on top of that).  The blocks are staged raw.
 *   unpack   every frame position u < span of every plane gets its float in the stage at
 *            c * bnf_f32_pitch(channels) + u: the conversion of the fetched sample(s), or +0.0f
 *            outside [lo, hi).
 *   filter   output p of the step (j = j_first + p): t = ph_first + p * M fits 32 bits;
 *            u = t / L is q - q_first, phase = t mod L; bnf_rsmp_fir(h row, stage + c * pitch + u, K).
 *   store    the step's values of a plane go through a small buffer to aligned groups of 4 floats
 *            with single floats at the ragged ends (bnf_f32_split).
 * Trip counts: steps by BNF_RSMP_TILE, blocks and samples by the span, taps by K, tiles by row_out.
 * A window's fields only enter through bnf_f32_window's check and n.
 */
#ifndef BNF_RESAMPLE_H
#define BNF_RESAMPLE_H

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bnf_pcm_f32.h"

#define BNF_RSMP_TILE 1024u        /* outputs of a tile (per plane) */
#define BNF_RSMP_MAX_RATIO 65535u  /* up, down at most */
#define BNF_RSMP_MAX_TAPS 512u     /* taps per phase at most */
#define BNF_RSMP_MAX_TABLE 16384u  /* up * taps at most: 64 KiB of float32 */
#define BNF_RSMP_YBUF (BNF_RSMP_TILE + 4u) /* floats of one store buffer: a step's outputs behind up to 3 slots of phase */

typedef struct {
    uint32_t up, down;  /* L, M: coprime, 1..65535 */
    uint32_t taps;      /* K: taps per phase, a multiple of 4 in 4..512 */
    uint32_t out_first; /* output index of the window that lands in row position 0 */
} bnf_rsmp_spec;          /* bnflac_resample_spec */

/* 4 floats, 16-byte aligned: a vector type, so that a read of it stays one 16-byte read */
typedef float bnf_rsmp_f4 __attribute__((vector_size(16)));

BNF_F32_HD inline uint32_t bnf_rsmp_gcd(uint32_t a, uint32_t b) {
    while (b) {
        const uint32_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

/* Why a spec (with row_out) is refused, or a null pointer. */
BNF_F32_HD inline const char *bnf_rsmp_spec_refusal(const bnf_rsmp_spec &sp, uint32_t row_out) {
    if (sp.up < 1 || sp.up > BNF_RSMP_MAX_RATIO || sp.down < 1 || sp.down > BNF_RSMP_MAX_RATIO) return "up and down must be 1..65535";
    if (bnf_rsmp_gcd(sp.up, sp.down) != 1) return "up and down must be coprime";
    if (sp.taps < 4 || sp.taps > BNF_RSMP_MAX_TAPS || (sp.taps & 3u)) return "taps must be a multiple of 4 in 4..512";
    if (sp.up * sp.taps > BNF_RSMP_MAX_TABLE) return "up * taps must not exceed 16384";
    if (row_out >> 31) return "row_out must be below 2^31";
    if (sp.out_first >> 31) return "out_first must be below 2^31";
    return nullptr;
}

/* Floats between the rows of two phases where the table is staged: K or K + 4, so that pitch / 4 is
 * odd.  A 16-lane group of a 16-byte read then takes 16 different banks when its lanes' phases
 * differ modulo 16 (bank of float a: a mod 64, so row * pitch / 4 mod 16 names the group of 4 banks). */
BNF_F32_HD inline uint32_t bnf_rsmp_tap_pitch(uint32_t K) { return (K >> 2) & 1u ? K : K + 4u; }

/* Outputs of one step: a function of the call, not of a window. */
BNF_F32_HD inline uint32_t bnf_rsmp_step_outputs(const bnf_rsmp_spec &sp, uint32_t channels) {
    const uint32_t F = bnf_f32_tile_frames(channels); /* >= 512 >= K */
    /* q_last - q_first <= ceil((so - 1) M / L), which is <= F - K when (so - 1) M <= (F - K) L */
    const uint64_t most = (uint64_t)(F - sp.taps) * sp.up / sp.down + 1u;
    const uint32_t so = most < BNF_RSMP_TILE ? (uint32_t)most : BNF_RSMP_TILE;
    const uint32_t nsteps = (BNF_RSMP_TILE + so - 1u) / so;
    return (BNF_RSMP_TILE + nsteps - 1u) / nsteps; /* not above so */
}

/* One window against the PCM and the spec. */
typedef struct {
    uint64_t src0;  /* byte of the PCM at which the window's first sample frame starts (0 when n is 0) */
    uint64_t n;     /* sample frames of the window (0 when bad) */
    uint32_t ncopy; /* row positions that carry values */
    uint32_t bad, cut;
} bnf_rsmp_row;

BNF_F32_HD inline bnf_rsmp_row bnf_rsmp_window(uint64_t pcm_first, uint64_t nsamples, uint64_t pcm_bytes, uint32_t stride,
                                           const bnf_rsmp_spec &sp, uint32_t row_out) {
    const bnf_f32_row w = bnf_f32_window(pcm_first, nsamples, pcm_bytes, stride, 1u);
    bnf_rsmp_row r;
    r.bad = w.bad;
    r.n = w.bad ? 0u : nsamples;
    r.src0 = w.src0;
    const uint64_t j_end = (uint64_t)sp.out_first + row_out; /* < 2^32, so j M < 2^48 */
    uint64_t total;                                          /* min(ceil(n L / M), j_end + 1) */
    if (r.n >= ((uint64_t)1 << 48))
        total = j_end + 1u; /* floor(j M / L) < 2^48 <= n for every j <= j_end */
    else {
        total = (r.n * sp.up + sp.down - 1u) / sp.down; /* n L < 2^64 */
        if (total > j_end) total = j_end + 1u;
    }
    r.cut = !r.bad && total > j_end ? 1u : 0u;
    r.ncopy = total > sp.out_first ? (uint32_t)((total < j_end ? total : j_end) - sp.out_first) : 0u;
    return r;
}

/* The step of a row that starts at row position r1 and covers cnt positions (within one tile). */
typedef struct {
    bnf_f32_tile blk;  /* blk0, nblk, phase: the aligned blocks of the frames [lo, hi) (nblk 0 when md is 0) */
    uint32_t md;       /* positions of the step that carry values: the first md */
    uint32_t span;     /* staged frame positions u = 0 .. span - 1, position u is source frame sbase + u */
    uint32_t z;        /* positions in front of frame lo: lo - sbase */
    uint32_t nin;      /* frames inside the window: hi - lo, at position z */
    uint32_t ph_first; /* (j_first M) mod L */
} bnf_rsmp_step;

BNF_F32_HD inline bnf_rsmp_step bnf_rsmp_step_of(const bnf_rsmp_row &row, const bnf_rsmp_spec &sp, uint32_t r1, uint32_t cnt,
                                             uint32_t stride) {
    bnf_rsmp_step st;
    st.md = row.ncopy > r1 ? (row.ncopy - r1 < cnt ? row.ncopy - r1 : cnt) : 0u;
    st.blk.blk0 = 0;
    st.blk.nblk = st.blk.phase = st.blk.ndata = st.blk.nt = 0;
    st.span = st.z = st.nin = st.ph_first = 0;
    if (!st.md) return st;
    const uint32_t c0 = sp.taps / 2u - 1u;
    const uint64_t jm_first = ((uint64_t)sp.out_first + r1) * sp.down, jm_last = jm_first + (uint64_t)(st.md - 1u) * sp.down;
    const uint64_t q_first = jm_first / sp.up, q_last = jm_last / sp.up; /* q_last < n: the output exists */
    st.ph_first = (uint32_t)(jm_first - q_first * sp.up);
    st.span = (uint32_t)(q_last - q_first) + sp.taps;
    st.z = q_first < c0 ? c0 - (uint32_t)q_first : 0u;
    const uint64_t lo = q_first < c0 ? 0u : q_first - c0;
    const uint64_t end = q_first + (st.span - c0); /* sbase + span, not negative: span > c0 */
    const uint64_t hi = end < row.n ? end : row.n;
    st.nin = (uint32_t)(hi - lo);
    const uint64_t begin = row.src0 + lo * stride, stop = row.src0 + hi * stride;
    st.blk.blk0 = begin & ~(uint64_t)15;
    st.blk.phase = (uint32_t)begin & 15u;
    st.blk.nblk = (uint32_t)((stop - st.blk.blk0 + 15u) >> 4);
    st.blk.ndata = st.blk.nt = st.nin;
    return st;
}

/* The float of stage slot e of a step (unpack).  Per channel: e = u * channels + c over span * channels
 * slots, stored at c * pitch + u.  Mono: e = u over span slots, stored at u. */
BNF_F32_HD inline float bnf_rsmp_unpack(const uint32_t *raw, const bnf_rsmp_step &st, const bnf_f32_conv &cv, uint32_t unit,
                                      uint32_t u, uint32_t c) {
    if (u < st.z || u - st.z >= st.nin) return 0.0f;
    const uint32_t at = st.blk.phase + (u - st.z) * cv.channels * unit;
    if (!cv.mono) return bnf_f32_cvt(bnf_f32_fetch(raw, at + c * unit, unit), cv.k);
    int64_t S = 0;
    for (uint32_t ch = 0; ch < cv.channels; ch++) S += bnf_f32_fetch(raw, at + ch * unit, unit);
    return bnf_f32_cvt_mono(S, cv.kd, cv.channels);
}

/* One output: K taps (a multiple of 4) from h, 16-byte aligned on the device, over x[0 .. K). */
BNF_F32_HD inline float bnf_rsmp_fir(const float *h, const float *x, uint32_t K) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4 /* the reads of four groups in flight before the first is used */
#endif
    for (uint32_t k = 0; k < K; k += 4u) {
#if defined(__HIP_DEVICE_COMPILE__)
        const bnf_rsmp_f4 hv = *(const bnf_rsmp_f4 *)(h + k);
#else
        bnf_rsmp_f4 hv;
        memcpy(&hv, h + k, sizeof hv);
#endif
        a0 = fmaf(hv[0], x[k], a0);
        a1 = fmaf(hv[1], x[k + 1u], a1);
        a2 = fmaf(hv[2], x[k + 2u], a2);
        a3 = fmaf(hv[3], x[k + 3u], a3);
    }
    return (a0 + a1) + (a2 + a3);
}

/* Output p of a step on plane c: the row of its phase (rows `tap_pitch` floats apart) over the stage. */
BNF_F32_HD inline float bnf_rsmp_value(const float *taps, uint32_t tap_pitch, const float *stage, const bnf_rsmp_step &st,
                                     const bnf_rsmp_spec &sp, uint32_t pitch, uint32_t c, uint32_t p) {
    if (p >= st.md) return 0.0f;
    const uint32_t t = st.ph_first + p * sp.down; /* < 2^16 + 2^10 2^16 */
    const uint32_t u = t / sp.up, phase = t - u * sp.up;
    return bnf_rsmp_fir(taps + (size_t)phase * tap_pitch, stage + c * pitch + u, sp.taps);
}

/* The whole call on host memory: the tiles, steps, loads, staging, store buffer and stores of
 * k_gather_f32_rs, one lane after the other.  The raw blocks, the stage and the store buffer of a
 * step are heap allocations of exactly the sizes the functions above name.  -1 when out of
 * memory, else 0. */
inline int bnf_gather_f32_rs_host(const uint8_t *pcm, uint64_t pcm_bytes, uint32_t stride, uint32_t unit, uint32_t bps,
                                  uint32_t channels, uint32_t flags, const bnf_window *windows, uint32_t nstreams,
                                  const bnf_rsmp_spec &sp, const float *taps, uint32_t row_out, uint64_t plane_pitch, float *out,
                                  uint32_t status[4]) {
    status[0] = status[1] = status[2] = status[3] = 0;
    const bnf_f32_conv cv = bnf_f32_conv_of(channels, bps, flags);
    const uint32_t magic = bnf_f32_magic(channels), planes = cv.mono ? 1u : channels;
    const uint32_t so = bnf_rsmp_step_outputs(sp, channels);
    const uint64_t last_blk = bnf_f32_last_block(pcm_bytes);
    for (uint32_t s = 0; s < nstreams; s++) {
        const bnf_rsmp_row row = bnf_rsmp_window(windows[s].pcm_first, windows[s].nsamples, pcm_bytes, stride, sp, row_out);
        if (row.bad) {
            status[0] |= BNF_F32_BAD_WINDOW;
            status[1]++;
        }
        status[2] += row.cut;
        for (uint32_t t0 = 0; t0 < row_out; t0 += BNF_RSMP_TILE) {
            const uint32_t tend = row_out - t0 < BNF_RSMP_TILE ? row_out : t0 + BNF_RSMP_TILE;
            for (uint32_t r1 = t0; r1 < tend; r1 += so) {
                const uint32_t cnt = tend - r1 < so ? tend - r1 : so;
                const bnf_rsmp_step st = bnf_rsmp_step_of(row, sp, r1, cnt, stride);
                uint32_t *raw = nullptr;
                float *stage = nullptr;
                float *ybuf = (float *)malloc(sizeof(float) * (cnt + 3u));
                if (st.md) {
                    raw = (uint32_t *)malloc(16u * (size_t)st.blk.nblk);
                    stage = (float *)malloc(sizeof(float) * ((size_t)(planes - 1u) * cv.pitch + st.span));
                }
                if (!ybuf || (st.md && (!raw || !stage))) {
                    free(raw);
                    free(stage);
                    free(ybuf);
                    return -1;
                }
                if (st.md) {
                    for (uint32_t j = 0; j < st.blk.nblk; j++)
                        memcpy(raw + 4u * j, pcm + bnf_f32_block_addr(st.blk, j, last_blk), 16);
                    if (cv.mono)
                        for (uint32_t u = 0; u < st.span; u++) stage[u] = bnf_rsmp_unpack(raw, st, cv, unit, u, 0);
                    else
                        for (uint32_t e = 0; e < st.span * channels; e++) {
                            const uint32_t u = bnf_f32_frame_of(e, magic), c = e - u * channels;
                            stage[c * cv.pitch + u] = bnf_rsmp_unpack(raw, st, cv, unit, u, c);
                        }
                }
                for (uint32_t c = 0; c < planes; c++) {
                    float *const D = out + ((uint64_t)s * planes + c) * plane_pitch + r1;
                    const uint32_t a = (uint32_t)((uintptr_t)D >> 2) & 3u;
                    uint32_t head, ngroups;
                    bnf_f32_split(a, cnt, head, ngroups);
                    for (uint32_t p = 0; p < cnt; p++) ybuf[a + p] = bnf_rsmp_value(taps, sp.taps, stage, st, sp, cv.pitch, c, p);
                    for (uint32_t p = 0; p < head; p++) D[p] = ybuf[a + p];
                    for (uint32_t q = 0; q < ngroups; q++) memcpy(D + head + 4u * q, ybuf + a + head + 4u * q, 16);
                    for (uint32_t p = head + 4u * ngroups; p < cnt; p++) D[p] = ybuf[a + p];
                }
                free(raw);
                free(stage);
                free(ybuf);
            }
        }
    }
    return 0;
}

/* ---------------------------------------------------------------- design and requests (host only) */

inline double bnf_rsmp_i0(double x) { /* modified Bessel function of the first kind, order 0: its power series */
    const double y = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 1000; k++) {
        term *= y / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-17) break;
    }
    return sum;
}

inline double bnf_rsmp_sinc(double x) { /* sin(pi x) / (pi x) */
    const double pi = 3.14159265358979323846;
    return x == 0.0 ? 1.0 : sin(pi * x) / (pi * x);
}

/* The spec of a Kaiser-windowed sinc design (out_first = 0).  -> null, or why there is none. */
inline const char *bnf_rsmp_design_spec(uint32_t rate_in, uint32_t rate_out, double zeros, bnf_rsmp_spec &sp, uint64_t &K_needed) {
    sp.up = sp.down = sp.taps = sp.out_first = 0;
    K_needed = 0;
    if (!rate_in || !rate_out) return "a rate is zero";
    const uint32_t g = bnf_rsmp_gcd(rate_in, rate_out);
    const uint32_t L = rate_out / g, M = rate_in / g;
    if (L > BNF_RSMP_MAX_RATIO || M > BNF_RSMP_MAX_RATIO) return "up and down must be 1..65535";
    sp.up = L;
    sp.down = M;
    if (L == 1 && M == 1) {
        sp.taps = 4;
        K_needed = 4;
        return nullptr;
    }
    const double s = L < M ? (double)L / (double)M : 1.0;
    const double half = ceil(zeros / s);
    if (!(half < 1e6)) return "zeros is too large";
    K_needed = ((uint64_t)(2.0 * half) + 3u) & ~(uint64_t)3;
    if (K_needed < 4) K_needed = 4;
    if (K_needed > BNF_RSMP_MAX_TAPS || L * K_needed > BNF_RSMP_MAX_TABLE) return "the table is over the limits";
    sp.taps = (uint32_t)K_needed;
    return nullptr;
}

/* The table of a design: taps[phase * K + k], sp.up * sp.taps floats. */
inline void bnf_rsmp_design_taps(const bnf_rsmp_spec &sp, double rolloff, double beta, float *taps) {
    const uint32_t L = sp.up, M = sp.down, K = sp.taps;
    if (L == 1 && M == 1) {
        taps[0] = taps[2] = taps[3] = 0.0f;
        taps[1] = 1.0f;
        return;
    }
    const double s = L < M ? (double)L / (double)M : 1.0, fc = rolloff * s;
    const double c0 = (double)(K / 2u - 1u), halfK = (double)(K / 2u), i0b = bnf_rsmp_i0(beta);
    double g[BNF_RSMP_MAX_TAPS];
    for (uint32_t ph = 0; ph < L; ph++) {
        double sum = 0.0;
        for (uint32_t k = 0; k < K; k++) {
            const double tau = ((double)k - c0) - (double)ph / (double)L;
            const double r = tau / halfK;
            const double w = fabs(tau) < halfK ? bnf_rsmp_i0(beta * sqrt(1.0 - r * r)) / i0b : 0.0;
            g[k] = fc * bnf_rsmp_sinc(fc * tau) * w;
            sum += g[k];
        }
        for (uint32_t k = 0; k < K; k++) taps[(size_t)ph * K + k] = (float)(g[k] / sum);
    }
}

/* The source window and out_first for outputs [j0, j0 + n_out) of a stream on the output-rate grid,
 * with the filter's whole support on both sides: b = max(0, floor(j0 M / L) - c0) / M,
 * first_sample = M b (so that the window's output grid is the stream's), out_first = j0 - L b,
 * nsamples = floor((j0 + n_out - 1) M / L) + K / 2 + 1 - first_sample (0 for n_out = 0).
 * j0 + n_out < 2^47. */
inline void bnf_rsmp_request(const bnf_rsmp_spec &sp, uint64_t j0, uint64_t n_out, uint64_t &first_sample, uint64_t &nsamples,
                           uint64_t &out_first) {
    const uint64_t c0 = sp.taps / 2u - 1u, q0 = j0 * sp.down / sp.up;
    const uint64_t b = (q0 > c0 ? q0 - c0 : 0u) / sp.down;
    first_sample = (uint64_t)sp.down * b;
    out_first = j0 - (uint64_t)sp.up * b;
    nsamples = n_out ? (j0 + n_out - 1u) * sp.down / sp.up + sp.taps / 2u + 1u - first_sample : 0u;
}

#endif
