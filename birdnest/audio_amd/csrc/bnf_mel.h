/*
 * bnf_mel.h -- the rule of bnflac_gather_ranges_mel: the windows of a decoded selection as mel (or
 * power) spectrogram planes [windows, planes, rows, frames], by an STFT whose analysis window,
 * twiddles and band weights the caller passes.  Everything k_gather_mel (bnflac_mel.hip) computes is
 * a function of this header, callable from host and device; bnf_gather_mel_host below walks the
 * same tiles, steps and passes with the same functions, one "lane" after the other, so
 * bnflac_gather_ranges_mel_host and the kernel are the same code, as bnf_resample.h is for the
 * resampling gather.  The header needs no HIP: a plain C++ compiler takes it too
 * (tools/gather_mel_sanitize.cpp builds it with the sanitizers).  The design of the tables
 * (bnf_mel_design_*) and the source window of a run of frames (bnf_mel_request) are host code.
 *
 * Tables.  tab (float32, 16-byte aligned on the device), with N = n_fft:
 *   tab[0 .. N)               the analysis window w
 *   tab[N .. 2N)              N / 2 twiddle pairs: tab[N + 2k] = C[k], tab[N + 2k + 1] = S[k],
 *                             k = 0 .. N/2 - 1; a design has C[k] = cos(2 pi k / N), S[k] = sin(2 pi k / N)
 *                             and the factor applied is C[k] - i S[k]
 *   tab[2N .. 2N + n_weights) the band weights
 * bands (uint32): n_mels + 1 pairs {first_bin, woff}.  Band m: nb = woff[m+1] - woff[m] bins from
 * first_bin[m], weights from woff[m].  Bad (empty, counted once per launch): woff[m+1] < woff[m],
 * woff[m+1] > n_weights, or first_bin[m] + nb > N/2 + 1.
 *
 * The rule.  Window s passes bnf_f32_window's check or is bad (nothing read, zero rows, counted).
 * n = nsamples of a good window, x[i] for 0 <= i < n the float bnflac_gather_ranges_f32 specifies
 * for sample frame i of the plane, x[i] = +0.0f elsewhere.  Frame t starts at a_t = origin + t hop
 * (signed 64-bit).  n_valid = 0 when n == 0 or c = n - N/2 - origin < 0, else c / hop + 1;
 * ncopy = min(n_valid, row_frames).  Per frame t < ncopy, every operation one float32 rounding:
 *   input      u[i] = w[i] * x[a_t + i]                                  (one product)
 *   FFT        v[brev(i)] = (u[i], +0.0f), brev the reversal of log2 N bits; then the radix-2
 *              decimation-in-time stages h = 1, 2, 4, .. N/2 in this order, no real-input packing:
 *              for every block base b (a multiple of 2h) and j < h, with k = j * (N / 2h),
 *              A = v[b + j], B = v[b + j + h]:
 *                  pr = B.im * S[k];   tr = fmaf(B.re, C[k], pr)
 *                  pi = B.re * S[k];   ti = fmaf(B.im, C[k], -pi)
 *                  v[b + j] = (A.re + tr, A.im + ti);   v[b + j + h] = (A.re - tr, A.im - ti)
 *              The twiddles come from the table only, k = 0 included.
 *   power      P[k] = fmaf(re, re, im * im) of v[k], k = 0 .. N/2
 *   rows       n_mels == 0: row k is P[k].  Else row m: acc = +0.0f; for i = 0 .. nb - 1 ascending
 *              acc = fmaf(weights[woff[m] + i], P[first_bin[m] + i], acc); a bad band's row is +0.0f.
 * No log: logf is not the same function on host and device, and the output is small enough for one
 * elementwise op downstream.
 * Every product above feeds an fmaf or a store, never a sum, and contraction is switched off in
 * every function here on top of that, so no compiler can fuse what the rule keeps apart.
 *
 * Tiles, passes, steps.  A workgroup takes one window and one tile of BNF_MEL_TF = 32 consecutive
 * frames, for all planes.  The rows go out in passes of pass_rows rows (all of them unless n_mels
 * == 0 and N/2 + 1 > 520), plane after plane; a plane's tile is worked in steps of `sf` frames whose
 * source span (sf - 1) hop + N fits the raw stage (bnf_mel_plan_of), G frames of a step at a time.
 * Per step the aligned 16-byte blocks of the span inside [0, n) are staged raw; a frame's samples
 * are fetched, converted and weighted straight out of them.  The values of a tile collect in ybuf at
 * (row - r0) * 33 + column and go out row by row: 9 pieces per row, piece j the aligned 16-byte group
 * of floats 4j - a .. 4j - a + 3 (a = the row start's float index modulo 4), as one 16-byte store
 * when all four lie in the tile, else as single floats.
 * Trip counts: tiles by row_frames, passes and planes by the spec and the layout, steps and frames
 * by ncopy (a function of the window check and n), blocks by the span, bins by a band's clamped nb.
 */
#ifndef BNF_MEL_H
#define BNF_MEL_H

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bnf_pcm_f32.h"

#if defined(__clang__)
#define BNF_MEL_STRICT _Pragma("clang fp contract(off)")
#else
#define BNF_MEL_STRICT _Pragma("STDC FP_CONTRACT OFF")
#endif

#define BNF_MEL_TF 32u            /* frames of a tile */
#define BNF_MEL_YPITCH 33u        /* floats between two rows of ybuf: 32 rows at one column take 32 banks */
#define BNF_MEL_MIN_FFT 64u
#define BNF_MEL_MAX_FFT 2048u
#define BNF_MEL_MAX_HOP 65535u
#define BNF_MEL_MAX_MELS 256u
#define BNF_MEL_MAX_WEIGHTS 8192u
#define BNF_MEL_THREADS 256u
#define BNF_MEL_RAW_BUDGET 16384u /* bytes of the raw stage unless one frame needs more */
#define BNF_MEL_PASS_ROWS 520u    /* rows of a pass at most when n_mels == 0 */
#define BNF_MEL_PIECES 9u         /* pieces of a row of a tile: 32 floats at any phase touch 9 aligned groups at most */

enum { BNF_MEL_BAD_BAND = 2u }; /* status word 0, next to BNF_F32_BAD_WINDOW */

typedef struct {
    uint32_t n_fft, hop, n_mels;
    int32_t origin;
    uint32_t n_weights;
    uint32_t reserved[3];
} bnf_mel_spec; /* bnflac_mel_spec */

BNF_F32_HD inline uint32_t bnf_mel_log2(uint32_t N) {
    uint32_t l = 0;
    while ((1u << l) < N) l++;
    return l;
}

/* Why a spec (with row_frames and frame_pitch) is refused, or a null pointer. */
BNF_F32_HD inline const char *bnf_mel_spec_refusal(const bnf_mel_spec &sp, uint32_t row_frames, uint64_t frame_pitch) {
    if (sp.n_fft < BNF_MEL_MIN_FFT || sp.n_fft > BNF_MEL_MAX_FFT || (sp.n_fft & (sp.n_fft - 1u))) return "n_fft must be a power of two in 64..2048";
    if (sp.hop < 1 || sp.hop > BNF_MEL_MAX_HOP) return "hop must be 1..65535";
    if (sp.n_mels > BNF_MEL_MAX_MELS) return "n_mels must be 0..256";
    if (sp.n_weights > BNF_MEL_MAX_WEIGHTS) return "n_weights must be 0..8192";
    if (!sp.n_mels && sp.n_weights) return "n_weights must be 0 when n_mels is 0";
    if (sp.reserved[0] | sp.reserved[1] | sp.reserved[2]) return "reserved words must be 0";
    if (row_frames >> 31) return "row_frames must be below 2^31";
    if (frame_pitch < row_frames) return "frame_pitch below row_frames";
    return nullptr;
}

/* How a call is worked: a function of the spec and the layout, not of a window.  Offsets in bytes
 * into the dynamic LDS, every part a multiple of 16. */
typedef struct {
    uint32_t N, log2n, rows, planes;
    uint32_t G, tpf;    /* frames in flight, threads per frame: G * tpf = BNF_MEL_THREADS */
    uint32_t raw_bytes; /* the raw stage */
    uint32_t sf;        /* frames of a step, 1..32 */
    uint32_t pass_rows; /* rows of a pass */
    uint32_t off_wt, off_bands, off_raw, off_work, off_ybuf, lds_bytes; /* the twiddles are at 0 */
} bnf_mel_plan;

BNF_F32_HD inline bnf_mel_plan bnf_mel_plan_of(const bnf_mel_spec &sp, uint32_t stride, uint32_t planes) {
    bnf_mel_plan p;
    p.N = sp.n_fft;
    p.log2n = bnf_mel_log2(p.N);
    p.rows = sp.n_mels ? sp.n_mels : p.N / 2u + 1u;
    p.planes = planes;
    p.G = p.N <= 512u ? 4u : p.N == 1024u ? 2u : 1u;
    p.tpf = BNF_MEL_THREADS / p.G;
    const uint32_t one = p.N * stride + 32u; /* a frame's bytes at any phase, rounded up to blocks */
    p.raw_bytes = ((one > BNF_MEL_RAW_BUDGET ? one : BNF_MEL_RAW_BUDGET) + 15u) & ~15u;
    const uint32_t span_cap = (p.raw_bytes - 32u) / stride; /* >= N */
    const uint32_t fit = (span_cap - p.N) / sp.hop + 1u;
    p.sf = fit < BNF_MEL_TF ? fit : BNF_MEL_TF;
    p.pass_rows = sp.n_mels ? sp.n_mels : p.rows < BNF_MEL_PASS_ROWS ? p.rows : BNF_MEL_PASS_ROWS;
    p.off_wt = 4u * p.N;
    p.off_bands = p.off_wt + 4u * ((sp.n_weights + 3u) & ~3u);
    p.off_raw = p.off_bands + 8u * ((sp.n_mels + 1u) & ~1u);
    p.off_work = p.off_raw + p.raw_bytes;
    p.off_ybuf = p.off_work + 8u * p.G * p.N;
    p.lds_bytes = p.off_ybuf + 4u * ((p.pass_rows * BNF_MEL_YPITCH + 3u) & ~3u);
    return p; /* at most 158,784 bytes (N 2048, stride 32, no bands: 520 rows of ybuf) of the CU's 163,840 */
}

/* One window against the PCM and the spec. */
typedef struct {
    uint64_t src0;  /* byte of the PCM at which the window's first sample frame starts (0 when n is 0) */
    uint64_t n;     /* sample frames of the window (0 when bad) */
    uint32_t ncopy; /* frames that carry values */
    uint32_t bad, cut;
} bnf_mel_row;

BNF_F32_HD inline bnf_mel_row bnf_mel_window(uint64_t pcm_first, uint64_t nsamples, uint64_t pcm_bytes, uint32_t stride,
                                             const bnf_mel_spec &sp, uint32_t row_frames) {
    const bnf_f32_row w = bnf_f32_window(pcm_first, nsamples, pcm_bytes, stride, 1u);
    bnf_mel_row r;
    r.bad = w.bad;
    r.n = w.bad ? 0u : nsamples;
    r.src0 = w.src0;
    uint64_t nv = 0;
    if (r.n) {
        /* a window of 2^48 sample frames or more has more than 2^31 hops of frames whatever the origin */
        const int64_t nn = r.n < ((uint64_t)1 << 48) ? (int64_t)r.n : (int64_t)1 << 48;
        const int64_t c = nn - (int64_t)(sp.n_fft / 2u) - (int64_t)sp.origin;
        if (c >= 0) nv = (uint64_t)c / sp.hop + 1u;
    }
    r.cut = !r.bad && nv > row_frames ? 1u : 0u;
    r.ncopy = nv < row_frames ? (uint32_t)nv : row_frames;
    return r;
}

/* The step of a row that starts at frame r1 and covers cnt frames (within one tile). */
typedef struct {
    bnf_f32_tile blk; /* blk0, nblk, phase: the aligned blocks of the sample frames [lo, hi) (nblk 0 when nin is 0) */
    uint32_t md;      /* frames of the step that carry values: the first md */
    uint32_t z;       /* positions of the span in front of sample frame lo */
    uint32_t nin;     /* sample frames of the span inside the window, from position z */
} bnf_mel_step;

BNF_F32_HD inline bnf_mel_step bnf_mel_step_of(const bnf_mel_row &row, const bnf_mel_spec &sp, uint32_t r1, uint32_t cnt,
                                               uint32_t stride) {
    bnf_mel_step st;
    st.md = row.ncopy > r1 ? (row.ncopy - r1 < cnt ? row.ncopy - r1 : cnt) : 0u;
    st.blk.blk0 = 0;
    st.blk.nblk = st.blk.phase = st.blk.ndata = st.blk.nt = 0;
    st.z = st.nin = 0;
    if (!st.md) return st;
    const int64_t a = (int64_t)sp.origin + (int64_t)r1 * sp.hop;       /* position 0 of the span */
    const int64_t end = a + (int64_t)(st.md - 1u) * sp.hop + sp.n_fft; /* below 2^48 */
    const int64_t n = row.n < ((uint64_t)1 << 62) ? (int64_t)row.n : (int64_t)1 << 62;
    const int64_t lo = a < 0 ? 0 : a, hi = end < n ? end : n;
    if (hi <= lo) return st; /* the whole span lies outside the window: every x is +0.0f */
    st.z = (uint32_t)(lo - a);
    st.nin = (uint32_t)(hi - lo);
    const uint64_t begin = row.src0 + (uint64_t)lo * stride, stop = row.src0 + (uint64_t)hi * stride;
    st.blk.blk0 = begin & ~(uint64_t)15;
    st.blk.phase = (uint32_t)begin & 15u;
    st.blk.nblk = (uint32_t)((stop - st.blk.blk0 + 15u) >> 4);
    st.blk.ndata = st.blk.nt = st.nin;
    return st;
}

/* x at position pos of a step's span, plane c (mono: the one plane), out of the raw blocks. */
BNF_F32_HD inline float bnf_mel_x(const uint32_t *raw, const bnf_mel_step &st, const bnf_f32_conv &cv, uint32_t unit,
                                  uint32_t pos, uint32_t c) {
    if (pos < st.z || pos - st.z >= st.nin) return 0.0f;
    const uint32_t at = st.blk.phase + (pos - st.z) * cv.channels * unit;
    if (!cv.mono) return bnf_f32_cvt(bnf_f32_fetch(raw, at + c * unit, unit), cv.k);
    int64_t S = 0;
    for (uint32_t ch = 0; ch < cv.channels; ch++) S += bnf_f32_fetch(raw, at + ch * unit, unit);
    return bnf_f32_cvt_mono(S, cv.kd, cv.channels);
}

/* The reversal of the low log2n bits of i. */
BNF_F32_HD inline uint32_t bnf_mel_brev(uint32_t i, uint32_t log2n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(i) >> (32u - log2n);
#else
    uint32_t r = 0;
    for (uint32_t b = 0; b < log2n; b++) r |= ((i >> b) & 1u) << (log2n - 1u - b);
    return r;
#endif
}

/* u[i] of a frame: one product. */
BNF_F32_HD inline float bnf_mel_input(float w, float x) {
    BNF_MEL_STRICT
    return w * x;
}

/* One butterfly: A, B at v + 2 ia, v + 2 ib (re, im), the twiddle pair at tw + 2 k. */
BNF_F32_HD inline void bnf_mel_bfly(float &ar, float &ai, float &br, float &bi, float c, float s) {
    BNF_MEL_STRICT
    const float pr = bi * s;
    const float tr = fmaf(br, c, pr);
    const float pi = br * s;
    const float ti = fmaf(bi, c, -pi);
    const float xr = ar, xi = ai;
    ar = xr + tr;
    ai = xi + ti;
    br = xr - tr;
    bi = xi - ti;
}

/* Butterfly q (< N/2) of the stage with half-size h = 1 << lh. */
BNF_F32_HD inline void bnf_mel_pass1(float *v, const float *tw, uint32_t log2n, uint32_t lh, uint32_t q) {
    const uint32_t h = 1u << lh, j = q & (h - 1u), i0 = ((q - j) << 1) + j, i1 = i0 + h;
    const uint32_t k = j << (log2n - lh - 1u);
    float ar = v[2u * i0], ai = v[2u * i0 + 1u], br = v[2u * i1], bi = v[2u * i1 + 1u];
    bnf_mel_bfly(ar, ai, br, bi, tw[2u * k], tw[2u * k + 1u]);
    v[2u * i0] = ar;
    v[2u * i0 + 1u] = ai;
    v[2u * i1] = br;
    v[2u * i1 + 1u] = bi;
}

/* The stages h and 2h on the four elements they couple, q < N/4: the same eight butterflies'
 * operations as two calls of the stage above per element, with one read and one write of v. */
BNF_F32_HD inline void bnf_mel_pass2(float *v, const float *tw, uint32_t log2n, uint32_t lh, uint32_t q) {
    const uint32_t h = 1u << lh, j = q & (h - 1u), i0 = ((q - j) << 2) + j;
    const uint32_t i1 = i0 + h, i2 = i1 + h, i3 = i2 + h;
    const uint32_t k1 = j << (log2n - lh - 1u), k2 = j << (log2n - lh - 2u), k3 = k2 + (1u << (log2n - 2u));
    float r0 = v[2u * i0], m0 = v[2u * i0 + 1u], r1 = v[2u * i1], m1 = v[2u * i1 + 1u];
    float r2 = v[2u * i2], m2 = v[2u * i2 + 1u], r3 = v[2u * i3], m3 = v[2u * i3 + 1u];
    const float c1 = tw[2u * k1], s1 = tw[2u * k1 + 1u];
    bnf_mel_bfly(r0, m0, r1, m1, c1, s1);
    bnf_mel_bfly(r2, m2, r3, m3, c1, s1);
    bnf_mel_bfly(r0, m0, r2, m2, tw[2u * k2], tw[2u * k2 + 1u]);
    bnf_mel_bfly(r1, m1, r3, m3, tw[2u * k3], tw[2u * k3 + 1u]);
    v[2u * i0] = r0;
    v[2u * i0 + 1u] = m0;
    v[2u * i1] = r1;
    v[2u * i1 + 1u] = m1;
    v[2u * i2] = r2;
    v[2u * i2 + 1u] = m2;
    v[2u * i3] = r3;
    v[2u * i3 + 1u] = m3;
}

/* P[k] of v[k]. */
BNF_F32_HD inline float bnf_mel_power(float re, float im) {
    BNF_MEL_STRICT
    const float q = im * im;
    return fmaf(re, re, q);
}

/* Band m of the table, checked: nb = 0 and 1 returned for a bad band. */
BNF_F32_HD inline uint32_t bnf_mel_band_of(const uint32_t *bands, uint32_t m, const bnf_mel_spec &sp, uint32_t &first,
                                           uint32_t &woff, uint32_t &nb) {
    const uint32_t f = bands[2u * m], w0 = bands[2u * m + 1u], w1 = bands[2u * m + 3u];
    first = woff = nb = 0;
    if (w1 < w0 || w1 > sp.n_weights || (uint64_t)f + (w1 - w0) > sp.n_fft / 2u + 1u) return 1u;
    first = f;
    woff = w0;
    nb = w1 - w0;
    return 0u;
}

/* A band's row value: P[k] is at p[2 k] (in the real slots of v). */
BNF_F32_HD inline float bnf_mel_band(const float *wt, const float *p, uint32_t first, uint32_t nb) {
    BNF_MEL_STRICT
    float acc = 0.0f;
    for (uint32_t i = 0; i < nb; i++) acc = fmaf(wt[i], p[2u * (first + i)], acc);
    return acc;
}

/* Piece j of a tile's row whose first float sits at index a modulo 4 of its 16-byte line: the floats
 * p0 .. p0 + 3 of the tile's cnt; whole when all four exist. */
BNF_F32_HD inline int32_t bnf_mel_piece(uint32_t a, uint32_t j) { return (int32_t)(4u * j) - (int32_t)(a & 3u); }

/* The whole call on host memory: the tiles, passes, planes, steps, frames and pieces of k_gather_mel,
 * one lane after the other.  The raw blocks, a frame's work area and ybuf are heap allocations of
 * exactly the sizes the functions above name.  -1 when out of memory, else 0. */
inline int bnf_gather_mel_host(const uint8_t *pcm, uint64_t pcm_bytes, uint32_t stride, uint32_t unit, uint32_t bps,
                               uint32_t channels, uint32_t flags, const bnf_window *windows, uint32_t nstreams,
                               const bnf_mel_spec &sp, const float *tab, const uint32_t *bands, uint32_t row_frames,
                               uint64_t frame_pitch, float *out, uint32_t status[4]) {
    status[0] = status[1] = status[2] = status[3] = 0;
    if (!nstreams) return 0;
    const bnf_f32_conv cv = bnf_f32_conv_of(channels, bps, flags);
    const uint32_t planes = cv.mono ? 1u : channels;
    const bnf_mel_plan pl = bnf_mel_plan_of(sp, stride, planes);
    const uint32_t N = pl.N;
    const float *const wnd = tab, *const tw = tab + N, *const wt = tab + 2u * (size_t)N;
    const uint64_t last_blk = bnf_f32_last_block(pcm_bytes);
    uint32_t *lb = (uint32_t *)malloc(sizeof(uint32_t) * 3u * (sp.n_mels + 1u)); /* first, woff, nb */
    if (!lb) return -1;
    for (uint32_t m = 0; m < sp.n_mels; m++)
        if (bnf_mel_band_of(bands, m, sp, lb[3u * m], lb[3u * m + 1u], lb[3u * m + 2u])) {
            status[0] |= BNF_MEL_BAD_BAND;
            status[3]++;
        }
    int rc = 0;
    for (uint32_t s = 0; s < nstreams && !rc; s++) {
        const bnf_mel_row row = bnf_mel_window(windows[s].pcm_first, windows[s].nsamples, pcm_bytes, stride, sp, row_frames);
        if (row.bad) {
            status[0] |= BNF_F32_BAD_WINDOW;
            status[1]++;
        }
        status[2] += row.cut;
        for (uint32_t t0 = 0; t0 < row_frames && !rc; t0 += BNF_MEL_TF) {
            const uint32_t cnt = row_frames - t0 < BNF_MEL_TF ? row_frames - t0 : BNF_MEL_TF;
            const uint32_t mdt = row.ncopy > t0 ? (row.ncopy - t0 < cnt ? row.ncopy - t0 : cnt) : 0u;
            for (uint32_t r0 = 0; r0 < pl.rows && !rc; r0 += pl.pass_rows) {
                const uint32_t nrow = pl.rows - r0 < pl.pass_rows ? pl.rows - r0 : pl.pass_rows;
                for (uint32_t c = 0; c < planes && !rc; c++) {
                    float *ybuf = (float *)malloc(sizeof(float) * ((size_t)(nrow - 1u) * BNF_MEL_YPITCH + BNF_MEL_TF));
                    if (!ybuf) {
                        rc = -1;
                        break;
                    }
                    for (uint32_t r1 = t0; r1 < t0 + mdt && !rc; r1 += pl.sf) {
                        const uint32_t scnt = t0 + cnt - r1 < pl.sf ? t0 + cnt - r1 : pl.sf;
                        const bnf_mel_step st = bnf_mel_step_of(row, sp, r1, scnt, stride);
                        uint32_t *raw = (uint32_t *)malloc(st.blk.nblk ? 16u * (size_t)st.blk.nblk : 1u);
                        float *v = (float *)malloc(sizeof(float) * 2u * N);
                        if (!raw || !v) {
                            free(raw);
                            free(v);
                            rc = -1;
                            break;
                        }
                        for (uint32_t j = 0; j < st.blk.nblk; j++) memcpy(raw + 4u * j, pcm + bnf_f32_block_addr(st.blk, j, last_blk), 16);
                        for (uint32_t f = 0; f < st.md; f++) {
                            for (uint32_t i = 0; i < N; i++) {
                                const uint32_t d = bnf_mel_brev(i, pl.log2n);
                                v[2u * d] = bnf_mel_input(wnd[i], bnf_mel_x(raw, st, cv, unit, f * sp.hop + i, c));
                                v[2u * d + 1u] = 0.0f;
                            }
                            uint32_t lh = 0;
                            if (pl.log2n & 1u) {
                                for (uint32_t q = 0; q < N / 2u; q++) bnf_mel_pass1(v, tw, pl.log2n, 0, q);
                                lh = 1;
                            }
                            for (; lh < pl.log2n; lh += 2u)
                                for (uint32_t q = 0; q < N / 4u; q++) bnf_mel_pass2(v, tw, pl.log2n, lh, q);
                            const uint32_t col = r1 - t0 + f;
                            if (sp.n_mels) {
                                for (uint32_t k = 0; k <= N / 2u; k++) v[2u * k] = bnf_mel_power(v[2u * k], v[2u * k + 1u]);
                                for (uint32_t m = 0; m < nrow; m++)
                                    ybuf[m * BNF_MEL_YPITCH + col] = bnf_mel_band(wt + lb[3u * m + 1u], v, lb[3u * m], lb[3u * m + 2u]);
                            } else {
                                for (uint32_t k = r0; k < r0 + nrow; k++)
                                    ybuf[(k - r0) * BNF_MEL_YPITCH + col] = bnf_mel_power(v[2u * k], v[2u * k + 1u]);
                            }
                        }
                        free(raw);
                        free(v);
                    }
                    for (uint32_t r = 0; r < nrow; r++) {
                        float *const D = out + (((uint64_t)s * planes + c) * pl.rows + r0 + r) * frame_pitch + t0;
                        const uint32_t a = (uint32_t)((uintptr_t)D >> 2) & 3u;
                        for (uint32_t j = 0; j < BNF_MEL_PIECES; j++) {
                            const int32_t p0 = bnf_mel_piece(a, j);
                            float f[4];
                            for (int e = 0; e < 4; e++) {
                                const int32_t p = p0 + e;
                                f[e] = p >= 0 && (uint32_t)p < mdt ? ybuf[r * BNF_MEL_YPITCH + (uint32_t)p] : 0.0f;
                            }
                            if (p0 >= 0 && (uint32_t)p0 + 3u < cnt)
                                memcpy(D + p0, f, sizeof f);
                            else
                                for (int e = 0; e < 4; e++)
                                    if (p0 + e >= 0 && (uint32_t)(p0 + e) < cnt) D[p0 + e] = f[e];
                        }
                    }
                    free(ybuf);
                }
            }
        }
    }
    free(lb);
    return rc;
}

/* ---------------------------------------------------------------- design and requests (host only) */

inline double bnf_mel_hz_to_mel(double f) { return 2595.0 * log10(1.0 + f / 700.0); }
inline double bnf_mel_mel_to_hz(double m) { return 700.0 * (pow(10.0, m / 2595.0) - 1.0); }

/* The three corner frequencies of triangle m of n_mels HTK triangles: points m, m + 1, m + 2 of the
 * n_mels + 2 points equally spaced in mel between f_min and f_max. */
typedef struct {
    double fl, fc, fr;
} bnf_mel_tri;

inline bnf_mel_tri bnf_mel_design_tri(uint32_t n_mels, double f_min, double f_max, uint32_t m) {
    const double m0 = bnf_mel_hz_to_mel(f_min), m1 = bnf_mel_hz_to_mel(f_max), dm = (m1 - m0) / (double)(n_mels + 1u);
    bnf_mel_tri t;
    t.fl = bnf_mel_mel_to_hz(m0 + dm * (double)m);
    t.fc = bnf_mel_mel_to_hz(m0 + dm * (double)(m + 1u));
    t.fr = bnf_mel_mel_to_hz(m0 + dm * (double)(m + 2u));
    return t;
}

/* Weight of bin k (of N/2 + 1 over [0, sample_rate / 2]) in a triangle, rounded to float32. */
inline float bnf_mel_design_weight(const bnf_mel_tri &t, uint32_t sample_rate, uint32_t N, uint32_t k) {
    const double f = (double)k * (double)sample_rate / (double)N;
    const double up = (f - t.fl) / (t.fc - t.fl), down = (t.fr - f) / (t.fr - t.fc);
    const double w = up < down ? up : down;
    return w > 0.0 ? (float)w : 0.0f;
}

/* The spec and the sizes of a design.  -> null, or why there is none (n_weights_needed is then what it takes). */
inline const char *bnf_mel_design_spec(uint32_t sample_rate, uint32_t N, uint32_t hop, uint32_t n_mels, double f_min, double f_max,
                                       bnf_mel_spec &sp, uint64_t &n_weights_needed) {
    memset(&sp, 0, sizeof sp);
    n_weights_needed = 0;
    if (!sample_rate) return "sample_rate is zero";
    if (N < BNF_MEL_MIN_FFT || N > BNF_MEL_MAX_FFT || (N & (N - 1u))) return "n_fft must be a power of two in 64..2048";
    if (hop < 1 || hop > BNF_MEL_MAX_HOP) return "hop must be 1..65535";
    if (n_mels && !(f_min >= 0.0 && f_min < f_max && f_max <= (double)sample_rate / 2.0)) return "0 <= f_min < f_max <= sample_rate / 2 must hold";
    if (n_mels <= 4096u) /* count what the design takes, also when it is over the limit, to report it */
        for (uint32_t m = 0; m < n_mels; m++) {
            const bnf_mel_tri t = bnf_mel_design_tri(n_mels, f_min, f_max, m);
            for (uint32_t k = 0; k <= N / 2u; k++)
                if (bnf_mel_design_weight(t, sample_rate, N, k) > 0.0f) n_weights_needed++;
        }
    if (n_mels > BNF_MEL_MAX_MELS || n_weights_needed > BNF_MEL_MAX_WEIGHTS) return "the design is over the limits";
    sp.n_fft = N;
    sp.hop = hop;
    sp.n_mels = n_mels;
    sp.origin = -(int32_t)(N / 2u);
    sp.n_weights = (uint32_t)n_weights_needed;
    return nullptr;
}

/* The tables of a design: tab of 2 N + n_weights floats, bands of 2 (n_mels + 1) words (not touched when n_mels is 0). */
inline void bnf_mel_design_tables(uint32_t sample_rate, const bnf_mel_spec &sp, double f_min, double f_max, float *tab,
                                  uint32_t *bands) {
    const double pi = 3.14159265358979323846;
    const uint32_t N = sp.n_fft;
    for (uint32_t i = 0; i < N; i++) tab[i] = (float)(0.5 - 0.5 * cos(2.0 * pi * (double)i / (double)N));
    for (uint32_t k = 0; k < N / 2u; k++) {
        tab[N + 2u * k] = (float)cos(2.0 * pi * (double)k / (double)N);
        tab[N + 2u * k + 1u] = (float)sin(2.0 * pi * (double)k / (double)N);
    }
    uint32_t woff = 0;
    for (uint32_t m = 0; m < sp.n_mels; m++) {
        uint32_t first = 0, nb = 0;
        const bnf_mel_tri t = bnf_mel_design_tri(sp.n_mels, f_min, f_max, m);
        for (uint32_t k = 0; k <= N / 2u; k++) {
            const float w = bnf_mel_design_weight(t, sample_rate, N, k);
            if (w > 0.0f) {
                if (!nb) first = k;
                /* a triangle's support is one run of bins */
                tab[2u * (size_t)N + woff + nb++] = w;
            }
        }
        bands[2u * m] = first;
        bands[2u * m + 1u] = woff;
        woff += nb;
    }
    if (sp.n_mels) {
        bands[2u * sp.n_mels] = 0;
        bands[2u * sp.n_mels + 1u] = woff;
    }
}

/* The source window and origin for frames [t0, t0 + n_frames) of a stream's own frame grid (frame t of
 * the stream starts at spec.origin + t hop), with the whole support of every frame:
 *   start = origin + t0 hop, first_sample = max(0, start), origin' = start - first_sample,
 *   nsamples = max(0, start + (n_frames - 1) hop + N - first_sample) (0 for n_frames = 0).
 * t0 + n_frames < 2^31. */
inline void bnf_mel_request(const bnf_mel_spec &sp, uint64_t t0, uint64_t n_frames, uint64_t &first_sample, uint64_t &nsamples,
                            int32_t &origin) {
    const int64_t start = (int64_t)sp.origin + (int64_t)t0 * sp.hop;
    const int64_t first = start < 0 ? 0 : start;
    const int64_t end = n_frames ? start + (int64_t)(n_frames - 1u) * sp.hop + sp.n_fft : first;
    first_sample = (uint64_t)first;
    origin = (int32_t)(start - first); /* start itself when negative (>= spec.origin), else 0 */
    nsamples = end > first ? (uint64_t)(end - first) : 0u;
}

#endif
