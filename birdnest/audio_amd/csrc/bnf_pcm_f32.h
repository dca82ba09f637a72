/*
 * bnf_pcm_f32.h -- the rule of bnflac_gather_ranges_f32: the windows of a decoded selection as
 * normalised float32 channel planes.  Everything k_gather_f32 (bnflac_f32.hip) computes is a
 * function of this header, callable from host and device: the window check, the tile of sample
 * frames a workgroup takes and the aligned 16-byte source blocks it loads for it, the sample
 * fetch out of the staged blocks, the plane-major staging index, the split of a plane segment
 * into aligned 4-float groups and the two conversions.  bnf_gather_f32_host below walks the same
 * tiles with the same functions, one "lane" after the other, so bnflac_gather_ranges_f32_host
 * (bnflac_runtime.cpp) and the kernel are the same code, as bnf_select.h is for the selection.
 * The header needs no HIP: a plain C++ compiler takes it too (tools/gather_f32_sanitize.cpp builds
 * it with the sanitizers).
 *
 * Layouts: those whose bytes are the samples themselves (bnflac_md5_layout != 0).  A sample frame
 * is `stride` bytes, its channel c the `unit` = stride / channels bytes at c * unit: an int32
 * (unit 4, INTERLEAVED32), an int16 (unit 2) or 3 little-endian bytes sign-extended from 24 bits
 * (unit 3).  With v the sample as int32 and k = 2^-(bps - 1):
 *   per channel   f = (float)v * k                  (int -> float rounds to nearest even; the
 *                                                    product with a power of two is exact)
 *   mono          f = (float)((double)S * k / channels), S the int64 sum of the frame's channels
 *                                                   (an exact product, one correctly rounded double
 *                                                    division, one double -> float rounding)
 * Window s (bnf_window): limit = pcm_bytes / stride; nsamples != 0 and (pcm_first > limit or
 * nsamples > limit - pcm_first) is bad: nothing of it is read, its planes are zero, it is counted.
 * ncopy = min(nsamples, row_samples).  Plane c of stream s starts at out + (s * planes + c) *
 * plane_pitch floats: ncopy values, then +0.0f up to row_samples; nothing behind that is written.
 *
 * Tiles.  A tile is bnf_f32_tile_frames(channels) sample frames of one window (at most 4,096
 * samples, at most 2,048 frames).  Its source bytes lie in the aligned 16-byte blocks
 * [blk0, blk0 + 16 nblk) that bnf_f32_tile_of names; a valid window ends at or below pcm_bytes, so
 * every block lies below round_up(pcm_bytes, 16), and bnf_f32_block_addr clamps to the buffer's
 * last block on top of that.  The blocks are staged as they are (raw), then every sample of the
 * tile is fetched from the raw bytes and staged as int32 at c * pitch + i (plane-major), then each
 * plane segment goes out as up to 3 single floats, aligned groups of 4 and up to 3 single floats.
 */
#ifndef BNF_PCM_F32_H
#define BNF_PCM_F32_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BNF_F32_HD __host__ __device__
#else
#define BNF_F32_HD
#endif

#include "bnf_select.h"

enum { BNF_F32_MONO = 1u };       /* flags */
enum { BNF_F32_BAD_WINDOW = 1u }; /* status word 0 */

#define BNF_F32_TILE_SAMPLES 4096u /* samples (frames x channels) of a tile at most */
#define BNF_F32_TILE_MAX 2048u     /* sample frames of a tile at most */
#define BNF_F32_RAW_BLOCKS 1026u   /* 16-byte blocks of a tile's source at most: 4,096 samples x 4 bytes, both ends ragged */
#define BNF_F32_STAGE_WORDS 4384u  /* int32 slots of the plane-major stage (bnf_f32_stage_words() at most) */

/* 4 stage slots, 16-byte aligned: a vector type, so that a read of it stays one 16-byte read */
typedef int32_t bnf_f32_i4 __attribute__((vector_size(16)));

/* Sample frames of one tile: a multiple of 4. */
BNF_F32_HD inline uint32_t bnf_f32_tile_frames(uint32_t channels) {
    const uint32_t f = (BNF_F32_TILE_SAMPLES / channels) & ~3u;
    return f < BNF_F32_TILE_MAX ? f : BNF_F32_TILE_MAX;
}

/* Distance in int32 slots between the stage rows of two neighbouring channels.  Modulo 32 it is
 * the value for which 32 consecutive samples e = i * channels + c (one ds_write_b32 lane group)
 * land in 32 different banks at c * pitch + i; for 6 channels no value does and this one puts at
 * most two on a bank.  tools/gather_f32_sanitize.cpp enumerates all of it. */
BNF_F32_HD inline uint32_t bnf_f32_pitch(uint32_t channels) {
    uint32_t p;
    switch (channels) {
    case 2: p = 16; break;
    case 3: p = 11; break;
    case 4: p = 8; break;
    case 5: p = 13; break;
    case 6: p = 11; break;
    case 7: p = 23; break;
    case 8: p = 4; break;
    default: p = 0; break;
    }
    return ((bnf_f32_tile_frames(channels) + 3u) | 31u) + 1u + p; /* a multiple of 32 not below frames + 4, plus p */
}

/* Slots of the stage a tile can touch: the rows, and the aligned group a read behind the last row ends in. */
BNF_F32_HD inline uint32_t bnf_f32_stage_words(uint32_t channels) {
    return (((channels - 1u) * bnf_f32_pitch(channels) + bnf_f32_tile_frames(channels) + 3u) | 3u) + 1u;
}

/* e = i * channels + c for e < 2^14 and channels 1..8, without a division per sample:
 * magic = bnf_f32_magic(channels), i = (e * magic) >> 17. */
BNF_F32_HD inline uint32_t bnf_f32_magic(uint32_t channels) { return (1u << 17) / channels + 1u; }
BNF_F32_HD inline uint32_t bnf_f32_frame_of(uint32_t e, uint32_t magic) { return (e * magic) >> 17; }

/* k = 2^-(bps - 1), bps 1..32, as float and as double (both normal numbers) */
BNF_F32_HD inline float bnf_f32_scale(uint32_t bps) {
    const uint32_t b = (127u - (bps - 1u)) << 23;
    float k;
    memcpy(&k, &b, sizeof k);
    return k;
}
BNF_F32_HD inline double bnf_f32_scale_d(uint32_t bps) {
    const uint64_t b = (uint64_t)(1023u - (bps - 1u)) << 52;
    double k;
    memcpy(&k, &b, sizeof k);
    return k;
}

/* The two conversions. */
BNF_F32_HD inline float bnf_f32_cvt(int32_t v, float k) { return (float)v * k; }
BNF_F32_HD inline float bnf_f32_cvt_mono(int64_t S, double k, uint32_t channels) {
    const double x = (double)S * k;
    /* a power of two divides exactly, and so does the product with its reciprocal: the same bits */
    if (!(channels & (channels - 1u))) return (float)(x * (1.0 / (double)channels));
    return (float)(x / (double)channels);
}

/* One window against the PCM. */
typedef struct {
    uint64_t src0;  /* byte of the PCM at which the window's first sample frame starts (0 when ncopy is 0) */
    uint64_t ncopy; /* sample frames that carry values */
    uint32_t bad, cut;
} bnf_f32_row;

BNF_F32_HD inline bnf_f32_row bnf_f32_window(uint64_t pcm_first, uint64_t nsamples, uint64_t pcm_bytes, uint32_t stride,
                                             uint32_t row_samples) {
    const uint64_t limit = pcm_bytes / stride; /* whole sample frames of the PCM */
    bnf_f32_row r;
    r.bad = nsamples != 0 && (pcm_first > limit || nsamples > limit - pcm_first) ? 1u : 0u;
    r.cut = !r.bad && nsamples > row_samples ? 1u : 0u;
    r.ncopy = r.bad ? 0u : nsamples < row_samples ? nsamples : row_samples;
    r.src0 = r.ncopy ? pcm_first * stride : 0u;
    return r;
}

/* The tile of a row that starts at sample frame t0 (a multiple of the tile's frames, below row_samples). */
typedef struct {
    uint64_t blk0;  /* byte address of the first aligned 16-byte block (ndata != 0) */
    uint32_t nblk;  /* blocks: blk0, blk0 + 16, ... */
    uint32_t phase; /* byte of block 0 at which the tile's first sample starts */
    uint32_t ndata; /* sample frames of the tile that carry values */
    uint32_t nt;    /* sample frames of the tile that are written: values, then zeros */
} bnf_f32_tile;

BNF_F32_HD inline bnf_f32_tile bnf_f32_tile_of(const bnf_f32_row &r, uint64_t t0, uint32_t frames, uint32_t stride,
                                               uint32_t row_samples) {
    bnf_f32_tile t;
    const uint64_t left = row_samples - t0, data = r.ncopy > t0 ? r.ncopy - t0 : 0u;
    t.nt = left < frames ? (uint32_t)left : frames;
    t.ndata = data < frames ? (uint32_t)data : frames;
    t.blk0 = 0;
    t.nblk = t.phase = 0;
    if (t.ndata) {
        const uint64_t begin = r.src0 + t0 * stride, end = begin + (uint64_t)t.ndata * stride;
        t.blk0 = begin & ~(uint64_t)15;
        t.phase = (uint32_t)begin & 15u;
        t.nblk = (uint32_t)((end - t.blk0 + 15u) >> 4);
    }
    return t;
}

/* Address of the buffer's last 16-byte block; the address of block j of a tile, never above it. */
BNF_F32_HD inline uint64_t bnf_f32_last_block(uint64_t pcm_bytes) {
    return pcm_bytes ? ((pcm_bytes + 15u) & ~(uint64_t)15) - 16u : 0u;
}
BNF_F32_HD inline uint64_t bnf_f32_block_addr(const bnf_f32_tile &t, uint32_t j, uint64_t last_blk) {
    const uint64_t a = t.blk0 + 16u * (uint64_t)j;
    return a < last_blk ? a : last_blk;
}

/* The sample whose first byte is byte `off` of the staged blocks (raw: their dwords, little-endian).
 * unit 2: off is even.  Reads dword off / 4, and the next one only when a 3-byte sample ends in it. */
BNF_F32_HD inline int32_t bnf_f32_fetch(const uint32_t *raw, uint32_t off, uint32_t unit) {
    const uint32_t j = off >> 2, b = off & 3u;
    const uint32_t w0 = raw[j];
    if (unit == 4u) return (int32_t)w0;
    if (unit == 2u) return (int32_t)(int16_t)(uint16_t)(w0 >> (8u * b));
    const uint32_t w1 = b > 1u ? raw[j + 1] : 0u;
    const uint32_t x = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8u * b)) & 0xffffffu;
    return (int32_t)(x ^ 0x800000u) - 0x800000;
}

/* A plane segment of nt floats whose first float sits at index a modulo 4 of its 16-byte line:
 * head single floats, ngroups aligned groups of 4, then nt - head - 4 ngroups (< 4) single floats. */
BNF_F32_HD inline void bnf_f32_split(uint32_t a, uint32_t nt, uint32_t &head, uint32_t &ngroups) {
    const uint32_t to4 = (4u - (a & 3u)) & 3u;
    head = to4 < nt ? to4 : nt;
    ngroups = (nt - head) >> 2;
}

/* Slots x .. x + 3 of the stage, as the one or two aligned groups of 4 they lie in. */
BNF_F32_HD inline void bnf_f32_read4(const bnf_f32_i4 *stage4, uint32_t x, int32_t v[4]) {
    const uint32_t sh = x & 3u;
    const bnf_f32_i4 lo = stage4[x >> 2];
    bnf_f32_i4 hi = lo;
    if (sh) hi = stage4[(x >> 2) + 1];
    v[0] = sh == 0 ? lo[0] : sh == 1 ? lo[1] : sh == 2 ? lo[2] : lo[3];
    v[1] = sh == 0 ? lo[1] : sh == 1 ? lo[2] : sh == 2 ? lo[3] : hi[0];
    v[2] = sh == 0 ? lo[2] : sh == 1 ? lo[3] : sh == 2 ? hi[0] : hi[1];
    v[3] = sh == 0 ? lo[3] : sh == 1 ? hi[0] : sh == 2 ? hi[1] : hi[2];
}

/* What the conversion of one call needs. */
typedef struct {
    uint32_t channels, pitch, mono;
    float k;
    double kd;
} bnf_f32_conv;

BNF_F32_HD inline bnf_f32_conv bnf_f32_conv_of(uint32_t channels, uint32_t bps, uint32_t flags) {
    bnf_f32_conv cv;
    cv.channels = channels;
    cv.pitch = bnf_f32_pitch(channels);
    cv.mono = flags & BNF_F32_MONO;
    cv.k = bnf_f32_scale(bps);
    cv.kd = bnf_f32_scale_d(bps);
    return cv;
}

/* Floats p .. p + 3 of plane c of a staged tile (mono: of the one plane): values below ndata, then +0. */
BNF_F32_HD inline void bnf_f32_value4(const bnf_f32_i4 *stage4, const bnf_f32_conv &cv, uint32_t c, uint32_t p,
                                      uint32_t ndata, float f[4]) {
    f[0] = f[1] = f[2] = f[3] = 0.0f;
    if (p >= ndata) return;
    int32_t v[4];
    if (!cv.mono) {
        bnf_f32_read4(stage4, c * cv.pitch + p, v);
        f[0] = bnf_f32_cvt(v[0], cv.k);
        if (p + 1u < ndata) f[1] = bnf_f32_cvt(v[1], cv.k);
        if (p + 2u < ndata) f[2] = bnf_f32_cvt(v[2], cv.k);
        if (p + 3u < ndata) f[3] = bnf_f32_cvt(v[3], cv.k);
        return;
    }
    int64_t S0 = 0, S1 = 0, S2 = 0, S3 = 0;
    for (uint32_t ch = 0; ch < cv.channels; ch++) {
        bnf_f32_read4(stage4, ch * cv.pitch + p, v);
        S0 += v[0];
        S1 += v[1];
        S2 += v[2];
        S3 += v[3];
    }
    f[0] = bnf_f32_cvt_mono(S0, cv.kd, cv.channels);
    if (p + 1u < ndata) f[1] = bnf_f32_cvt_mono(S1, cv.kd, cv.channels);
    if (p + 2u < ndata) f[2] = bnf_f32_cvt_mono(S2, cv.kd, cv.channels);
    if (p + 3u < ndata) f[3] = bnf_f32_cvt_mono(S3, cv.kd, cv.channels);
}

/* Float p alone (the singles in front of and behind the aligned groups). */
BNF_F32_HD inline float bnf_f32_value1(const bnf_f32_i4 *stage4, const bnf_f32_conv &cv, uint32_t c, uint32_t p,
                                       uint32_t ndata) {
    if (p >= ndata) return 0.0f;
    const int32_t *stage = (const int32_t *)stage4;
    if (!cv.mono) return bnf_f32_cvt(stage[c * cv.pitch + p], cv.k);
    int64_t S = 0;
    for (uint32_t ch = 0; ch < cv.channels; ch++) S += stage[ch * cv.pitch + p];
    return bnf_f32_cvt_mono(S, cv.kd, cv.channels);
}

/* The whole call on host memory: the tiles, loads, staging and stores of k_gather_f32, one lane
 * after the other.  The raw blocks and the stage of a tile are heap allocations of exactly the
 * sizes the functions above name.  -1 when out of memory, else 0. */
inline int bnf_gather_f32_host(const uint8_t *pcm, uint64_t pcm_bytes, uint32_t stride, uint32_t unit, uint32_t bps,
                               uint32_t channels, uint32_t flags, const bnf_window *windows, uint32_t nstreams,
                               uint32_t row_samples, uint64_t plane_pitch, float *out, uint32_t status[4]) {
    status[0] = status[1] = status[2] = status[3] = 0;
    const bnf_f32_conv cv = bnf_f32_conv_of(channels, bps, flags);
    const uint32_t frames = bnf_f32_tile_frames(channels), magic = bnf_f32_magic(channels);
    const uint32_t planes = cv.mono ? 1u : channels;
    const uint64_t last_blk = bnf_f32_last_block(pcm_bytes);
    for (uint32_t s = 0; s < nstreams; s++) {
        const bnf_f32_row row = bnf_f32_window(windows[s].pcm_first, windows[s].nsamples, pcm_bytes, stride, row_samples);
        if (row.bad) {
            status[0] |= BNF_F32_BAD_WINDOW;
            status[1]++;
        }
        status[2] += row.cut;
        for (uint64_t t0 = 0; t0 < row_samples; t0 += frames) {
            const bnf_f32_tile t = bnf_f32_tile_of(row, t0, frames, stride, row_samples);
            uint32_t *raw = nullptr;
            bnf_f32_i4 *stage4 = nullptr;
            if (t.ndata) {
                raw = (uint32_t *)malloc(16u * (size_t)t.nblk);
                stage4 = (bnf_f32_i4 *)calloc(bnf_f32_stage_words(channels) / 4u, sizeof(bnf_f32_i4));
                if (!raw || !stage4) {
                    free(raw);
                    free(stage4);
                    return -1;
                }
                for (uint32_t j = 0; j < t.nblk; j++) memcpy(raw + 4u * j, pcm + bnf_f32_block_addr(t, j, last_blk), 16);
                int32_t *stage = (int32_t *)stage4;
                for (uint32_t e = 0; e < t.ndata * channels; e++) {
                    const uint32_t i = bnf_f32_frame_of(e, magic), c = e - i * channels;
                    stage[c * cv.pitch + i] = bnf_f32_fetch(raw, t.phase + e * unit, unit);
                }
            }
            for (uint32_t c = 0; c < planes; c++) {
                float *const D = out + ((uint64_t)s * planes + c) * plane_pitch + t0;
                uint32_t head, ngroups;
                bnf_f32_split((uint32_t)((uintptr_t)D >> 2), t.nt, head, ngroups);
                for (uint32_t p = 0; p < head; p++) D[p] = bnf_f32_value1(stage4, cv, c, p, t.ndata);
                for (uint32_t q = 0; q < ngroups; q++) {
                    float f[4];
                    bnf_f32_value4(stage4, cv, c, head + 4u * q, t.ndata, f);
                    memcpy(D + head + 4u * q, f, sizeof f);
                }
                for (uint32_t p = head + 4u * ngroups; p < t.nt; p++) D[p] = bnf_f32_value1(stage4, cv, c, p, t.ndata);
            }
            free(raw);
            free(stage4);
        }
    }
    return 0;
}

#endif
