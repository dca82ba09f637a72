/*
 * bnflac_runtime.cpp -- host side of libbnflac.so.
 *
 *  - bnflac_* batched API: thin, asynchronous launchers over the HIP kernels.
 *  - FLAC__stream_decoder_*: libFLAC 1.2.1-compatible stream decoder.  Metadata and
 *    the libFLAC state machine (find_metadata_, frame_sync_, the per-frame error and
 *    write sequence of read_frame_, LibFlac.dll@0x10010130/0x10011760/0x100118c0) are
 *    replayed on the host from per-frame records; every frame body is decoded on the
 *    GPU in windows of many frames at once.  Read-ahead changes when the client's read
 *    callback is called, never what the write/error callbacks receive.
 *
 * The product path has no CPU decode: if no GPU is usable the decoder fails loudly
 * (init returns MEMORY_ALLOCATION_ERROR and bnflac_last_error() says why).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "../../../include/bnflac.h"
#include "bnf_metadata.h"
#include "bnf_pcm_f32.h"
#include "bnflac_device.h"
#include "bnflac_launch.h"
#include "bnflac_md5.h"

static_assert(sizeof(bnflac_frame_info) == sizeof(bnf_frame_info), "frame info layout");
static_assert(sizeof(bnf_frame_info) == 128, "frame info is 128 bytes");
static_assert(offsetof(FLAC__FrameHeader, number) == 24, "FrameHeader.FrameOrSampleNumber @24 (LibFLACSharp.cs:232)");
static_assert(offsetof(FLAC__FrameHeader, crc) == 32, "FrameHeader.Crc @32 (LibFLACSharp.cs:233)");
static_assert(offsetof(FLAC__StreamMetadata, data) == 16, "StreamMetadata.data @16 (LibFLACSharp.cs:299)");
static_assert(offsetof(FLAC__StreamMetadata, data.stream_info.sample_rate) == 32, "sample_rate @32");
static_assert(offsetof(FLAC__StreamMetadata, data.stream_info.total_samples) == 48, "total_samples @48");

/* ------------------------------------------------------------------ errors */
static thread_local std::string g_err;
static int fail(const std::string &m, int code = -1) {
    g_err = m;
    return code;
}
extern "C" BNFLAC_API const char *bnflac_last_error(void) { return g_err.c_str(); }

/* ------------------------------------------------------------ CRC tables */
static void build_tables(uint8_t *c8, uint16_t *c16, uint16_t *xp) {
    for (int i = 0; i < 256; i++) {
        uint8_t c = (uint8_t)i;
        for (int b = 0; b < 8; b++) c = (uint8_t)((c & 0x80) ? (c << 1) ^ 0x07 : (c << 1));
        c8[i] = c;
        uint16_t w = (uint16_t)(i << 8);
        for (int b = 0; b < 8; b++) w = (uint16_t)((w & 0x8000) ? (w << 1) ^ 0x8005 : (w << 1));
        c16[i] = w;
    }
    for (int k = 1; k < 8; k++)
        for (int i = 0; i < 256; i++) {
            uint16_t p = c16[(k - 1) * 256 + i];
            c16[k * 256 + i] = (uint16_t)((p << 8) ^ c16[p >> 8]);
        }
    /* x^(8*2^j) mod P */
    auto mulmod = [](uint32_t a, uint32_t b) {
        uint32_t r = 0;
        for (int i = 15; i >= 0; i--) {
            r = (r & 0x8000u) ? ((r << 1) ^ 0x8005u) & 0xffffu : (r << 1);
            if ((b >> i) & 1u) r ^= a;
        }
        return r;
    };
    uint32_t v = 0x0100; /* x^8 */
    for (int j = 0; j < 40; j++) {
        xp[j] = (uint16_t)v;
        v = mulmod(v, v);
    }
}

/* The caller's current HIP device is restored on scope exit (the library never leaves the
 * thread on another device). */
struct DevGuard {
    int prev = -1;
    explicit DevGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DevGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

static std::mutex g_dev_mu;
static bool g_tables_ready[64];

static int ensure_device(int dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail("bnflac: no HIP device available (the decode path is GPU-only)");
    if (dev < 0 || dev >= n || dev >= 64) return fail("bnflac: bad device index");
    std::lock_guard<std::mutex> lk(g_dev_mu);
    DevGuard g(dev);
    if (!g_tables_ready[dev]) {
        uint8_t c8[256];
        uint16_t c16[8 * 256], xp[40];
        build_tables(c8, c16, xp);
        if (bnf_upload_tables(c8, c16, xp) != hipSuccess) return fail("bnflac: table upload failed");
        g_tables_ready[dev] = true;
    }
    return 0;
}

/* Timing experiments and exact A/B switches (bench.py --ablate); the bits are listed in
 * bnflac_launch.h (BNF_ABLATE_*).  Results are wrong while a timing bit is set. */
extern "C" BNFLAC_API void bnflac_debug_set_ablate(uint32_t flags) { bnf_set_ablate(flags); }
/* 1 in a -DBNFLAC_CRC_FOLD_CHECK build (k_decode_st's tail computes the CRC-16 both ways and
 * counts the lanes that disagree, bnflac_debug_stats slot 7); 0 in the shipped library */
extern "C" BNFLAC_API int bnflac_debug_crc_fold_check(void) {
#ifdef BNFLAC_CRC_FOLD_CHECK
    return 1;
#else
    return 0;
#endif
}
/* parse kernel: -1 auto (k_parse_wave for small launches), 0 k_parse, 1 k_parse_wave (tests, A/B) */
extern "C" BNFLAC_API void bnflac_debug_set_parse_wave(int mode) { bnf_set_parse_wave(mode); }
/* k_decode_sys (systolic restore, every frame class): -1 auto (BNFLAC_DECODE_SYS), 0 the lane
 * kernels by class, 1 always (tests, A/B) */
extern "C" BNFLAC_API void bnflac_debug_set_decode_sys(int mode) { bnf_set_decode_sys(mode); }
/* the CRC-16 hand-off: -1 env BNFLAC_CRC_MODE (default 3), 0 none, 1 k_parse's prefix, 2 + its verdict,
 * 3 the prefix where it pays (bnf_launch_parse) */
extern "C" BNFLAC_API void bnflac_debug_set_crc_mode(int mode) { bnf_set_crc_mode(mode); }
extern "C" BNFLAC_API uint64_t bnflac_debug_decode_seg_launches(void) { return bnf_decode_seg_launches(); }
/* which kernels and streams the process's last decode and parse launches chose, and the history
 * words they read (include/bnflac.h; 12 words) */
extern "C" BNFLAC_API void bnflac_debug_last_route(uint32_t *out12) {
    if (out12) bnf_last_route(out12);
}
/* k_parse_wave's debug counters (collected when BNFLAC_PW_STATS is set): passes, splice rounds,
 * serial fallbacks, partitions, frames, wave-cycles in scans.  out8: 8 values. */
extern "C" BNFLAC_API int bnflac_debug_parse_wave_stats(uint64_t *out8, int reset) {
    return bnf_parse_wave_stats(out8, reset) == hipSuccess ? 0 : -1;
}
extern "C" BNFLAC_API int bnflac_debug_stats(uint64_t *out16, int reset) {
    return bnf_stats(out16, reset) == hipSuccess ? 0 : fail("bnflac_debug_stats failed");
}

extern "C" BNFLAC_API int bnflac_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

/* ----------------------------------------------------------------- context */
struct CtxBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool grow(size_t n) {
        if (n <= cap) return true;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        if (hipMalloc(&p, n) != hipSuccess) return false;
        cap = n;
        return true;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct bnflac_ctx {
    int device;
    uint32_t *d_block_counts = nullptr;
    uint32_t block_cap = 0;
    /* bnflac_index_stream scratch */
    CtxBuf cand, info, gap, jump, mark, pos, bs, small;
    CtxBuf ms; /* bnflac_index_streams scratch (bnf_ms_scratch, one allocation) */
    /* the candidate table the last bnflac_index_streams_resync left in ms, and the control words
     * that hold its length (nullptr: none) */
    const bnf_index_cand *rs_ct = nullptr;
    const uint32_t *rs_ctl = nullptr;
    CtxBuf sel; /* bnflac_select_ranges scratch (flags and workgroup sums) */
    CtxBuf order, porder; /* decode / parse order: histogram + permutation (k_order_*) */
    /* k_parse's CRC-16 hand-off of the last bnflac_parse_frames batch (8 words per frame), and
     * the batch they belong to: bnflac_decode_parsed uses them only for that same batch */
    CtxBuf crcp;
    const void *crcp_bytes = nullptr, *crcp_info = nullptr;
    uint64_t crcp_nbytes = 0;
    uint32_t crcp_n = 0;
};

/* crc mode 0: no CRC-16 hand-off, the decode tails check the whole frame (1 / 2 choose who
 * computes it: bnf_launch_parse) */
static bool crc_prefix_on() { return bnf_crc_mode() != 0; }

extern "C" BNFLAC_API int bnflac_ctx_create(int device, bnflac_ctx **out) {
    *out = nullptr;
    if (ensure_device(device)) return -1;
    bnflac_ctx *c = new bnflac_ctx();
    c->device = device;
    *out = c;
    return 0;
}

/* Debug: the CRC-16 hand-off of the ctx's last bnflac_parse_frames (8 words per frame, see
 * CRCP_WORDS in bnf_crc16.h), synchronously; -1 when there is none for nframes frames */
extern "C" BNFLAC_API int bnflac_debug_crc_handoff(bnflac_ctx *ctx, uint32_t *out, uint32_t nframes) {
    if (!ctx || !out) return fail("bnflac_debug_crc_handoff: null argument");
    if (!ctx->crcp_bytes || ctx->crcp_n != nframes) return fail("bnflac_debug_crc_handoff: no hand-off for this batch");
    DevGuard dg(ctx->device);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, ctx->crcp.p, 32ull * nframes, hipMemcpyDeviceToHost) != hipSuccess)
        return fail("bnflac_debug_crc_handoff: HIP error");
    return 0;
}

extern "C" BNFLAC_API void bnflac_ctx_destroy(bnflac_ctx *ctx) {
    if (!ctx) return;
    if (ctx->d_block_counts) (void)hipFree(ctx->d_block_counts);
    for (CtxBuf *b : {&ctx->cand, &ctx->info, &ctx->gap, &ctx->jump, &ctx->mark, &ctx->pos, &ctx->bs, &ctx->small,
                      &ctx->ms, &ctx->sel, &ctx->order, &ctx->porder, &ctx->crcp})
        b->release();
    delete ctx;
}

static uint32_t lanes_for(uint32_t channels) {
    uint32_t l = 1;
    while (l < channels) l <<= 1;
    return l > 8 ? 8 : l;
}

extern "C" BNFLAC_API uint32_t bnflac_out_stride(int fmt, const bnflac_stream_params *sp) {
    switch (fmt) {
    case BNFLAC_OUT_PLANAR32:
    case BNFLAC_OUT_INTERLEAVED32: return 4u * sp->channels;
    case BNFLAC_OUT_FLACDECODER: return sp->channels == 2 ? 4u : 2u;
    default: return sp->channels * (sp->bps == 24 ? 3u : 2u);
    }
}

extern "C" BNFLAC_API int bnflac_md5_interleaved32(const int32_t *pcm, uint64_t nsamples, uint32_t channels,
                                                   uint32_t bps, uint8_t out_md5[16]) {
    if ((!pcm && nsamples) || !out_md5) return fail("bnflac_md5_interleaved32: null pointer");
    if (channels < 1 || channels > FLAC__MAX_CHANNELS || bps < 4 || bps > 32)
        return fail("bnflac_md5_interleaved32: bad channels/bps");
    Md5 m;
    md5_init(m);
    const int32_t *chan[FLAC__MAX_CHANNELS];
    for (uint32_t c = 0; c < channels; c++) chan[c] = pcm + c;
    md5_accumulate(m, chan, channels, nsamples, channels, (bps + 7) / 8);
    md5_final(m, out_md5);
    return 0;
}

extern "C" BNFLAC_API uint32_t bnflac_md5_layout(int fmt, const bnflac_stream_params *sp) {
    if (!sp || sp->channels < 1 || sp->channels > FLAC__MAX_CHANNELS || sp->bps < 4 || sp->bps > 32) return 0;
    const uint32_t B = (sp->bps + 7) / 8;
    switch (fmt) {
    case BNFLAC_OUT_INTERLEAVED32: return B;
    case BNFLAC_OUT_FLACDECODER: return sp->bps == 16 && sp->channels <= 2 ? B : 0; /* 16-bit samples, 1-2 channels */
    case BNFLAC_OUT_FILEREADER: return sp->bps == 16 || sp->bps == 24 ? B : 0;      /* bps / 8 bytes, every channel */
    default: return 0; /* PLANAR32 is channel-major per frame: it needs the frame table */
    }
}

extern "C" BNFLAC_API int bnflac_md5_streams(bnflac_ctx *ctx, const uint8_t *d_pcm, uint64_t pcm_bytes, int fmt,
                                             const bnflac_stream_params *sp, const uint64_t *d_stream_samples,
                                             uint32_t nstreams, const uint8_t *d_expected, uint8_t *d_md5,
                                             uint32_t *d_verdict, uint32_t *d_status, void *hs) {
    if (!ctx || !sp) return fail("bnflac_md5_streams: null argument");
    DevGuard dg(ctx->device); /* the launch on the context's device */
    if (!d_status || (nstreams && (!d_stream_samples || !d_md5))) return fail("bnflac_md5_streams: null output");
    if (pcm_bytes && !d_pcm) return fail("bnflac_md5_streams: null d_pcm");
    if (((uintptr_t)d_pcm) & 15u) return fail("bnflac_md5_streams: d_pcm must be 16-byte aligned");
    if (nstreams >= (1u << 30)) return fail("bnflac_md5_streams: too many streams");
    const uint32_t B = bnflac_md5_layout(fmt, sp);
    if (!B) return fail("bnflac_md5_streams: layout does not carry the MD5 bytes");
    const bool int32_src = fmt == BNFLAC_OUT_INTERLEAVED32;
    hipError_t e = bnf_launch_md5_streams(d_pcm, pcm_bytes, bnflac_out_stride(fmt, sp), int32_src ? B : 0, d_stream_samples,
                                          nstreams, d_expected, d_md5, d_verdict, d_status, (hipStream_t)hs);
    return e == hipSuccess ? 0 : fail(std::string("bnflac_md5_streams: ") + hipGetErrorString(e));
}

extern "C" BNFLAC_API int bnflac_index_frames(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes,
                                              uint64_t *d_offsets, uint32_t cap, uint32_t *d_count, void *hs) {
    if (!ctx) return fail("bnflac_index_frames: null ctx");
    DevGuard dg(ctx->device); /* launches and scratch on the context's device */
    if (((uintptr_t)d_bytes) & 3u) return fail("bnflac_index_frames: d_bytes must be 4-byte aligned");
    const uint32_t nb = bnf_scan_blocks(nbytes);
    if (nb > ctx->block_cap) {
        if (ctx->d_block_counts) (void)hipFree(ctx->d_block_counts);
        ctx->d_block_counts = nullptr;
        if (hipMalloc(&ctx->d_block_counts, sizeof(uint32_t) * (size_t)std::max(nb, 1u)) != hipSuccess)
            return fail("bnflac_index_frames: out of device memory");
        ctx->block_cap = nb;
    }
    hipError_t e = bnf_launch_sync_scan(d_bytes, nbytes, ctx->d_block_counts, d_count, d_offsets, cap, (hipStream_t)hs);
    return e == hipSuccess ? 0 : fail(std::string("bnflac_index_frames: ") + hipGetErrorString(e));
}

static int check_args(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes, const bnflac_stream_params *sp,
                      const char *who) {
    if (!ctx || !sp) return fail(std::string(who) + ": null argument");
    if (((uintptr_t)d_bytes) & 15u) return fail(std::string(who) + ": d_bytes must be 16-byte aligned");
    if (sp->channels < 1 || sp->channels > 8) return fail(std::string(who) + ": channels must be 1..8");
    if (nbytes >= (1ull << 34)) return fail(std::string(who) + ": buffer larger than 16 GiB");
    return 0;
}

extern "C" BNFLAC_API int bnflac_parse_frames(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes,
                                              const uint64_t *d_frame_offsets, uint32_t nframes,
                                              const bnflac_stream_params *sp, const uint64_t *d_out_sample,
                                              uint64_t base_sample, bnflac_frame_info *d_info, void *hs) {
    if (check_args(ctx, d_bytes, nbytes, sp, "bnflac_parse_frames")) return -1;
    DevGuard dg(ctx->device); /* launches and scratch on the context's device */
    bnf_stream_params p;
    memcpy(&p, sp, sizeof p);
    if (!ctx->porder.grow(sizeof(uint32_t) * (256u + (size_t)nframes)))
        return fail("bnflac_parse_frames: out of device memory (parse-order scratch)");
    ctx->crcp_bytes = ctx->crcp_info = nullptr; /* no prefixes until this launch is enqueued */
    const bool pre = crc_prefix_on() && ctx->crcp.grow(32u * std::max<size_t>(nframes, 1u));
    bool handed = false;
    hipError_t e = bnf_launch_parse((const uint32_t *)d_bytes, nbytes, d_frame_offsets,
                                    nframes, p, d_out_sample, base_sample, (bnf_frame_info *)d_info,
                                    (uint32_t *)ctx->porder.p, pre ? (uint32_t *)ctx->crcp.p : nullptr, &handed,
                                    (hipStream_t)hs);
    if (e == hipSuccess && pre && handed) {
        ctx->crcp_bytes = d_bytes;
        ctx->crcp_info = d_info;
        ctx->crcp_nbytes = nbytes;
        ctx->crcp_n = nframes;
    }
    return e == hipSuccess ? 0 : fail(std::string("k_parse: ") + hipGetErrorString(e));
}

extern "C" BNFLAC_API int bnflac_decode_parsed(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes, uint32_t nframes,
                                               const bnflac_stream_params *sp, int out_format, uint8_t *d_out,
                                               uint64_t out_bytes, bnflac_frame_info *d_info, void *hs) {
    if (check_args(ctx, d_bytes, nbytes, sp, "bnflac_decode_parsed")) return -1;
    DevGuard dg(ctx->device); /* launches and scratch on the context's device */
    if (out_format < 0 || out_format > 3) return fail("bnflac_decode_parsed: bad out_format");
    bnf_stream_params p;
    memcpy(&p, sp, sizeof p);
    /* decode order (256 + nframes) + k_decode_sys's hand-back list (4 + nframes) */
    if (!ctx->order.grow(sizeof(uint32_t) * (260u + 2u * (size_t)nframes)))
        return fail("bnflac_decode_parsed: out of device memory (decode-order scratch)");
    /* the parse of this same batch on this context handed over its CRC-16 work (used once) */
    const bool pre = ctx->crcp_bytes == d_bytes && ctx->crcp_info == d_info && ctx->crcp_nbytes == nbytes &&
                     ctx->crcp_n == nframes;
    ctx->crcp_bytes = ctx->crcp_info = nullptr;
    hipError_t e = bnf_launch_decode((const uint32_t *)d_bytes, nbytes, nframes, p,
                                     lanes_for(sp->channels), out_format, d_out, out_bytes, (bnf_frame_info *)d_info,
                                     (uint32_t *)ctx->order.p, pre ? (const uint32_t *)ctx->crcp.p : nullptr,
                                     (hipStream_t)hs);
    if (e == hipSuccess) /* a non-OK frame's range: zeros (include/bnflac.h) */
        e = bnf_launch_fill_bad((const bnf_frame_info *)d_info, nframes, p, out_format, d_out, out_bytes, (hipStream_t)hs);
    return e == hipSuccess ? 0 : fail(std::string("k_decode: ") + hipGetErrorString(e));
}

extern "C" BNFLAC_API int bnflac_decode_frames(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes,
                                               const uint64_t *d_frame_offsets, uint32_t nframes,
                                               const bnflac_stream_params *sp, const uint64_t *d_out_sample,
                                               uint64_t base_sample, int out_format, uint8_t *d_out, uint64_t out_bytes,
                                               bnflac_frame_info *d_info, void *hs) {
    if (out_format < 0 || out_format > 3) return fail("bnflac_decode_frames: bad out_format");
    int rc = bnflac_parse_frames(ctx, d_bytes, nbytes, d_frame_offsets, nframes, sp, d_out_sample, base_sample, d_info, hs);
    if (rc) return rc;
    return bnflac_decode_parsed(ctx, d_bytes, nbytes, nframes, sp, out_format, d_out, out_bytes, d_info, hs);
}

extern "C" BNFLAC_API int bnflac_index_stream(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes,
                                              uint64_t first_offset, const bnflac_stream_params *sp,
                                              uint64_t *d_frame_offsets, uint64_t *d_out_sample,
                                              bnflac_frame_info *d_info, uint32_t cap, uint32_t *d_nframes, void *hs) {
    if (check_args(ctx, d_bytes, nbytes, sp, "bnflac_index_stream")) return -1;
    DevGuard dg(ctx->device); /* launches and scratch on the context's device */
    if (!d_frame_offsets || !d_nframes) return fail("bnflac_index_stream: null output");
    hipStream_t s = (hipStream_t)hs;
    /* 1. sync candidates (one host sync for their count) */
    uint32_t ccap = (uint32_t)std::min<uint64_t>(nbytes / 1024 + 4096, 1u << 30), ncand = 0;
    for (int attempt = 0;; attempt++) {
        if (!ctx->cand.grow(sizeof(uint64_t) * ccap) || !ctx->small.grow(64))
            return fail("bnflac_index_stream: out of device memory");
        if (bnflac_index_frames(ctx, d_bytes, nbytes, (uint64_t *)ctx->cand.p, ccap, (uint32_t *)ctx->small.p, hs))
            return -1;
        if (hipMemcpyAsync(&ncand, ctx->small.p, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return fail("bnflac_index_stream: HIP error reading the candidate count");
        if (ncand <= ccap) break;
        if (attempt) return fail("bnflac_index_stream: candidate count changed");
        ccap = ncand;
    }
    if (ncand >= (1u << 30)) return fail("bnflac_index_stream: too many sync candidates");
    uint32_t levels = 1;
    while ((1ull << levels) <= ncand) levels++;
    const size_t n = std::max<uint32_t>(ncand, 1u);
    if (!ctx->info.grow(sizeof(bnf_frame_info) * n) || !ctx->gap.grow(4 * n) || !ctx->jump.grow(4 * n * levels) ||
        !ctx->mark.grow(4 * n) || !ctx->pos.grow(4 * n) || !ctx->bs.grow(8 * n))
        return fail("bnflac_index_stream: out of device memory");
    bnf_stream_params p;
    memcpy(&p, sp, sizeof p);
    ctx->crcp_bytes = ctx->crcp_info = nullptr; /* the records this writes carry no CRC-16 hand-off */
    /* 2. header, CRC-8 and subframe walk of every candidate */
    hipError_t e = bnf_launch_parse((const uint32_t *)d_bytes, nbytes, (const uint64_t *)ctx->cand.p, ncand, p, nullptr,
                                    0, (bnf_frame_info *)ctx->info.p, nullptr, nullptr, nullptr, s);
    /* 3. successor chain, EOS rule, compaction */
    if (e == hipSuccess)
        e = bnf_launch_chain(d_bytes, nbytes, (const uint64_t *)ctx->cand.p, ncand, (const bnf_frame_info *)ctx->info.p,
                             first_offset, p, (uint32_t *)ctx->gap.p, (int32_t *)ctx->jump.p, levels,
                             (uint32_t *)ctx->mark.p, (uint32_t *)ctx->pos.p, (uint64_t *)ctx->bs.p,
                             (uint8_t *)ctx->small.p + 16, d_frame_offsets, d_out_sample, (bnf_frame_info *)d_info, cap,
                             d_nframes, s);
    return e == hipSuccess ? 0 : fail(std::string("bnflac_index_stream: ") + hipGetErrorString(e));
}

static_assert(sizeof(bnflac_stream_desc) == sizeof(bnf_stream_desc), "stream descriptor layout");

/* The scratch of the batched chain, sized on the host from cand_cap, nstreams and nbytes: every
 * array starts on a 16-byte boundary of one allocation (ctx->ms); `extra` more bytes behind them
 * at *extra_p.  false: out of device memory. */
static bool ms_scratch(bnflac_ctx *ctx, size_t C, size_t S, uint64_t nbytes, size_t extra, bnf_ms_scratch &w,
                       uint8_t **extra_p) {
    const size_t B = bnf_scan_blocks(nbytes);
    const size_t nsum = std::max(B, std::max(C, S)) / 1024 + 2;
    size_t off = 0;
    auto take = [&off](size_t bytes) {
        const size_t at = off;
        off += (bytes + 15) & ~(size_t)15;
        return at;
    };
    const size_t o_ctl = take(16), o_blk = take(4 * (B + 1)), o_csum = take(4 * nsum), o_asum = take(8 * nsum),
                 o_cand = take(8 * C), o_info = take(sizeof(bnf_frame_info) * C), o_seg = take(4 * C), o_key = take(4 * C),
                 o_mark = take(4 * C), o_pos = take(4 * (C + 1)), o_bs = take(8 * C), o_smp = take(8 * (C + 1)),
                 o_jump = take(8 * C), o_clo = take(4 * S), o_chi = take(4 * S), o_kept = take(4 * S), o_head = take(4 * S),
                 o_ssum = take(8 * S), o_ss = take(8 * (S + 1)), o_extra = take(extra);
    if (!ctx->ms.grow(off)) return false;
    uint8_t *m = (uint8_t *)ctx->ms.p;
    w.ctl = (uint32_t *)(m + o_ctl);
    w.blk = (uint32_t *)(m + o_blk);
    w.csum = (uint32_t *)(m + o_csum);
    w.asum = (uint64_t *)(m + o_asum);
    w.cand = (uint64_t *)(m + o_cand);
    w.info = (bnf_frame_info *)(m + o_info);
    w.seg = (int32_t *)(m + o_seg);
    w.key = (uint32_t *)(m + o_key);
    w.mark = (uint32_t *)(m + o_mark);
    w.pos = (uint32_t *)(m + o_pos);
    w.bs = (uint64_t *)(m + o_bs);
    w.smp = (uint64_t *)(m + o_smp);
    w.jump = (int32_t *)(m + o_jump);
    w.clo = (uint32_t *)(m + o_clo);
    w.chi = (uint32_t *)(m + o_chi);
    w.kept = (uint32_t *)(m + o_kept);
    w.head = (int32_t *)(m + o_head);
    w.ssum = (uint64_t *)(m + o_ssum);
    w.ss = (uint64_t *)(m + o_ss);
    if (extra_p) *extra_p = m + o_extra;
    return true;
}

extern "C" BNFLAC_API int bnflac_index_streams(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes,
                                               const bnflac_stream_desc *d_streams, uint32_t nstreams,
                                               const bnflac_stream_params *sp, uint32_t cand_cap,
                                               uint64_t *d_frame_offsets, uint64_t *d_out_sample,
                                               bnflac_frame_info *d_info, uint32_t cap, uint32_t *d_stream_frames,
                                               uint64_t *d_stream_samples, uint32_t *d_status, void *hs) {
    if (check_args(ctx, d_bytes, nbytes, sp, "bnflac_index_streams")) return -1;
    DevGuard dg(ctx->device); /* launches and scratch on the context's device */
    if (!d_stream_frames || !d_status || (cap && !d_frame_offsets)) return fail("bnflac_index_streams: null output");
    if (nstreams && !d_streams) return fail("bnflac_index_streams: null descriptor table");
    if (nstreams >= (1u << 30)) return fail("bnflac_index_streams: too many streams");
    hipStream_t s = (hipStream_t)hs;
    ctx->crcp_bytes = ctx->crcp_info = nullptr; /* the records this writes carry no CRC-16 hand-off */
    if (!nstreams || !nbytes) { /* nothing to index: zeros */
        hipError_t e = hipMemsetAsync(d_status, 0, 4 * sizeof(uint32_t), s);
        if (e == hipSuccess) e = hipMemsetAsync(d_stream_frames, 0, sizeof(uint32_t) * ((size_t)nstreams + 1), s);
        if (e == hipSuccess && d_stream_samples)
            e = hipMemsetAsync(d_stream_samples, 0, sizeof(uint64_t) * ((size_t)nstreams + 1), s);
        return e == hipSuccess ? 0 : fail(std::string("bnflac_index_streams: ") + hipGetErrorString(e));
    }
    const uint64_t C64 = cand_cap ? cand_cap : nbytes / 1024 + 4096;
    if (C64 >= (1u << 30)) return fail("bnflac_index_streams: cand_cap too large");
    const size_t C = (size_t)C64;
    bnf_ms_scratch w;
    ctx->rs_ct = nullptr; /* the scratch is reused: no candidate table of a resync call any more */
    if (!ms_scratch(ctx, C, nstreams, nbytes, 0, w, nullptr)) return fail("bnflac_index_streams: out of device memory");
    bnf_stream_params p;
    memcpy(&p, sp, sizeof p);
    hipError_t e = bnf_launch_chain_streams(d_bytes, nbytes, (const bnf_stream_desc *)d_streams, nstreams, p, (uint32_t)C, w,
                                            d_frame_offsets, d_out_sample, (bnf_frame_info *)d_info, cap, d_stream_frames,
                                            d_stream_samples, d_status, s);
    return e == hipSuccess ? 0 : fail(std::string("bnflac_index_streams: ") + hipGetErrorString(e));
}

static_assert(sizeof(bnflac_index_cand) == sizeof(bnf_index_cand) && sizeof(bnf_index_cand) == 32, "index candidate layout");
static_assert(sizeof(bnflac_resync_slot) == sizeof(bnf_resync_slot) && sizeof(bnf_resync_slot) == 16, "resync slot layout");
static_assert(sizeof(bnflac_resync_rec) == sizeof(bnf_resync_rec) && sizeof(bnf_resync_rec) == 32, "resync record layout");
static_assert(offsetof(bnflac_index_cand, succ) == 16 && offsetof(bnf_index_cand, succ) == 16 &&
                  offsetof(bnflac_index_cand, flags) == 28 && offsetof(bnf_index_cand, flags) == 28,
              "index candidate fields");
static_assert(offsetof(bnflac_resync_rec, gap_samples) == 16 && offsetof(bnf_resync_rec, gap_samples) == 16,
              "resync record: gap_samples @16");
static_assert((uint32_t)BNFLAC_FRAME_GAP == (uint32_t)BNF_FL_GAP && (int)BNFLAC_RESYNC_LEADING == (int)BNF_RESYNC_LEADING &&
                  (int)BNFLAC_RESYNC_RESYNCED == (int)BNF_RESYNC_RESYNCED,
              "resync flag values");

/* what both resync calls refuse about the blocksize */
static const char *resync_refusal(const bnflac_stream_params *sp) {
    if (!sp->has_stream_info) return "needs STREAMINFO (has_stream_info)";
    if (sp->min_blocksize != sp->max_blocksize || sp->min_blocksize < 1) return "a fixed-blocksize stream only (min == max >= 1)";
    return nullptr;
}

extern "C" BNFLAC_API int bnflac_index_streams_resync(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes,
                                                      const bnflac_stream_desc *d_streams, uint32_t nstreams,
                                                      const bnflac_stream_params *sp, uint32_t cand_cap,
                                                      uint64_t *d_frame_offsets, uint64_t *d_out_sample,
                                                      bnflac_frame_info *d_info, uint32_t cap, uint32_t *d_stream_frames,
                                                      uint64_t *d_stream_samples, bnflac_resync_rec *d_resync,
                                                      uint32_t *d_status, void *hs) {
    if (check_args(ctx, d_bytes, nbytes, sp, "bnflac_index_streams_resync")) return -1;
    if (const char *why = resync_refusal(sp)) return fail(std::string("bnflac_index_streams_resync: ") + why);
    DevGuard dg(ctx->device); /* launches and scratch on the context's device */
    if (!d_stream_frames || !d_status || (cap && !d_frame_offsets)) return fail("bnflac_index_streams_resync: null output");
    if (nstreams && !d_streams) return fail("bnflac_index_streams_resync: null descriptor table");
    if (nstreams >= (1u << 30)) return fail("bnflac_index_streams_resync: too many streams");
    hipStream_t s = (hipStream_t)hs;
    ctx->crcp_bytes = ctx->crcp_info = nullptr; /* the records this writes carry no CRC-16 hand-off */
    ctx->rs_ct = nullptr;
    if (!nstreams || !nbytes) { /* nothing to index: zeros */
        hipError_t e = hipMemsetAsync(d_status, 0, 4 * sizeof(uint32_t), s);
        if (e == hipSuccess) e = hipMemsetAsync(d_stream_frames, 0, sizeof(uint32_t) * ((size_t)nstreams + 1), s);
        if (e == hipSuccess && d_stream_samples)
            e = hipMemsetAsync(d_stream_samples, 0, sizeof(uint64_t) * ((size_t)nstreams + 1), s);
        if (e == hipSuccess && d_resync && nstreams) e = hipMemsetAsync(d_resync, 0, sizeof(bnf_resync_rec) * (size_t)nstreams, s);
        return e == hipSuccess ? 0 : fail(std::string("bnflac_index_streams_resync: ") + hipGetErrorString(e));
    }
    const uint64_t C64 = cand_cap ? cand_cap : nbytes / 1024 + 4096;
    if (C64 >= (1u << 30)) return fail("bnflac_index_streams_resync: cand_cap too large");
    const uint32_t C = (uint32_t)C64;
    bnf_ms_scratch w;
    uint8_t *extra = nullptr;
    if (!ms_scratch(ctx, C, nstreams, nbytes, (size_t)bnf_resync_scratch_bytes(C, nstreams), w, &extra))
        return fail("bnflac_index_streams_resync: out of device memory");
    const bnf_rs_scratch r = bnf_resync_carve(extra, C, nstreams);
    bnf_stream_params p;
    memcpy(&p, sp, sizeof p);
    hipError_t e = bnf_launch_chain_streams_resync(d_bytes, nbytes, (const bnf_stream_desc *)d_streams, nstreams, p, C, w, r,
                                                   d_frame_offsets, d_out_sample, (bnf_frame_info *)d_info, cap,
                                                   d_stream_frames, d_stream_samples, (bnf_resync_rec *)d_resync, d_status, s);
    if (e != hipSuccess) return fail(std::string("bnflac_index_streams_resync: ") + hipGetErrorString(e));
    ctx->rs_ct = r.ct;
    ctx->rs_ctl = w.ctl;
    return 0;
}

extern "C" BNFLAC_API int bnflac_debug_index_candidates(bnflac_ctx *ctx, bnflac_index_cand *out, uint32_t cap,
                                                        uint32_t *ncand) {
    if (!ctx || !ncand || (cap && !out)) return fail("bnflac_debug_index_candidates: null argument");
    if (!ctx->rs_ct) return fail("bnflac_debug_index_candidates: no resync call on this context since its scratch was reused");
    DevGuard dg(ctx->device);
    uint32_t ctl[BNF_MS_CTL_WORDS];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(ctl, ctx->rs_ctl, sizeof ctl, hipMemcpyDeviceToHost) != hipSuccess)
        return fail("bnflac_debug_index_candidates: HIP error");
    *ncand = ctl[BNF_MS_N];
    const uint32_t k = std::min(ctl[BNF_MS_N], cap);
    if (k && hipMemcpy(out, ctx->rs_ct, sizeof(bnf_index_cand) * (size_t)k, hipMemcpyDeviceToHost) != hipSuccess)
        return fail("bnflac_debug_index_candidates: HIP error");
    return 0;
}

extern "C" BNFLAC_API int bnflac_resync_plan_host(const bnflac_index_cand *cands, uint32_t ncand,
                                                  const bnflac_stream_desc *streams, uint32_t nstreams, uint32_t B,
                                                  bnflac_resync_slot *slots, uint32_t cap, uint32_t *stream_frames,
                                                  uint64_t *stream_samples, bnflac_resync_rec *resync, uint32_t status[4]) {
    if (!stream_frames || !stream_samples || !status) return fail("bnflac_resync_plan_host: null output");
    if ((ncand && !cands) || (nstreams && !streams)) return fail("bnflac_resync_plan_host: null table");
    if (B < 1) return fail("bnflac_resync_plan_host: the blocksize must be at least 1");
    if (ncand >= (1u << 30) || nstreams >= (1u << 30)) return fail("bnflac_resync_plan_host: table too large");
    if (!bnf_resync_plan_host((const bnf_index_cand *)cands, ncand, (const bnf_stream_desc *)streams, nstreams, B,
                              (bnf_resync_slot *)slots, cap, stream_frames, stream_samples, (bnf_resync_rec *)resync, status))
        return fail("bnflac_resync_plan_host: out of memory");
    return 0;
}

static_assert(sizeof(bnflac_stream_meta) == sizeof(bnf_stream_meta) && sizeof(bnf_stream_meta) == 64, "stream meta layout");
static_assert(offsetof(bnflac_stream_meta, sp) == 16 && offsetof(bnf_stream_meta, sp) == 16, "stream meta: sp @16");
static_assert(offsetof(bnflac_stream_meta, min_framesize) == 48 && offsetof(bnf_stream_meta, min_framesize) == 48,
              "stream meta: min_framesize @48");
static_assert(offsetof(bnflac_stream_meta, first_offset) == 56 && offsetof(bnf_stream_meta, first_offset) == 56,
              "stream meta: first_offset @56");
static_assert(sizeof(bnflac_stream_params) == sizeof(bnf_stream_params), "stream params layout");
static_assert((int)BNFLAC_SCAN_BAD_RANGE == (int)BNF_SCAN_BAD_RANGE && (int)BNFLAC_SCAN_MAX_BLOCKS == (int)BNF_SCAN_MAX_BLOCKS,
              "scan status codes");

extern "C" BNFLAC_API int bnflac_scan_streams(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes,
                                              bnflac_stream_desc *d_streams, uint32_t nstreams,
                                              const bnflac_stream_params *expect, bnflac_stream_meta *d_meta,
                                              uint8_t *d_md5_expected, uint32_t *d_status, void *hs) {
    if (!ctx) return fail("bnflac_scan_streams: null ctx");
    DevGuard dg(ctx->device); /* the launch on the context's device */
    if (!d_status) return fail("bnflac_scan_streams: null d_status");
    if (nstreams && !d_streams) return fail("bnflac_scan_streams: null descriptor table");
    if (nbytes && !d_bytes) return fail("bnflac_scan_streams: null d_bytes");
    if (((uintptr_t)d_bytes) & 15u) return fail("bnflac_scan_streams: d_bytes must be 16-byte aligned");
    if ((((uintptr_t)d_streams) | ((uintptr_t)d_meta)) & 7u)
        return fail("bnflac_scan_streams: d_streams and d_meta must be 8-byte aligned");
    if (((uintptr_t)d_status) & 3u) return fail("bnflac_scan_streams: d_status must be 4-byte aligned");
    if (nbytes >= (1ull << 34)) return fail("bnflac_scan_streams: buffer larger than 16 GiB");
    if (nstreams >= (1u << 30)) return fail("bnflac_scan_streams: too many streams");
    bnf_stream_params x;
    if (expect) memcpy(&x, expect, sizeof x);
    hipError_t e = bnf_launch_scan_streams(d_bytes, nbytes, (bnf_stream_desc *)d_streams, nstreams, expect ? &x : nullptr,
                                           (bnf_stream_meta *)d_meta, d_md5_expected, d_status, (hipStream_t)hs);
    return e == hipSuccess ? 0 : fail(std::string("bnflac_scan_streams: ") + hipGetErrorString(e));
}

extern "C" BNFLAC_API int bnflac_scan_stream_host(const uint8_t *bytes, uint64_t nbytes, bnflac_stream_meta *meta,
                                                  uint8_t md5[16]) {
    if (!meta || (nbytes && !bytes)) return fail("bnflac_scan_stream_host: null argument");
    bnf_stream_meta m;
    uint64_t first, total;
    uint32_t sum[4];
    bnf_metadata_scan(bnf_bytes{bytes}, 0, nbytes, false, nullptr, m, first, total, sum);
    memcpy(meta, &m, sizeof m);
    if (md5)
        for (int i = 0; i < 16; i++) md5[i] = (uint8_t)(sum[i >> 2] >> (8 * (i & 3)));
    return 0;
}

static_assert(sizeof(bnflac_sample_range) == sizeof(bnf_sample_range) && sizeof(bnf_sample_range) == 16, "sample range layout");
static_assert(sizeof(bnflac_window) == sizeof(bnf_window) && sizeof(bnf_window) == 32, "window layout");
static_assert(offsetof(bnflac_window, skip) == 16 && offsetof(bnf_window, skip) == 16 &&
                  offsetof(bnflac_window, flags) == 28 && offsetof(bnf_window, flags) == 28,
              "window: skip @16, flags @28");
static_assert(sizeof(bnflac_frame_info) == sizeof(bnf_frame_info) && sizeof(bnf_frame_info) == 128 &&
                  offsetof(bnf_frame_info, out_sample) == 64,
              "frame record: 128 bytes, out_sample @64");

extern "C" BNFLAC_API int bnflac_select_ranges(bnflac_ctx *ctx, const uint64_t *d_frame_offsets,
                                               const bnflac_frame_info *d_info, uint32_t cap,
                                               const uint32_t *d_stream_frames, const uint64_t *d_stream_samples,
                                               uint32_t nstreams, const bnflac_sample_range *d_ranges,
                                               uint64_t *d_sel_offsets, bnflac_frame_info *d_sel_info, uint32_t sel_cap,
                                               uint32_t *d_sel_frames, uint64_t *d_sel_samples, bnflac_window *d_windows,
                                               uint32_t *d_status, void *hs) {
    if (!ctx) return fail("bnflac_select_ranges: null ctx");
    DevGuard dg(ctx->device); /* launches and scratch on the context's device */
    if (!d_status || !d_sel_frames || !d_sel_samples || (sel_cap && !d_sel_info))
        return fail("bnflac_select_ranges: null output");
    if (nstreams && (!d_stream_frames || !d_stream_samples || !d_ranges || !d_windows))
        return fail("bnflac_select_ranges: null table");
    if (cap && nstreams && !d_info) return fail("bnflac_select_ranges: null d_info");
    if (d_sel_offsets && cap && nstreams && !d_frame_offsets)
        return fail("bnflac_select_ranges: d_sel_offsets without d_frame_offsets");
    if ((((uintptr_t)d_info) | ((uintptr_t)d_sel_info)) & 15u)
        return fail("bnflac_select_ranges: d_info and d_sel_info must be 16-byte aligned");
    if ((((uintptr_t)d_frame_offsets) | ((uintptr_t)d_stream_samples) | ((uintptr_t)d_ranges) | ((uintptr_t)d_sel_offsets) |
         ((uintptr_t)d_sel_samples) | ((uintptr_t)d_windows)) & 7u)
        return fail("bnflac_select_ranges: the 64-bit tables must be 8-byte aligned");
    if ((((uintptr_t)d_stream_frames) | ((uintptr_t)d_sel_frames) | ((uintptr_t)d_status)) & 3u)
        return fail("bnflac_select_ranges: the 32-bit tables must be 4-byte aligned");
    if (nstreams >= (1u << 30)) return fail("bnflac_select_ranges: too many streams");
    /* a floor of 4 KiB: batches of up to 340,000 streams never grow it again */
    if (!ctx->sel.grow(std::max<size_t>((size_t)bnf_select_scratch_bytes(nstreams), 4096)))
        return fail("bnflac_select_ranges: out of device memory");
    hipError_t e = bnf_launch_select_ranges(d_frame_offsets, (const bnf_frame_info *)d_info, cap, d_stream_frames,
                                            d_stream_samples, nstreams, (const bnf_sample_range *)d_ranges, d_sel_offsets,
                                            (bnf_frame_info *)d_sel_info, sel_cap, d_sel_frames, d_sel_samples,
                                            (bnf_window *)d_windows, d_status, ctx->sel.p, (hipStream_t)hs);
    return e == hipSuccess ? 0 : fail(std::string("bnflac_select_ranges: ") + hipGetErrorString(e));
}

extern "C" BNFLAC_API int bnflac_select_ranges_host(const bnflac_frame_info *info, uint32_t cap,
                                                    const uint32_t *stream_frames, const uint64_t *stream_samples,
                                                    uint32_t nstreams, const bnflac_sample_range *ranges,
                                                    bnflac_frame_info *sel_info, uint32_t sel_cap, uint32_t *sel_frames,
                                                    uint64_t *sel_samples, bnflac_window *windows, uint32_t status[4]) {
    if (!status || !sel_frames || !sel_samples || (sel_cap && !sel_info))
        return fail("bnflac_select_ranges_host: null output");
    if (nstreams && (!stream_frames || !stream_samples || !ranges || !windows))
        return fail("bnflac_select_ranges_host: null table");
    if (cap && nstreams && !info) return fail("bnflac_select_ranges_host: null info");
    bnf_select_ranges_host(nullptr, (const bnf_frame_info *)info, cap, stream_frames, stream_samples, nstreams,
                           (const bnf_sample_range *)ranges, nullptr, (bnf_frame_info *)sel_info, sel_cap, sel_frames,
                           sel_samples, (bnf_window *)windows, status);
    return 0;
}

static_assert(sizeof(bnflac_window_request) == sizeof(bnf_window_request) && sizeof(bnf_window_request) == 24 &&
                  offsetof(bnflac_window_request, first_sample) == 8 && offsetof(bnf_window_request, first_sample) == 8,
              "window request layout");
static_assert((int)BNFLAC_WIN_NO_STREAM == (int)BNF_WIN_NO_STREAM, "window flags");

extern "C" BNFLAC_API int bnflac_select_windows(bnflac_ctx *ctx, const uint64_t *d_frame_offsets,
                                                const bnflac_frame_info *d_info, uint32_t cap,
                                                const uint32_t *d_stream_frames, const uint64_t *d_stream_samples,
                                                uint32_t nstreams, const bnflac_window_request *d_requests,
                                                uint32_t nwindows, uint64_t *d_sel_offsets, bnflac_frame_info *d_sel_info,
                                                uint32_t sel_cap, uint32_t *d_sel_frames, uint64_t *d_sel_samples,
                                                bnflac_window *d_windows, uint32_t *d_status, void *hs) {
    if (!ctx) return fail("bnflac_select_windows: null ctx");
    DevGuard dg(ctx->device); /* launches and scratch on the context's device */
    if (!d_status || !d_sel_frames || !d_sel_samples || (sel_cap && !d_sel_info))
        return fail("bnflac_select_windows: null output");
    if (nwindows && (!d_requests || !d_windows)) return fail("bnflac_select_windows: null table");
    if (nwindows && nstreams && (!d_stream_frames || !d_stream_samples)) return fail("bnflac_select_windows: null table");
    if (cap && nstreams && nwindows && !d_info) return fail("bnflac_select_windows: null d_info");
    if (d_sel_offsets && cap && nstreams && nwindows && !d_frame_offsets)
        return fail("bnflac_select_windows: d_sel_offsets without d_frame_offsets");
    if ((((uintptr_t)d_info) | ((uintptr_t)d_sel_info)) & 15u)
        return fail("bnflac_select_windows: d_info and d_sel_info must be 16-byte aligned");
    if (((uintptr_t)d_requests) & 7u) return fail("bnflac_select_windows: d_requests must be 8-byte aligned");
    if ((((uintptr_t)d_frame_offsets) | ((uintptr_t)d_stream_samples) | ((uintptr_t)d_sel_offsets) |
         ((uintptr_t)d_sel_samples) | ((uintptr_t)d_windows)) & 7u)
        return fail("bnflac_select_windows: the 64-bit tables must be 8-byte aligned");
    if ((((uintptr_t)d_stream_frames) | ((uintptr_t)d_sel_frames) | ((uintptr_t)d_status)) & 3u)
        return fail("bnflac_select_windows: the 32-bit tables must be 4-byte aligned");
    if (nwindows >= (1u << 30)) return fail("bnflac_select_windows: too many windows");
    /* the scratch of bnflac_select_ranges, which only ever grows; 64 KiB: up to 8,000 windows never grow it again */
    if (!ctx->sel.grow(std::max<size_t>((size_t)bnf_select_windows_scratch_bytes(nwindows), 65536)))
        return fail("bnflac_select_windows: out of device memory");
    hipError_t e = bnf_launch_select_windows(d_frame_offsets, (const bnf_frame_info *)d_info, cap, d_stream_frames,
                                             d_stream_samples, nstreams, (const bnf_window_request *)d_requests, nwindows,
                                             d_sel_offsets, (bnf_frame_info *)d_sel_info, sel_cap, d_sel_frames,
                                             d_sel_samples, (bnf_window *)d_windows, d_status, ctx->sel.p, (hipStream_t)hs);
    return e == hipSuccess ? 0 : fail(std::string("bnflac_select_windows: ") + hipGetErrorString(e));
}

extern "C" BNFLAC_API int bnflac_select_windows_host(const bnflac_frame_info *info, uint32_t cap,
                                                     const uint32_t *stream_frames, const uint64_t *stream_samples,
                                                     uint32_t nstreams, const bnflac_window_request *requests,
                                                     uint32_t nwindows, bnflac_frame_info *sel_info, uint32_t sel_cap,
                                                     uint32_t *sel_frames, uint64_t *sel_samples, bnflac_window *windows,
                                                     uint32_t status[4]) {
    if (!status || !sel_frames || !sel_samples || (sel_cap && !sel_info))
        return fail("bnflac_select_windows_host: null output");
    if (nwindows && (!requests || !windows)) return fail("bnflac_select_windows_host: null table");
    if (nwindows && nstreams && (!stream_frames || !stream_samples)) return fail("bnflac_select_windows_host: null table");
    if (cap && nstreams && nwindows && !info) return fail("bnflac_select_windows_host: null info");
    if (nwindows >= (1u << 30)) return fail("bnflac_select_windows_host: too many windows");
    bnf_select_windows_host(nullptr, (const bnf_frame_info *)info, cap, stream_frames, stream_samples, nstreams,
                            (const bnf_window_request *)requests, nwindows, nullptr, (bnf_frame_info *)sel_info, sel_cap,
                            sel_frames, sel_samples, (bnf_window *)windows, status);
    return 0;
}

extern "C" BNFLAC_API int bnflac_select_windows_shared(bnflac_ctx *ctx, const uint64_t *d_frame_offsets,
                                                       const bnflac_frame_info *d_info, uint32_t cap,
                                                       const uint32_t *d_stream_frames, const uint64_t *d_stream_samples,
                                                       uint32_t nstreams, const bnflac_window_request *d_requests,
                                                       uint32_t nwindows, uint64_t *d_sel_offsets,
                                                       bnflac_frame_info *d_sel_info, uint32_t sel_cap,
                                                       bnflac_window *d_windows, uint32_t *d_win_sel_first,
                                                       uint64_t *d_sel_totals, uint32_t *d_status, void *hs) {
    if (!ctx) return fail("bnflac_select_windows_shared: null ctx");
    DevGuard dg(ctx->device); /* launches and scratch on the context's device */
    if (!d_status || !d_sel_totals || (sel_cap && !d_sel_info)) return fail("bnflac_select_windows_shared: null output");
    if (nwindows && (!d_requests || !d_windows)) return fail("bnflac_select_windows_shared: null table");
    if (nwindows && nstreams && (!d_stream_frames || !d_stream_samples))
        return fail("bnflac_select_windows_shared: null table");
    if (cap && nstreams && nwindows && !d_info) return fail("bnflac_select_windows_shared: null d_info");
    if (d_sel_offsets && cap && nstreams && nwindows && !d_frame_offsets)
        return fail("bnflac_select_windows_shared: d_sel_offsets without d_frame_offsets");
    if ((((uintptr_t)d_info) | ((uintptr_t)d_sel_info)) & 15u)
        return fail("bnflac_select_windows_shared: d_info and d_sel_info must be 16-byte aligned");
    if (((uintptr_t)d_requests) & 7u) return fail("bnflac_select_windows_shared: d_requests must be 8-byte aligned");
    if (((uintptr_t)d_sel_totals) & 7u) return fail("bnflac_select_windows_shared: d_sel_totals must be 8-byte aligned");
    if ((((uintptr_t)d_frame_offsets) | ((uintptr_t)d_stream_samples) | ((uintptr_t)d_sel_offsets) | ((uintptr_t)d_windows)) & 7u)
        return fail("bnflac_select_windows_shared: the 64-bit tables must be 8-byte aligned");
    if ((((uintptr_t)d_stream_frames) | ((uintptr_t)d_win_sel_first) | ((uintptr_t)d_status)) & 3u)
        return fail("bnflac_select_windows_shared: the 32-bit tables must be 4-byte aligned");
    if (nwindows >= (1u << 30)) return fail("bnflac_select_windows_shared: too many windows");
    /* the scratch of bnflac_select_ranges, which only ever grows: 16 bytes per position of the index */
    if (!ctx->sel.grow(std::max<size_t>((size_t)bnf_select_shared_scratch_bytes(cap, nwindows), 65536)))
        return fail("bnflac_select_windows_shared: out of device memory");
    hipError_t e = bnf_launch_select_windows_shared(d_frame_offsets, (const bnf_frame_info *)d_info, cap, d_stream_frames,
                                                    d_stream_samples, nstreams, (const bnf_window_request *)d_requests,
                                                    nwindows, d_sel_offsets, (bnf_frame_info *)d_sel_info, sel_cap,
                                                    (bnf_window *)d_windows, d_win_sel_first, d_sel_totals, d_status,
                                                    ctx->sel.p, (hipStream_t)hs);
    return e == hipSuccess ? 0 : fail(std::string("bnflac_select_windows_shared: ") + hipGetErrorString(e));
}

extern "C" BNFLAC_API int bnflac_select_windows_shared_host(const bnflac_frame_info *info, uint32_t cap,
                                                            const uint32_t *stream_frames, const uint64_t *stream_samples,
                                                            uint32_t nstreams, const bnflac_window_request *requests,
                                                            uint32_t nwindows, bnflac_frame_info *sel_info, uint32_t sel_cap,
                                                            bnflac_window *windows, uint32_t *win_sel_first,
                                                            uint64_t sel_totals[2], uint32_t status[4]) {
    if (!status || !sel_totals || (sel_cap && !sel_info)) return fail("bnflac_select_windows_shared_host: null output");
    if (nwindows && (!requests || !windows)) return fail("bnflac_select_windows_shared_host: null table");
    if (nwindows && nstreams && (!stream_frames || !stream_samples))
        return fail("bnflac_select_windows_shared_host: null table");
    if (cap && nstreams && nwindows && !info) return fail("bnflac_select_windows_shared_host: null info");
    if (nwindows >= (1u << 30)) return fail("bnflac_select_windows_shared_host: too many windows");
    if (!bnf_select_windows_shared_host(nullptr, (const bnf_frame_info *)info, cap, stream_frames, stream_samples, nstreams,
                                        (const bnf_window_request *)requests, nwindows, nullptr, (bnf_frame_info *)sel_info,
                                        sel_cap, (bnf_window *)windows, win_sel_first, sel_totals, status))
        return fail("bnflac_select_windows_shared_host: out of memory");
    return 0;
}

static_assert(sizeof(bnflac_window_health_rec) == sizeof(bnf_window_health) && sizeof(bnf_window_health) == 32 &&
                  offsetof(bnflac_window_health_rec, bad_samples) == 16 && offsetof(bnf_window_health, bad_samples) == 16 &&
                  offsetof(bnflac_window_health_rec, missing) == 24 && offsetof(bnf_window_health, missing) == 24,
              "window health record: 32 bytes, bad_samples @16, missing @24");
static_assert(sizeof(bnflac_stream_desc) == sizeof(bnf_stream_desc) &&
                  offsetof(bnflac_stream_desc, total_samples) == offsetof(bnf_stream_desc, total_samples),
              "stream descriptor layout");
static_assert((int)BNFLAC_HEALTH_DAMAGED == (int)BNF_HEALTH_DAMAGED && (int)BNFLAC_HEALTH_SHORT == (int)BNF_HEALTH_SHORT &&
                  (int)BNFLAC_HEALTH_UNKNOWN == (int)BNF_HEALTH_UNKNOWN && (int)BNFLAC_HEALTH_EMPTY == (int)BNF_HEALTH_EMPTY &&
                  (int)BNFLAC_HEALTH_NO_STREAM == (int)BNF_HEALTH_NO_STREAM,
              "window health flags");

extern "C" BNFLAC_API int bnflac_window_health(bnflac_ctx *ctx, const bnflac_frame_info *d_sel_info, uint32_t sel_cap,
                                               const bnflac_window *d_windows, const uint32_t *d_first, uint32_t nwindows,
                                               const bnflac_window_request *d_requests, const bnflac_stream_desc *d_streams,
                                               const uint64_t *d_stream_samples, uint32_t nstreams,
                                               bnflac_window_health_rec *d_health, uint32_t *d_status, void *hs) {
    if (!ctx) return fail("bnflac_window_health: null ctx");
    DevGuard dg(ctx->device); /* launches and scratch on the context's device */
    if (!d_health || !d_status) return fail("bnflac_window_health: null output");
    if (!d_sel_info || !d_windows || !d_first) return fail("bnflac_window_health: null table");
    if ((!d_requests || !d_streams || !d_stream_samples) && (d_requests || d_streams || d_stream_samples))
        return fail("bnflac_window_health: d_requests, d_streams and d_stream_samples are all given or all null");
    if (((uintptr_t)d_sel_info) & 15u) return fail("bnflac_window_health: d_sel_info must be 16-byte aligned");
    if ((((uintptr_t)d_windows) | ((uintptr_t)d_requests) | ((uintptr_t)d_streams) | ((uintptr_t)d_stream_samples) |
         ((uintptr_t)d_health)) & 7u)
        return fail("bnflac_window_health: the 64-bit tables must be 8-byte aligned");
    if ((((uintptr_t)d_first) | ((uintptr_t)d_status)) & 3u)
        return fail("bnflac_window_health: the 32-bit tables must be 4-byte aligned");
    if (nwindows >= (1u << 30)) return fail("bnflac_window_health: too many windows");
    /* the scratch of bnflac_select_ranges, which only ever grows: 24 bytes per position of the selection */
    if (!ctx->sel.grow(std::max<size_t>((size_t)bnf_window_health_scratch_bytes(sel_cap, nwindows), 65536)))
        return fail("bnflac_window_health: out of device memory");
    hipError_t e = bnf_launch_window_health((const bnf_frame_info *)d_sel_info, sel_cap, (const bnf_window *)d_windows, d_first,
                                            nwindows, (const bnf_window_request *)d_requests,
                                            (const bnf_stream_desc *)d_streams, d_stream_samples, nstreams,
                                            (bnf_window_health *)d_health, d_status, ctx->sel.p, (hipStream_t)hs);
    return e == hipSuccess ? 0 : fail(std::string("bnflac_window_health: ") + hipGetErrorString(e));
}

extern "C" BNFLAC_API int bnflac_window_health_host(const bnflac_frame_info *sel_info, uint32_t sel_cap,
                                                    const bnflac_window *windows, const uint32_t *first, uint32_t nwindows,
                                                    const bnflac_window_request *requests, const bnflac_stream_desc *streams,
                                                    const uint64_t *stream_samples, uint32_t nstreams,
                                                    bnflac_window_health_rec *health, uint32_t status[4]) {
    if (!health || !status) return fail("bnflac_window_health_host: null output");
    if (!sel_info || !windows || !first) return fail("bnflac_window_health_host: null table");
    if ((!requests || !streams || !stream_samples) && (requests || streams || stream_samples))
        return fail("bnflac_window_health_host: requests, streams and stream_samples are all given or all null");
    if (nwindows >= (1u << 30)) return fail("bnflac_window_health_host: too many windows");
    if (!bnf_window_health_host((const bnf_frame_info *)sel_info, sel_cap, (const bnf_window *)windows, first, nwindows,
                                (const bnf_window_request *)requests, (const bnf_stream_desc *)streams, stream_samples,
                                nstreams, (bnf_window_health *)health, status))
        return fail("bnflac_window_health_host: out of memory");
    return 0;
}

extern "C" BNFLAC_API int bnflac_gather_ranges(bnflac_ctx *ctx, const uint8_t *d_pcm, uint64_t pcm_bytes, int fmt,
                                               const bnflac_stream_params *sp, const bnflac_window *d_windows,
                                               uint32_t nstreams, uint32_t row_samples, uint64_t row_bytes, uint8_t *d_rows,
                                               uint32_t *d_status, void *hs) {
    if (!ctx || !sp) return fail("bnflac_gather_ranges: null argument");
    DevGuard dg(ctx->device); /* the launch on the context's device */
    if (!d_status || (nstreams && (!d_windows || (row_samples && !d_rows)))) return fail("bnflac_gather_ranges: null output");
    if (pcm_bytes && !d_pcm) return fail("bnflac_gather_ranges: null d_pcm");
    if (fmt == BNFLAC_OUT_PLANAR32)
        return fail("bnflac_gather_ranges: BNFLAC_OUT_PLANAR32 is channel-major per frame, a window of it is no byte range");
    if (fmt < 0 || fmt > 3) return fail("bnflac_gather_ranges: bad out_format");
    if (sp->channels < 1 || sp->channels > 8) return fail("bnflac_gather_ranges: channels must be 1..8");
    if ((((uintptr_t)d_pcm) | ((uintptr_t)d_rows)) & 15u)
        return fail("bnflac_gather_ranges: d_pcm and d_rows must be 16-byte aligned");
    if (((uintptr_t)d_windows) & 7u) return fail("bnflac_gather_ranges: d_windows must be 8-byte aligned");
    if (nstreams >= (1u << 30)) return fail("bnflac_gather_ranges: too many streams");
    const uint32_t stride = bnflac_out_stride(fmt, sp);
    if (row_bytes < (uint64_t)row_samples * stride) return fail("bnflac_gather_ranges: row_bytes below row_samples * stride");
    hipError_t e = bnf_launch_gather_ranges(d_pcm, pcm_bytes, stride, (const bnf_window *)d_windows, nstreams, row_samples,
                                            row_bytes, d_rows, d_status, (hipStream_t)hs);
    return e == hipSuccess ? 0 : fail(std::string("bnflac_gather_ranges: ") + hipGetErrorString(e));
}

/* What both bnflac_gather_ranges_f32 calls refuse apart from pointers; fills stride and unit. */
static const char *gather_f32_refusal(int fmt, const bnflac_stream_params *sp, uint32_t nstreams, uint32_t row_samples,
                                      uint64_t plane_pitch, uint32_t flags, uint32_t &stride, uint32_t &unit) {
    if (fmt == BNFLAC_OUT_PLANAR32) return "BNFLAC_OUT_PLANAR32 is channel-major per frame, a window of it is no byte range";
    if (fmt < 0 || fmt > 3) return "bad out_format";
    if (sp->channels < 1 || sp->channels > 8) return "channels must be 1..8";
    if (!bnflac_md5_layout(fmt, sp)) return "the layout's bytes are not the samples (bnflac_md5_layout is 0)";
    if (flags & ~(uint32_t)BNFLAC_F32_MONO) return "unknown flags";
    if (plane_pitch < row_samples) return "plane_pitch below row_samples";
    if (nstreams >= (1u << 30)) return "too many streams";
    stride = bnflac_out_stride(fmt, sp);
    unit = stride / sp->channels;
    return nullptr;
}

extern "C" BNFLAC_API int bnflac_gather_ranges_f32(bnflac_ctx *ctx, const uint8_t *d_pcm, uint64_t pcm_bytes, int fmt,
                                                   const bnflac_stream_params *sp, const bnflac_window *d_windows,
                                                   uint32_t nstreams, uint32_t row_samples, uint64_t plane_pitch,
                                                   uint32_t flags, float *d_out, uint32_t *d_status, void *hs) {
    if (!ctx || !sp) return fail("bnflac_gather_ranges_f32: null argument");
    DevGuard dg(ctx->device); /* the launch on the context's device */
    if (!d_status || (nstreams && (!d_windows || (row_samples && !d_out)))) return fail("bnflac_gather_ranges_f32: null output");
    if (pcm_bytes && !d_pcm) return fail("bnflac_gather_ranges_f32: null d_pcm");
    uint32_t stride = 0, unit = 0;
    if (const char *why = gather_f32_refusal(fmt, sp, nstreams, row_samples, plane_pitch, flags, stride, unit))
        return fail(std::string("bnflac_gather_ranges_f32: ") + why);
    if ((((uintptr_t)d_pcm) | ((uintptr_t)d_out)) & 15u)
        return fail("bnflac_gather_ranges_f32: d_pcm and d_out must be 16-byte aligned");
    if (((uintptr_t)d_windows) & 7u) return fail("bnflac_gather_ranges_f32: d_windows must be 8-byte aligned");
    hipError_t e = bnf_launch_gather_f32(d_pcm, pcm_bytes, stride, unit, sp->bps, sp->channels, flags,
                                         (const bnf_window *)d_windows, nstreams, row_samples, plane_pitch, d_out, d_status,
                                         (hipStream_t)hs);
    return e == hipSuccess ? 0 : fail(std::string("bnflac_gather_ranges_f32: ") + hipGetErrorString(e));
}

extern "C" BNFLAC_API int bnflac_gather_ranges_f32_host(const uint8_t *pcm, uint64_t pcm_bytes, int fmt,
                                                        const bnflac_stream_params *sp, const bnflac_window *windows,
                                                        uint32_t nstreams, uint32_t row_samples, uint64_t plane_pitch,
                                                        uint32_t flags, float *out, uint32_t status[4]) {
    if (!sp) return fail("bnflac_gather_ranges_f32_host: null argument");
    if (!status || (nstreams && (!windows || (row_samples && !out)))) return fail("bnflac_gather_ranges_f32_host: null output");
    if (pcm_bytes && !pcm) return fail("bnflac_gather_ranges_f32_host: null pcm");
    uint32_t stride = 0, unit = 0;
    if (const char *why = gather_f32_refusal(fmt, sp, nstreams, row_samples, plane_pitch, flags, stride, unit))
        return fail(std::string("bnflac_gather_ranges_f32_host: ") + why);
    if (bnf_gather_f32_host(pcm, pcm_bytes, stride, unit, sp->bps, sp->channels, flags, (const bnf_window *)windows, nstreams,
                            row_samples, plane_pitch, out, status) != 0)
        return fail("bnflac_gather_ranges_f32_host: out of memory");
    return 0;
}

static_assert(sizeof(bnflac_resample_spec) == sizeof(bnf_rsmp_spec) && sizeof(bnf_rsmp_spec) == 16, "bnflac_resample_spec");

extern "C" BNFLAC_API int bnflac_gather_ranges_f32_rs(bnflac_ctx *ctx, const uint8_t *d_pcm, uint64_t pcm_bytes, int fmt,
                                                      const bnflac_stream_params *sp, const bnflac_window *d_windows,
                                                      uint32_t nstreams, const bnflac_resample_spec *spec,
                                                      const float *d_taps, uint32_t row_out, uint64_t plane_pitch,
                                                      uint32_t flags, float *d_out, uint32_t *d_status, void *hs) {
    if (!ctx || !sp || !spec) return fail("bnflac_gather_ranges_f32_rs: null argument");
    DevGuard dg(ctx->device); /* the launch on the context's device */
    if (!d_status || (nstreams && (!d_windows || (row_out && !d_out)))) return fail("bnflac_gather_ranges_f32_rs: null output");
    if (pcm_bytes && !d_pcm) return fail("bnflac_gather_ranges_f32_rs: null d_pcm");
    if (!d_taps) return fail("bnflac_gather_ranges_f32_rs: null d_taps");
    bnf_rsmp_spec rs;
    memcpy(&rs, spec, sizeof rs);
    if (const char *why = bnf_rsmp_spec_refusal(rs, row_out)) return fail(std::string("bnflac_gather_ranges_f32_rs: ") + why);
    uint32_t stride = 0, unit = 0;
    if (const char *why = gather_f32_refusal(fmt, sp, nstreams, row_out, plane_pitch, flags, stride, unit))
        return fail(std::string("bnflac_gather_ranges_f32_rs: ") + why);
    if ((((uintptr_t)d_pcm) | ((uintptr_t)d_out) | ((uintptr_t)d_taps)) & 15u)
        return fail("bnflac_gather_ranges_f32_rs: d_pcm, d_out and d_taps must be 16-byte aligned");
    if (((uintptr_t)d_windows) & 7u) return fail("bnflac_gather_ranges_f32_rs: d_windows must be 8-byte aligned");
    hipError_t e = bnf_launch_gather_f32_rs(d_pcm, pcm_bytes, stride, unit, sp->bps, sp->channels, flags,
                                            (const bnf_window *)d_windows, nstreams, &rs, d_taps, row_out, plane_pitch, d_out,
                                            d_status, (hipStream_t)hs);
    return e == hipSuccess ? 0 : fail(std::string("bnflac_gather_ranges_f32_rs: ") + hipGetErrorString(e));
}

extern "C" BNFLAC_API int bnflac_gather_ranges_f32_rs_host(const uint8_t *pcm, uint64_t pcm_bytes, int fmt,
                                                           const bnflac_stream_params *sp, const bnflac_window *windows,
                                                           uint32_t nstreams, const bnflac_resample_spec *spec,
                                                           const float *taps, uint32_t row_out, uint64_t plane_pitch,
                                                           uint32_t flags, float *out, uint32_t status[4]) {
    if (!sp || !spec) return fail("bnflac_gather_ranges_f32_rs_host: null argument");
    if (!status || (nstreams && (!windows || (row_out && !out)))) return fail("bnflac_gather_ranges_f32_rs_host: null output");
    if (pcm_bytes && !pcm) return fail("bnflac_gather_ranges_f32_rs_host: null pcm");
    if (!taps) return fail("bnflac_gather_ranges_f32_rs_host: null taps");
    bnf_rsmp_spec rs;
    memcpy(&rs, spec, sizeof rs);
    if (const char *why = bnf_rsmp_spec_refusal(rs, row_out)) return fail(std::string("bnflac_gather_ranges_f32_rs_host: ") + why);
    uint32_t stride = 0, unit = 0;
    if (const char *why = gather_f32_refusal(fmt, sp, nstreams, row_out, plane_pitch, flags, stride, unit))
        return fail(std::string("bnflac_gather_ranges_f32_rs_host: ") + why);
    if (bnf_gather_f32_rs_host(pcm, pcm_bytes, stride, unit, sp->bps, sp->channels, flags, (const bnf_window *)windows, nstreams,
                               rs, taps, row_out, plane_pitch, out, status) != 0)
        return fail("bnflac_gather_ranges_f32_rs_host: out of memory");
    return 0;
}

extern "C" BNFLAC_API int64_t bnflac_resample_design(uint32_t rate_in, uint32_t rate_out, double zeros, double rolloff,
                                                     double beta, bnflac_resample_spec *spec, float *taps, uint64_t taps_cap) {
    if (!spec) return fail("bnflac_resample_design: null spec");
    if (!(zeros > 0.0)) zeros = 16.0;
    if (!(rolloff > 0.0)) rolloff = 0.945;
    if (!(beta > 0.0)) beta = 9.0;
    bnf_rsmp_spec rs;
    uint64_t K = 0;
    const char *why = bnf_rsmp_design_spec(rate_in, rate_out, zeros, rs, K);
    if (why) {
        std::string m = std::string("bnflac_resample_design: ") + why;
        if (K) m += ": needs up = " + std::to_string(rs.up) + " x taps = " + std::to_string(K) + " (up * taps <= 16384, taps <= 512)";
        return fail(m);
    }
    const int64_t need = (int64_t)rs.up * rs.taps;
    memcpy(spec, &rs, sizeof rs);
    if (taps_cap >= (uint64_t)need) {
        if (!taps) return fail("bnflac_resample_design: null taps");
        bnf_rsmp_design_taps(rs, rolloff, beta, taps);
    }
    return need;
}

extern "C" BNFLAC_API int bnflac_resample_request(const bnflac_resample_spec *spec, uint64_t j0, uint64_t n_out,
                                                  uint64_t *first_sample, uint64_t *nsamples, uint32_t *out_first) {
    if (!spec || !first_sample || !nsamples || !out_first) return fail("bnflac_resample_request: null argument");
    bnf_rsmp_spec rs;
    memcpy(&rs, spec, sizeof rs);
    rs.out_first = 0; /* the spec's own is not read */
    if (const char *why = bnf_rsmp_spec_refusal(rs, 0)) return fail(std::string("bnflac_resample_request: ") + why);
    if ((j0 >> 47) || (n_out >> 47) || ((j0 + n_out) >> 47)) return fail("bnflac_resample_request: j0 + n_out must be below 2^47");
    uint64_t of = 0;
    bnf_rsmp_request(rs, j0, n_out, *first_sample, *nsamples, of);
    *out_first = (uint32_t)of; /* below (K / 2 + M + 1) L / M + L < 2^26 */
    return 0;
}

static_assert(sizeof(bnflac_mel_spec) == sizeof(bnf_mel_spec) && sizeof(bnf_mel_spec) == 32, "bnflac_mel_spec");

extern "C" BNFLAC_API int bnflac_gather_ranges_mel(bnflac_ctx *ctx, const uint8_t *d_pcm, uint64_t pcm_bytes, int fmt,
                                                   const bnflac_stream_params *sp, const bnflac_window *d_windows,
                                                   uint32_t nstreams, const bnflac_mel_spec *spec, const float *d_tab,
                                                   const uint32_t *d_bands, uint32_t row_frames, uint64_t frame_pitch,
                                                   uint32_t flags, float *d_out, uint32_t *d_status, void *hs) {
    if (!ctx || !sp || !spec) return fail("bnflac_gather_ranges_mel: null argument");
    DevGuard dg(ctx->device); /* the launch on the context's device */
    if (!d_status || (nstreams && (!d_windows || (row_frames && !d_out)))) return fail("bnflac_gather_ranges_mel: null output");
    if (pcm_bytes && !d_pcm) return fail("bnflac_gather_ranges_mel: null d_pcm");
    if (!d_tab) return fail("bnflac_gather_ranges_mel: null d_tab");
    bnf_mel_spec ms;
    memcpy(&ms, spec, sizeof ms);
    if (ms.n_mels && !d_bands) return fail("bnflac_gather_ranges_mel: null d_bands with n_mels != 0");
    uint32_t stride = 0, unit = 0;
    if (const char *why = gather_f32_refusal(fmt, sp, nstreams, 0, 0, flags, stride, unit))
        return fail(std::string("bnflac_gather_ranges_mel: ") + why);
    if (const char *why = bnf_mel_spec_refusal(ms, row_frames, frame_pitch)) return fail(std::string("bnflac_gather_ranges_mel: ") + why);
    if ((((uintptr_t)d_pcm) | ((uintptr_t)d_out) | ((uintptr_t)d_tab)) & 15u)
        return fail("bnflac_gather_ranges_mel: d_pcm, d_out and d_tab must be 16-byte aligned");
    if (((uintptr_t)d_windows) & 7u) return fail("bnflac_gather_ranges_mel: d_windows must be 8-byte aligned");
    if (((uintptr_t)d_bands) & 3u) return fail("bnflac_gather_ranges_mel: d_bands must be 4-byte aligned");
    hipError_t e = bnf_launch_gather_mel(d_pcm, pcm_bytes, stride, unit, sp->bps, sp->channels, flags,
                                         (const bnf_window *)d_windows, nstreams, &ms, d_tab, d_bands, row_frames, frame_pitch,
                                         d_out, d_status, (hipStream_t)hs);
    return e == hipSuccess ? 0 : fail(std::string("bnflac_gather_ranges_mel: ") + hipGetErrorString(e));
}

extern "C" BNFLAC_API int bnflac_gather_ranges_mel_host(const uint8_t *pcm, uint64_t pcm_bytes, int fmt,
                                                        const bnflac_stream_params *sp, const bnflac_window *windows,
                                                        uint32_t nstreams, const bnflac_mel_spec *spec, const float *tab,
                                                        const uint32_t *bands, uint32_t row_frames, uint64_t frame_pitch,
                                                        uint32_t flags, float *out, uint32_t status[4]) {
    if (!sp || !spec) return fail("bnflac_gather_ranges_mel_host: null argument");
    if (!status || (nstreams && (!windows || (row_frames && !out)))) return fail("bnflac_gather_ranges_mel_host: null output");
    if (pcm_bytes && !pcm) return fail("bnflac_gather_ranges_mel_host: null pcm");
    if (!tab) return fail("bnflac_gather_ranges_mel_host: null tab");
    bnf_mel_spec ms;
    memcpy(&ms, spec, sizeof ms);
    if (ms.n_mels && !bands) return fail("bnflac_gather_ranges_mel_host: null bands with n_mels != 0");
    uint32_t stride = 0, unit = 0;
    if (const char *why = gather_f32_refusal(fmt, sp, nstreams, 0, 0, flags, stride, unit))
        return fail(std::string("bnflac_gather_ranges_mel_host: ") + why);
    if (const char *why = bnf_mel_spec_refusal(ms, row_frames, frame_pitch))
        return fail(std::string("bnflac_gather_ranges_mel_host: ") + why);
    if (bnf_gather_mel_host(pcm, pcm_bytes, stride, unit, sp->bps, sp->channels, flags, (const bnf_window *)windows, nstreams, ms,
                            tab, bands, row_frames, frame_pitch, out, status) != 0)
        return fail("bnflac_gather_ranges_mel_host: out of memory");
    return 0;
}

extern "C" BNFLAC_API int64_t bnflac_mel_design(uint32_t sample_rate, uint32_t n_fft, uint32_t hop, uint32_t n_mels, double f_min,
                                                double f_max, bnflac_mel_spec *spec, float *tab, uint64_t tab_cap,
                                                uint32_t *bands, uint64_t bands_cap) {
    if (!spec) return fail("bnflac_mel_design: null spec");
    if (!(f_max > 0.0)) f_max = (double)sample_rate / 2.0;
    bnf_mel_spec ms;
    uint64_t nw = 0;
    const char *why = bnf_mel_design_spec(sample_rate, n_fft, hop, n_mels, f_min, f_max, ms, nw);
    if (why) {
        std::string m = std::string("bnflac_mel_design: ") + why;
        if (nw || n_mels > BNF_MEL_MAX_MELS)
            m += ": needs n_mels = " + std::to_string(n_mels) + " and n_weights = " + std::to_string(nw) +
                 " (n_mels <= 256, n_weights <= 8192)";
        return fail(m);
    }
    const int64_t need = 2 * (int64_t)ms.n_fft + ms.n_weights;
    memcpy(spec, &ms, sizeof ms);
    if (tab_cap >= (uint64_t)need && bands_cap >= (ms.n_mels ? 2u * ((uint64_t)ms.n_mels + 1u) : 0u)) {
        if (!tab || (ms.n_mels && !bands)) return fail("bnflac_mel_design: null table");
        bnf_mel_design_tables(sample_rate, ms, f_min, f_max, tab, bands);
    }
    return need;
}

extern "C" BNFLAC_API int bnflac_mel_request(const bnflac_mel_spec *spec, uint64_t t0, uint64_t n_frames, uint64_t *first_sample,
                                             uint64_t *nsamples, int32_t *origin) {
    if (!spec || !first_sample || !nsamples || !origin) return fail("bnflac_mel_request: null argument");
    bnf_mel_spec ms;
    memcpy(&ms, spec, sizeof ms);
    if (const char *why = bnf_mel_spec_refusal(ms, 0, 0)) return fail(std::string("bnflac_mel_request: ") + why);
    if ((t0 >> 31) || (n_frames >> 31) || ((t0 + n_frames) >> 31)) return fail("bnflac_mel_request: t0 + n_frames must be below 2^31");
    bnf_mel_request(ms, t0, n_frames, *first_sample, *nsamples, *origin);
    return 0;
}

/* ====================================================================== */
/*                 libFLAC-compatible stream decoder                       */
/* ====================================================================== */

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool grow(size_t n) {
        if (n <= cap) return true;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t c = std::max<size_t>(n, 1 << 16);
        c = c + c / 4;
        if (hipMalloc(&p, c) != hipSuccess) return false;
        cap = c;
        return true;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

} // namespace

struct FLAC__StreamDecoder {
    FLAC__StreamDecoderState state = FLAC__STREAM_DECODER_UNINITIALIZED;
    FLAC__StreamDecoderReadCallback read_cb = nullptr;
    FLAC__StreamDecoderSeekCallback seek_cb = nullptr;
    FLAC__StreamDecoderTellCallback tell_cb = nullptr;
    FLAC__StreamDecoderLengthCallback length_cb = nullptr;
    FLAC__StreamDecoderEofCallback eof_cb = nullptr;
    FLAC__StreamDecoderWriteCallback write_cb = nullptr;
    FLAC__StreamDecoderMetadataCallback metadata_cb = nullptr;
    FLAC__StreamDecoderErrorCallback error_cb = nullptr;
    void *client = nullptr;
    FILE *file = nullptr;
    bool ignore_write_status = false;

    /* bytes delivered by the read callback, stream offsets [buf_base, buf_base + buf.size());
     * pos = consumed (absolute).  Bytes below the frame being decoded are dropped once they
     * pile up (trim_consumed); a seek repositions the client and restarts the buffer there. */
    std::vector<uint8_t> buf;
    uint64_t buf_base = 0;
    uint64_t pos = 0;
    uint64_t bitpos_meta = 0; /* bit cursor used while reading metadata */
    bool cached = false;
    uint8_t lookahead = 0;
    uint8_t header_warmup[2] = {0, 0};
    int client_done = 0; /* 1: client reported end of stream, 2: abort */

    bool has_stream_info = false;
    FLAC__StreamMetadata stream_info;
    uint64_t samples_decoded = 0;
    unsigned fixed_block_size = 0, next_fixed_block_size = 0;
    uint64_t first_frame_offset = 0;
    bool is_seeking = false;
    /* MD5 of the decoded PCM vs STREAMINFO md5sum (stream_decoder.c md5_checking /
     * do_md5_checking / md5context); off unless set_md5_checking(true) before init */
    bool md5_checking = false, do_md5 = false;
    Md5 md5;
    uint64_t seek_target = 0;
    int seek_done = 0;
    /* SEEKTABLE points (read_metadata_seektable_): sample number, byte offset from the first
     * frame header, frame samples; placeholders dropped.  Only narrows a seek's search. */
    struct SeekPoint { uint64_t sample, offset; uint32_t frame_samples; };
    std::vector<SeekPoint> seek_table;

    FLAC__Frame frame;
    std::vector<int32_t> output[FLAC__MAX_CHANNELS];
    unsigned output_capacity = 0, output_channels = 0;

    unsigned channels = 0, bits_per_sample = 0, sample_rate = 0, blocksize = 0;
    FLAC__ChannelAssignment channel_assignment = FLAC__CHANNEL_ASSIGNMENT_INDEPENDENT;

    /* GPU window */
    int device = 0;
    bool gpu_ready = false;
    hipStream_t stream = nullptr;
    bnflac_ctx *ctx = nullptr;
    DevBuf d_bytes, d_cand, d_count, d_info, d_pcm;
    uint64_t win_base = 0, win_end = 0;
    bool win_valid = false;
    std::vector<uint64_t> cand;
    std::vector<bnf_frame_info> info;
    std::vector<int32_t> pcm;
    uint32_t pcm_ch = 1;                    /* planar slots per sample in pcm: the window's widest frame */
    uint64_t read_ahead = 32ull << 20;      /* window read-ahead cap */
    uint64_t read_ahead_cur = 256ull << 10; /* grows x2 per window up to the cap: the first frame comes quickly */
};

namespace {

using Dec = FLAC__StreamDecoder;

uint64_t bend(const Dec *d) { return d->buf_base + d->buf.size(); } /* one past the last buffered byte */
uint8_t bat(const Dec *d, uint64_t p) { return d->buf[(size_t)(p - d->buf_base)]; }


/* read_callback_ (stream_decoder.c) semantics, without touching the decoder state:
 * 0 = got bytes, 1 = end of stream, 2 = abort. */
int fill_raw(Dec *d, size_t want = 65536) {
    if (d->client_done) {
        /* libFLAC would ask again: the eof callback answers first */
        if (d->client_done == 2) return 2;
        if (d->eof_cb && d->eof_cb(d, d->client)) return 1;
    }
    for (int spins = 0; spins < 1000000; spins++) {
        if (d->eof_cb && d->eof_cb(d, d->client)) return 1;
        size_t old = d->buf.size();
        size_t bytes = want;
        d->buf.resize(old + bytes);
        FLAC__StreamDecoderReadStatus st = d->read_cb(d, d->buf.data() + old, &bytes, d->client);
        if (bytes > want) bytes = want;
        d->buf.resize(old + bytes);
        if (st == FLAC__STREAM_DECODER_READ_STATUS_ABORT) return 2;
        if (bytes == 0) {
            if (st == FLAC__STREAM_DECODER_READ_STATUS_END_OF_STREAM || (d->eof_cb && d->eof_cb(d, d->client))) return 1;
            continue;
        }
        return 0;
    }
    return 2;
}

/* the decoder genuinely needs bytes [.., upto): failure sets END_OF_STREAM / ABORTED */
bool need_bytes(Dec *d, uint64_t upto) {
    while (bend(d) < upto) {
        int r = fill_raw(d);
        if (r) {
            if (!d->client_done) d->client_done = r;
            d->state = (r == 2) ? FLAC__STREAM_DECODER_ABORTED : FLAC__STREAM_DECODER_END_OF_STREAM;
            return false;
        }
    }
    return true;
}

/* read ahead for the GPU window; hitting the client's end is remembered, not reported */
void read_ahead(Dec *d, uint64_t upto) {
    while (bend(d) < upto && !d->client_done) {
        int r = fill_raw(d);
        if (r) d->client_done = r;
    }
}

/* metadata bit reader on the host buffer */
bool mb_read(Dec *d, uint32_t *v, unsigned bits) {
    if (bits == 0) {
        *v = 0;
        return true;
    }
    uint64_t end = d->bitpos_meta + bits;
    if (!need_bytes(d, (end + 7) / 8)) return false;
    uint64_t x = 0;
    for (uint64_t p = d->bitpos_meta; p < end; p++) x = (x << 1) | ((bat(d, p >> 3) >> (7 - (p & 7))) & 1u);
    d->bitpos_meta = end;
    *v = (uint32_t)x;
    return true;
}

bool mb_byte(Dec *d, uint32_t *x) {
    if (d->cached) {
        *x = d->lookahead;
        d->cached = false;
        return true;
    }
    return mb_read(d, x, 8);
}

void send_error(Dec *d, FLAC__StreamDecoderErrorStatus st) {
    if (!d->is_seeking) d->error_cb(d, st, d->client);
}

bool skip_id3v2(Dec *d) {
    uint32_t x, skip = 0;
    if (!mb_read(d, &x, 24)) return false;
    for (int i = 0; i < 4; i++) {
        if (!mb_read(d, &x, 8)) return false;
        skip = (skip << 7) | (x & 0x7f);
    }
    uint64_t end = d->bitpos_meta + (uint64_t)skip * 8;
    if (!need_bytes(d, end / 8)) return false;
    d->bitpos_meta = end;
    return true;
}

/* find_metadata_ */
bool find_metadata(Dec *d) {
    static const uint8_t sync[4] = {'f', 'L', 'a', 'C'};
    static const uint8_t id3[3] = {'I', 'D', '3'};
    uint32_t x;
    unsigned i = 0, id = 0;
    bool first = true;
    while (i < 4) {
        if (!mb_byte(d, &x)) return false;
        if (x == sync[i]) {
            first = true;
            i++;
            id = 0;
            continue;
        }
        if (x == id3[id]) {
            id++;
            i = 0;
            if (id == 3 && !skip_id3v2(d)) return false;
            continue;
        }
        id = 0;
        if (x == 0xff) {
            d->header_warmup[0] = (uint8_t)x;
            if (!mb_read(d, &x, 8)) return false;
            if (x == 0xff) {
                d->lookahead = (uint8_t)x;
                d->cached = true;
            } else if (x >> 2 == 0x3e) {
                d->header_warmup[1] = (uint8_t)x;
                d->pos = d->bitpos_meta / 8;
                d->state = FLAC__STREAM_DECODER_READ_FRAME;
                return true;
            }
        }
        i = 0;
        if (first) {
            send_error(d, FLAC__STREAM_DECODER_ERROR_STATUS_LOST_SYNC);
            first = false;
        }
    }
    d->state = FLAC__STREAM_DECODER_READ_METADATA;
    return true;
}

/* read_metadata_ (STREAMINFO reported; every other block skipped, as libFLAC's default
 * metadata_respond set does) */
bool read_metadata(Dec *d) {
    uint32_t last, type, length;
    if (!mb_read(d, &last, 1) || !mb_read(d, &type, 7) || !mb_read(d, &length, 24)) return false;
    if (type == FLAC__METADATA_TYPE_STREAMINFO) {
        FLAC__StreamMetadata &m = d->stream_info;
        FLAC__StreamMetadata_StreamInfo &si = m.data.stream_info;
        uint32_t v, hi, lo;
        memset(&m, 0, sizeof m);
        m.type = FLAC__METADATA_TYPE_STREAMINFO;
        m.is_last = last ? 1 : 0;
        m.length = length;
        if (!mb_read(d, &v, 16)) return false;
        si.min_blocksize = v;
        if (!mb_read(d, &v, 16)) return false;
        si.max_blocksize = v;
        if (!mb_read(d, &v, 24)) return false;
        si.min_framesize = v;
        if (!mb_read(d, &v, 24)) return false;
        si.max_framesize = v;
        if (!mb_read(d, &v, 20)) return false;
        si.sample_rate = v;
        if (!mb_read(d, &v, 3)) return false;
        si.channels = v + 1;
        if (!mb_read(d, &v, 5)) return false;
        si.bits_per_sample = v + 1;
        if (!mb_read(d, &hi, 4) || !mb_read(d, &lo, 32)) return false;
        si.total_samples = ((uint64_t)hi << 32) | lo;
        for (int i = 0; i < 16; i++) {
            if (!mb_read(d, &v, 8)) return false;
            si.md5sum[i] = (uint8_t)v;
        }
        uint64_t end = d->bitpos_meta + (uint64_t)(uint32_t)(length - 34u) * 8;
        if (!need_bytes(d, end / 8)) return false;
        d->bitpos_meta = end;
        d->has_stream_info = true;
        /* an all-zero md5sum means "not computed": nothing to check against */
        bool zero = true;
        for (int i = 0; i < 16; i++) zero = zero && si.md5sum[i] == 0;
        if (zero) d->do_md5 = false;
        if (d->metadata_cb && !d->is_seeking) d->metadata_cb(d, &m, d->client);
    } else if (type == FLAC__METADATA_TYPE_SEEKTABLE) {
        /* read_metadata_seektable_: length / 18 points of (sample 64, offset 64, samples 16),
         * kept whatever the respond set (libFLAC's seek uses them; no callback here, as the
         * reference leaves metadata_respond at its STREAMINFO-only default) */
        const uint64_t end = d->bitpos_meta + (uint64_t)length * 8;
        d->seek_table.clear();
        for (uint32_t i = 0; i < length / 18u; i++) {
            uint32_t a, b, c, e, f;
            if (!mb_read(d, &a, 32) || !mb_read(d, &b, 32) || !mb_read(d, &c, 32) || !mb_read(d, &e, 32) ||
                !mb_read(d, &f, 16))
                return false;
            const uint64_t sample = ((uint64_t)a << 32) | b;
            if (sample == ~0ull) continue; /* FLAC__STREAM_METADATA_SEEKPOINT_PLACEHOLDER */
            d->seek_table.push_back({sample, ((uint64_t)c << 32) | e, f});
        }
        if (!need_bytes(d, end / 8)) return false;
        d->bitpos_meta = end;
    } else {
        uint64_t end = d->bitpos_meta + (uint64_t)length * 8;
        if (!need_bytes(d, end / 8)) return false;
        d->bitpos_meta = end;
    }
    if (last) {
        d->pos = d->bitpos_meta / 8;
        d->first_frame_offset = d->pos;
        d->state = FLAC__STREAM_DECODER_SEARCH_FOR_FRAME_SYNC;
    }
    return true;
}

bool byte_at(Dec *d, uint64_t p, uint32_t *x) {
    if (!need_bytes(d, p + 1)) return false;
    *x = bat(d, p);
    return true;
}

/* Drop consumed bytes once they pile up: everything below `keep` (the frame being decoded)
 * is no longer needed -- decoded windows live on the GPU and in info/pcm, and a seek
 * refills through the client's seek callback. */
void trim_consumed(Dec *d, uint64_t keep) {
    if (keep <= d->buf_base) return;
    const uint64_t drop = std::min<uint64_t>(keep - d->buf_base, d->buf.size());
    if (drop < (16ull << 20) || drop * 2 < d->buf.size()) return;
    d->buf.erase(d->buf.begin(), d->buf.begin() + (ptrdiff_t)drop);
    d->buf_base += drop;
}

/* frame_sync_ (@0x10011760) over the host buffer */
bool frame_sync(Dec *d) {
    bool first = true;
    uint64_t total = d->has_stream_info ? d->stream_info.data.stream_info.total_samples : 0;
    if (total > 0 && d->samples_decoded >= total) {
        d->state = FLAC__STREAM_DECODER_END_OF_STREAM;
        return true;
    }
    for (;;) {
        uint32_t x;
        if (d->cached) {
            x = d->lookahead;
            d->cached = false;
        } else {
            if (!byte_at(d, d->pos, &x)) return false;
            d->pos++;
        }
        if (x == 0xff) {
            d->header_warmup[0] = (uint8_t)x;
            if (!byte_at(d, d->pos, &x)) return false;
            d->pos++;
            if (x == 0xff) {
                d->lookahead = (uint8_t)x;
                d->cached = true;
            } else if (x >> 2 == 0x3e) {
                d->header_warmup[1] = (uint8_t)x;
                d->state = FLAC__STREAM_DECODER_READ_FRAME;
                return true;
            }
        }
        if (first) {
            send_error(d, FLAC__STREAM_DECODER_ERROR_STATUS_LOST_SYNC);
            first = false;
        }
    }
}

bool gpu_init(Dec *d) {
    if (d->gpu_ready) return true;
    const char *dev = getenv("BNFLAC_DEVICE");
    int cur = 0;
    if (!dev && hipGetDevice(&cur) != hipSuccess) cur = 0;
    d->device = dev ? atoi(dev) : cur; /* the caller's device (a torchrun rank's), unless overridden */
    if (bnflac_ctx_create(d->device, &d->ctx) != 0) return false;
    DevGuard g(d->device);
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) return fail("bnflac: stream create failed") == 0;
    d->gpu_ready = true;
    return true;
}

void gpu_free(Dec *d) {
    if (!d->gpu_ready) return;
    DevGuard g(d->device);
    d->d_bytes.release();
    d->d_cand.release();
    d->d_count.release();
    d->d_info.release();
    d->d_pcm.release();
    if (d->stream) (void)hipStreamDestroy(d->stream);
    d->stream = nullptr;
    bnflac_ctx_destroy(d->ctx);
    d->ctx = nullptr;
    d->gpu_ready = false;
}

/* Decode every candidate frame in buf[base, buf.size()) on the GPU. */
bool decode_window(Dec *d, uint64_t base) {
    if (!gpu_init(d)) {
        d->state = FLAC__STREAM_DECODER_MEMORY_ALLOCATION_ERROR;
        return false;
    }
    DevGuard g(d->device);
    const uint64_t n = bend(d) - base;
    const size_t padded = (size_t)((n + 3) & ~3ull) + 16;
    if (!d->d_bytes.grow(padded)) goto oom;
    if (hipMemsetAsync((uint8_t *)d->d_bytes.p + (n & ~3ull), 0, padded - (n & ~3ull), d->stream) != hipSuccess) goto hip_fail;
    if (hipMemcpyAsync(d->d_bytes.p, d->buf.data() + (base - d->buf_base), n, hipMemcpyHostToDevice, d->stream) != hipSuccess) goto hip_fail;
    {
        uint32_t cap = (uint32_t)std::min<uint64_t>(n / 2 + 16, 1u << 30);
        cap = std::min<uint32_t>(cap, (uint32_t)(n / 64 + 4096));
        for (int attempt = 0; attempt < 2; attempt++) {
            if (!d->d_cand.grow(sizeof(uint64_t) * cap) || !d->d_count.grow(16)) goto oom;
            if (bnflac_index_frames(d->ctx, (const uint8_t *)d->d_bytes.p, n, (uint64_t *)d->d_cand.p, cap,
                                    (uint32_t *)d->d_count.p, d->stream) != 0)
                goto hip_fail;
            uint32_t cnt = 0;
            if (hipMemcpyAsync(&cnt, d->d_count.p, 4, hipMemcpyDeviceToHost, d->stream) != hipSuccess) goto hip_fail;
            if (hipStreamSynchronize(d->stream) != hipSuccess) goto hip_fail;
            if (cnt <= cap) {
                cap = cnt;
                break;
            }
            cap = cnt;
        }
        const uint32_t ncand = cap;
        d->cand.resize(ncand);
        d->info.resize(ncand);
        if (ncand) {
            if (hipMemcpyAsync(d->cand.data(), d->d_cand.p, sizeof(uint64_t) * ncand, hipMemcpyDeviceToHost, d->stream) != hipSuccess)
                goto hip_fail;
            bnf_stream_params sp;
            memset(&sp, 0, sizeof sp);
            if (d->has_stream_info) {
                const FLAC__StreamMetadata_StreamInfo &si = d->stream_info.data.stream_info;
                sp.has_stream_info = 1;
                sp.min_blocksize = si.min_blocksize;
                sp.max_blocksize = si.max_blocksize;
                sp.sample_rate = si.sample_rate;
                sp.channels = si.channels;
                sp.bps = si.bits_per_sample;
                sp.total_samples = si.total_samples;
            }
            if (!d->d_info.grow(sizeof(bnf_frame_info) * ncand)) goto oom;
            if (bnf_launch_parse((const uint32_t *)d->d_bytes.p, n, (const uint64_t *)d->d_cand.p, ncand, sp,
                                 nullptr, 0, (bnf_frame_info *)d->d_info.p, nullptr, nullptr, nullptr, d->stream) != hipSuccess)
                goto hip_fail;
            if (hipMemcpyAsync(d->info.data(), d->d_info.p, sizeof(bnf_frame_info) * ncand, hipMemcpyDeviceToHost, d->stream) != hipSuccess)
                goto hip_fail;
            if (hipStreamSynchronize(d->stream) != hipSuccess) goto hip_fail;
            uint64_t tot = 0;
            uint32_t pcm_ch = 1; /* planar slots per sample: the window's widest frame */
            for (auto &fi : d->info) {
                fi.out_sample = tot;
                if (fi.status == BNF_ST_OK) {
                    tot += fi.blocksize;
                    pcm_ch = std::max(pcm_ch, std::min<uint32_t>(fi.channels, 8u));
                }
            }
            d->pcm_ch = pcm_ch;
            if (!d->d_pcm.grow(sizeof(int32_t) * (size_t)std::max<uint64_t>(tot, 1) * pcm_ch)) goto oom;
            if (hipMemcpyAsync(d->d_info.p, d->info.data(), sizeof(bnf_frame_info) * ncand, hipMemcpyHostToDevice, d->stream) != hipSuccess)
                goto hip_fail;
            bnf_stream_params spd = sp;
            spd.channels = pcm_ch;
            if (bnf_launch_decode((const uint32_t *)d->d_bytes.p, n, ncand, spd, lanes_for(pcm_ch), BNF_OUT_PLANAR32,
                                  (uint8_t *)d->d_pcm.p, (uint64_t)std::max<uint64_t>(tot, 1) * pcm_ch * 4,
                                  (bnf_frame_info *)d->d_info.p, nullptr, nullptr, d->stream) != hipSuccess)
                goto hip_fail;
            d->pcm.resize((size_t)tot * pcm_ch);
            if (tot && hipMemcpyAsync(d->pcm.data(), d->d_pcm.p, sizeof(int32_t) * (size_t)tot * pcm_ch, hipMemcpyDeviceToHost, d->stream) != hipSuccess)
                goto hip_fail;
            if (hipMemcpyAsync(d->info.data(), d->d_info.p, sizeof(bnf_frame_info) * ncand, hipMemcpyDeviceToHost, d->stream) != hipSuccess)
                goto hip_fail;
            if (hipStreamSynchronize(d->stream) != hipSuccess) goto hip_fail;
        }
    }
    d->win_base = base;
    d->win_end = bend(d);
    d->win_valid = true;
    d->read_ahead_cur = std::min(d->read_ahead, d->read_ahead_cur * 2);
    return true;
oom:
    fail("bnflac: out of device memory");
    d->state = FLAC__STREAM_DECODER_MEMORY_ALLOCATION_ERROR;
    return false;
hip_fail:
    fail(std::string("bnflac: HIP error in decode window: ") + hipGetErrorString(hipGetLastError()));
    d->state = FLAC__STREAM_DECODER_MEMORY_ALLOCATION_ERROR;
    return false;
}

const bnf_frame_info *lookup(Dec *d, uint64_t p) {
    if (!d->win_valid || p < d->win_base || p >= d->win_end) return nullptr;
    uint64_t rel = p - d->win_base;
    auto it = std::lower_bound(d->cand.begin(), d->cand.end(), rel);
    if (it == d->cand.end() || *it != rel) return nullptr;
    return &d->info[(size_t)(it - d->cand.begin())];
}

void allocate_output(Dec *d, unsigned size, unsigned ch) {
    if (size <= d->output_capacity && ch <= d->output_channels) return;
    for (unsigned i = 0; i < FLAC__MAX_CHANNELS; i++) d->output[i].clear();
    /* twice the capacity: a client that copies more than the frame (FLACFileReader copies
     * the first frame's blocksize from a trimmed seek frame, FLACFileReader.cs:287) reads
     * stale values instead of running off the allocation */
    for (unsigned i = 0; i < ch; i++) d->output[i].assign(2u * (size ? size : 1), 0);
    d->output_capacity = size;
    d->output_channels = ch;
}

/* read_frame_ (@0x100118c0) replay for the frame whose sync starts at d->pos - 2 */
bool read_frame(Dec *d, bool *got) {
    *got = false;
    const uint64_t p = d->pos - 2;
    const bnf_frame_info *fi = nullptr;
    for (int tries = 0;; tries++) {
        fi = lookup(d, p);
        if (fi && fi->status != BNF_ST_TRUNC) break;
        if (tries > 200) {
            fail("bnflac: frame window did not converge");
            d->state = FLAC__STREAM_DECODER_ABORTED;
            return false;
        }
        if (d->client_done) {
            /* no more bytes will come: a truncated frame makes libFLAC's reader fail here */
            if ((fi && fi->status == BNF_ST_TRUNC) ||
                (d->win_valid && d->win_base == p && d->win_end == bend(d))) {
                need_bytes(d, bend(d) + 1);
                return false;
            }
        } else {
            const uint64_t have = bend(d) > p ? bend(d) - p : 0;
            read_ahead(d, p + std::max<uint64_t>(d->read_ahead_cur, 2 * have + 4096));
        }
        if (!decode_window(d, p)) return false;
    }
    if (!fi) {
        d->state = FLAC__STREAM_DECODER_ABORTED;
        return false;
    }
    if (fi->status == BNF_ST_SKIPPED) {
        fail("bnflac: frame not decodable with the configured lanes");
        d->state = FLAC__STREAM_DECODER_ABORTED;
        return false;
    }
    const uint64_t abs_resume = d->win_base * 8 + fi->resume_bit;
    if (fi->status == BNF_ST_ERROR) {
        send_error(d, (FLAC__StreamDecoderErrorStatus)fi->err);
        d->state = FLAC__STREAM_DECODER_SEARCH_FOR_FRAME_SYNC;
        d->pos = (abs_resume + 7) / 8;
        if (fi->cached >= 0) {
            d->cached = true;
            d->lookahead = (uint8_t)fi->cached;
        }
        return true;
    }
    /* header -> FLAC__Frame, frame/sample number conversion (@0x1001231f-0x100123ca) */
    FLAC__FrameHeader &h = d->frame.header;
    memset(&d->frame, 0, sizeof d->frame);
    h.blocksize = fi->blocksize;
    h.sample_rate = fi->sample_rate;
    h.channels = fi->channels;
    h.channel_assignment = (FLAC__ChannelAssignment)fi->assignment;
    h.bits_per_sample = fi->bps;
    h.crc = (FLAC__uint8)fi->crc8;
    d->next_fixed_block_size = 0;
    bool unparseable = false;
    if (fi->number_type == 0) {
        const uint32_t fn = (uint32_t)fi->number;
        h.number_type = FLAC__FRAME_NUMBER_TYPE_SAMPLE_NUMBER;
        if (d->fixed_block_size) {
            h.number.sample_number = (uint64_t)d->fixed_block_size * fn;
        } else if (d->has_stream_info) {
            const FLAC__StreamMetadata_StreamInfo &si = d->stream_info.data.stream_info;
            if (si.min_blocksize == si.max_blocksize) {
                h.number.sample_number = (uint64_t)si.min_blocksize * fn;
                d->next_fixed_block_size = si.max_blocksize;
            } else {
                unparseable = true;
            }
        } else if (fn == 0) {
            h.number.sample_number = 0;
            d->next_fixed_block_size = h.blocksize;
        } else {
            h.number.sample_number = (uint64_t)h.blocksize * fn;
        }
    } else {
        h.number_type = FLAC__FRAME_NUMBER_TYPE_SAMPLE_NUMBER;
        h.number.sample_number = fi->number;
    }
    if (unparseable) {
        send_error(d, FLAC__STREAM_DECODER_ERROR_STATUS_UNPARSEABLE_STREAM);
        d->state = FLAC__STREAM_DECODER_SEARCH_FOR_FRAME_SYNC;
        /* libFLAC stops right after the header's CRC-8 byte */
        d->pos = fi->frame_off + d->win_base + 2; /* conservative: resync just past the sync */
        return true;
    }
    d->frame.footer.crc = (FLAC__uint16)fi->crc16_read;
    allocate_output(d, h.blocksize, h.channels);
    const int32_t *src = d->pcm.data() + (size_t)fi->out_sample * d->pcm_ch;
    for (unsigned c = 0; c < h.channels; c++)
        memcpy(d->output[c].data(), src + (size_t)c * h.blocksize, sizeof(int32_t) * h.blocksize);
    if (!fi->crc_ok) send_error(d, FLAC__STREAM_DECODER_ERROR_STATUS_FRAME_CRC_MISMATCH); /* output already zeroed */
    *got = true;
    if (d->next_fixed_block_size) d->fixed_block_size = d->next_fixed_block_size;
    d->channels = h.channels;
    d->channel_assignment = h.channel_assignment;
    d->bits_per_sample = h.bits_per_sample;
    d->sample_rate = h.sample_rate;
    d->blocksize = h.blocksize;
    d->samples_decoded = h.number.sample_number + h.blocksize;
    d->pos = abs_resume / 8;
    trim_consumed(d, p);
    const FLAC__int32 *bufs[FLAC__MAX_CHANNELS];
    for (unsigned c = 0; c < FLAC__MAX_CHANNELS; c++) bufs[c] = c < d->output_channels ? d->output[c].data() : nullptr;
    if (d->is_seeking) {
        /* write_audio_frame_to_client_ while seeking: deliver only the frame holding the
         * target sample, trimmed so it starts there */
        const uint64_t sn = h.number.sample_number;
        if (d->seek_target >= sn && d->seek_target < sn + h.blocksize) {
            const unsigned delta = (unsigned)(d->seek_target - sn);
            FLAC__Frame fr = d->frame;
            fr.header.blocksize -= delta;
            fr.header.number.sample_number += delta;
            const FLAC__int32 *nb[FLAC__MAX_CHANNELS];
            for (unsigned c = 0; c < FLAC__MAX_CHANNELS; c++) nb[c] = bufs[c] ? bufs[c] + delta : nullptr;
            d->is_seeking = false;
            /* the callback runs in READ_FRAME, as libFLAC's; it may itself seek again */
            FLAC__StreamDecoderWriteStatus ws = d->write_cb(d, &fr, nb, d->client);
            if (ws != FLAC__STREAM_DECODER_WRITE_STATUS_CONTINUE && !d->ignore_write_status) {
                d->seek_done = -1;
                return false; /* state stays READ_FRAME */
            }
            d->seek_done = 1;
            d->state = FLAC__STREAM_DECODER_SEARCH_FOR_FRAME_SYNC;
            return true;
        }
        d->state = FLAC__STREAM_DECODER_SEARCH_FOR_FRAME_SYNC;
        return true;
    }
    /* write_audio_frame_to_client_: no STREAMINFO -> no sum to compare, stop hashing */
    if (!d->has_stream_info) d->do_md5 = false;
    if (d->do_md5) md5_accumulate(d->md5, bufs, h.channels, h.blocksize, 1, (h.bits_per_sample + 7) / 8);
    FLAC__StreamDecoderWriteStatus ws = d->write_cb(d, &d->frame, bufs, d->client);
    if (ws != FLAC__STREAM_DECODER_WRITE_STATUS_CONTINUE && !d->ignore_write_status) return false; /* state stays READ_FRAME */
    d->state = FLAC__STREAM_DECODER_SEARCH_FOR_FRAME_SYNC;
    return true;
}

void reset_fields(Dec *d) {
    d->buf.clear();
    d->buf_base = 0;
    d->pos = 0;
    d->bitpos_meta = 0;
    d->cached = false;
    d->client_done = 0;
    d->has_stream_info = false;
    d->seek_table.clear();
    d->samples_decoded = 0;
    d->fixed_block_size = d->next_fixed_block_size = 0;
    d->first_frame_offset = 0;
    d->win_valid = false;
    d->cand.clear();
    d->info.clear();
    d->pcm.clear();
    d->is_seeking = false;
    d->do_md5 = d->md5_checking;
    d->read_ahead_cur = std::min<uint64_t>(d->read_ahead, 256ull << 10);
    md5_init(d->md5);
}

/* Sample number of a decoded window frame (the header number conversion of read_frame). */
uint64_t frame_first_sample(const Dec *d, const bnf_frame_info &fi) {
    if (fi.number_type == 1) return fi.number;
    if (d->fixed_block_size) return (uint64_t)d->fixed_block_size * fi.number;
    if (d->has_stream_info) {
        const FLAC__StreamMetadata_StreamInfo &si = d->stream_info.data.stream_info;
        if (si.min_blocksize == si.max_blocksize) return (uint64_t)si.min_blocksize * fi.number;
    }
    return (uint64_t)fi.blocksize * fi.number;
}

/* Frame of the decoded window that holds `target` (intact frames only: header, CRC-16).
 * Returns 1 found (*off = its absolute offset), 0 the window's frames all lie before it
 * (lo_off/lo_s = the last one), -1 they all lie after it (hi_off/hi_s = the first one),
 * -2 the window has no intact frame. */
int window_find(const Dec *d, uint64_t target, uint64_t *off, uint64_t *lo_off, uint64_t *lo_s, uint64_t *hi_off,
                uint64_t *hi_s) {
    bool any = false;
    uint64_t f_off = 0, f_s = 0, l_off = 0, l_s = 0;
    for (size_t i = 0; i < d->info.size(); i++) {
        const bnf_frame_info &fi = d->info[i];
        if (fi.status != BNF_ST_OK || !fi.crc_ok) continue;
        const uint64_t sn = frame_first_sample(d, fi), o = d->win_base + d->cand[i];
        if (sn <= target && target < sn + fi.blocksize) {
            *off = o;
            return 1;
        }
        if (!any) { f_off = o; f_s = sn; }
        l_off = o;
        l_s = sn + fi.blocksize;
        any = true;
    }
    if (!any) return -2;
    if (target < f_s) { *hi_off = f_off; *hi_s = f_s; return -1; }
    *lo_off = l_off;
    *lo_s = l_s;
    return 0;
}

/* Reposition the client at `at` and decode one window from there. */
bool window_at(Dec *d, uint64_t at, uint64_t bytes) {
    if (d->seek_cb(d, at, d->client) != FLAC__STREAM_DECODER_SEEK_STATUS_OK) return false;
    d->buf.clear();
    d->buf_base = at;
    d->client_done = 0;
    d->win_valid = false;
    d->cached = false;
    read_ahead(d, at + bytes);
    if (bend(d) <= at) return false;
    return decode_window(d, at);
}

/* Byte offset of the frame holding `target`: the current window when it is there and its
 * bytes are still buffered; otherwise an interpolation search between known (offset,
 * sample) points, each probe one client seek + one GPU window (O(window) per probe,
 * O(log) probes), like libFLAC's seek_to_absolute_sample_ but over decoded windows. */
bool seek_search(Dec *d, uint64_t target, uint64_t length, uint64_t *start, bool use_table);

bool seek_position(Dec *d, uint64_t target, uint64_t length, uint64_t *start) {
    uint64_t off = 0, lo_off = d->first_frame_offset, lo_s = 0, hi_off = length, hi_s = 0;
    if (d->win_valid && window_find(d, target, &off, &lo_off, &lo_s, &hi_off, &hi_s) == 1 && off >= d->buf_base) {
        *start = off;
        return true;
    }
    /* a SEEKTABLE only narrows the search; one that misleads it (offsets past the stream,
     * points out of order) costs a second, table-free search, never different output */
    if (!d->seek_table.empty() && seek_search(d, target, length, start, true)) return true;
    return seek_search(d, target, length, start, false);
}

/* seek_to_absolute_sample_ over decoded windows; use_table: bracket the target between the
 * SEEKTABLE points around it (libFLAC's lower/upper bound from the table) */
bool seek_search(Dec *d, uint64_t target, uint64_t length, uint64_t *start, bool use_table) {
    uint64_t off = 0, lo_off, lo_s, hi_off, hi_s;
    const FLAC__uint64 total = FLAC__stream_decoder_get_total_samples(d);
    lo_off = d->first_frame_offset;
    lo_s = 0;
    hi_off = length;
    hi_s = total ? total : ~0ull;
    if (use_table) {
        for (const auto &p : d->seek_table) {
            if (p.frame_samples == 0 || (total && p.sample >= total)) continue;
            const uint64_t o = d->first_frame_offset + p.offset;
            if (p.offset > length || o >= length) continue;
            if (p.sample <= target && p.sample >= lo_s && o >= lo_off) {
                lo_s = p.sample;
                lo_off = o;
            } else if (p.sample > target && p.sample < hi_s && o < hi_off) {
                hi_s = p.sample;
                hi_off = o;
            }
        }
        if (hi_off <= lo_off) return false;
    }
    const uint32_t maxfs = d->has_stream_info ? d->stream_info.data.stream_info.max_framesize : 0;
    const uint64_t win = std::max<uint64_t>(1ull << 20, 4ull * (maxfs ? maxfs : 65536));
    for (int probe = 0; probe < 64; probe++) {
        if (hi_off <= lo_off) return false;
        uint64_t est = lo_off;
        if (hi_s != ~0ull && hi_s > lo_s && target > lo_s)
            est = lo_off + (uint64_t)((double)(target - lo_s) / (double)(hi_s - lo_s) * (double)(hi_off - lo_off));
        est = (est > lo_off + win / 2) ? est - win / 2 : lo_off; /* aim the window's middle at the target */
        if (!window_at(d, est, win)) return false;
        const int r = window_find(d, target, &off, &lo_off, &lo_s, &hi_off, &hi_s);
        if (r == 1) {
            *start = off;
            return true;
        }
        if (r == -2) { /* nothing intact here: shrink the range from above */
            if (est == lo_off) return false;
            hi_off = est;
        } else if (r == -1 && est <= lo_off) {
            return false; /* the first frame at/after the range start is already past the target */
        }
    }
    return false;
}

/* file callbacks (stream_decoder.c file_*_callback_) */
FLAC__StreamDecoderReadStatus file_read(const FLAC__StreamDecoder *dec, FLAC__byte buffer[], size_t *bytes, void *) {
    FILE *f = dec->file;
    if (*bytes > 0) {
        *bytes = fread(buffer, 1, *bytes, f);
        if (ferror(f)) return FLAC__STREAM_DECODER_READ_STATUS_ABORT;
        if (*bytes == 0) return FLAC__STREAM_DECODER_READ_STATUS_END_OF_STREAM;
        return FLAC__STREAM_DECODER_READ_STATUS_CONTINUE;
    }
    return FLAC__STREAM_DECODER_READ_STATUS_ABORT;
}
FLAC__StreamDecoderSeekStatus file_seek(const FLAC__StreamDecoder *dec, FLAC__uint64 off, void *) {
    return fseeko(dec->file, (off_t)off, SEEK_SET) < 0 ? FLAC__STREAM_DECODER_SEEK_STATUS_ERROR : FLAC__STREAM_DECODER_SEEK_STATUS_OK;
}
FLAC__StreamDecoderTellStatus file_tell(const FLAC__StreamDecoder *dec, FLAC__uint64 *off, void *) {
    off_t p = ftello(dec->file);
    if (p < 0) return FLAC__STREAM_DECODER_TELL_STATUS_ERROR;
    *off = (FLAC__uint64)p;
    return FLAC__STREAM_DECODER_TELL_STATUS_OK;
}
FLAC__StreamDecoderLengthStatus file_length(const FLAC__StreamDecoder *dec, FLAC__uint64 *len, void *) {
    struct stat st;
    if (fstat(fileno(dec->file), &st) != 0) return FLAC__STREAM_DECODER_LENGTH_STATUS_ERROR;
    *len = (FLAC__uint64)st.st_size;
    return FLAC__STREAM_DECODER_LENGTH_STATUS_OK;
}
FLAC__bool file_eof(const FLAC__StreamDecoder *dec, void *) { return feof(dec->file) ? 1 : 0; }

} // namespace

/* ---------------------------------------------------------------- exports */
extern "C" {

BNFLAC_API FLAC__StreamDecoder *FLAC__stream_decoder_new(void) {
    Dec *d = new (std::nothrow) Dec();
    if (!d) return nullptr;
    memset(&d->stream_info, 0, sizeof d->stream_info);
    memset(&d->frame, 0, sizeof d->frame);
    const char *ra = getenv("BNFLAC_READ_AHEAD_MB");
    if (ra) d->read_ahead = (uint64_t)std::max(1, atoi(ra)) << 20;
    return d;
}

static int init_common(Dec *d) {
    reset_fields(d);
    if (!gpu_init(d)) return FLAC__STREAM_DECODER_INIT_STATUS_MEMORY_ALLOCATION_ERROR;
    d->state = FLAC__STREAM_DECODER_SEARCH_FOR_METADATA;
    return FLAC__STREAM_DECODER_INIT_STATUS_OK;
}

BNFLAC_API int FLAC__stream_decoder_init_stream(FLAC__StreamDecoder *d, FLAC__StreamDecoderReadCallback read,
                                                FLAC__StreamDecoderSeekCallback seek, FLAC__StreamDecoderTellCallback tell,
                                                FLAC__StreamDecoderLengthCallback length, FLAC__StreamDecoderEofCallback eof,
                                                FLAC__StreamDecoderWriteCallback write,
                                                FLAC__StreamDecoderMetadataCallback metadata,
                                                FLAC__StreamDecoderErrorCallback error, void *client) {
    if (!d) return FLAC__STREAM_DECODER_INIT_STATUS_MEMORY_ALLOCATION_ERROR;
    if (d->state != FLAC__STREAM_DECODER_UNINITIALIZED) return FLAC__STREAM_DECODER_INIT_STATUS_ALREADY_INITIALIZED;
    if (!read || !write || !error || (seek && (!tell || !length || !eof)))
        return FLAC__STREAM_DECODER_INIT_STATUS_INVALID_CALLBACKS;
    d->read_cb = read; d->seek_cb = seek; d->tell_cb = tell; d->length_cb = length; d->eof_cb = eof;
    d->write_cb = write; d->metadata_cb = metadata; d->error_cb = error; d->client = client;
    d->ignore_write_status = false;
    return init_common(d);
}

BNFLAC_API int FLAC__stream_decoder_init_file(FLAC__StreamDecoder *d, const char *filename,
                                              FLAC__StreamDecoderWriteCallback write,
                                              FLAC__StreamDecoderMetadataCallback metadata,
                                              FLAC__StreamDecoderErrorCallback error, void *client) {
    if (!d) return FLAC__STREAM_DECODER_INIT_STATUS_MEMORY_ALLOCATION_ERROR;
    if (d->state != FLAC__STREAM_DECODER_UNINITIALIZED) return FLAC__STREAM_DECODER_INIT_STATUS_ALREADY_INITIALIZED;
    if (!write || !error) return FLAC__STREAM_DECODER_INIT_STATUS_INVALID_CALLBACKS;
    FILE *f = filename ? fopen(filename, "rb") : stdin;
    if (!f) return FLAC__STREAM_DECODER_INIT_STATUS_ERROR_OPENING_FILE;
    d->file = f;
    d->read_cb = file_read; d->seek_cb = file_seek; d->tell_cb = file_tell; d->length_cb = file_length; d->eof_cb = file_eof;
    d->write_cb = write; d->metadata_cb = metadata; d->error_cb = error; d->client = client;
    /* LibFLACSharp.cs:205-206 declares this write callback void: its return register is
     * garbage, so it is treated as CONTINUE (BNFLAC_STRICT_WRITE_STATUS=1 honours it). */
    const char *strict = getenv("BNFLAC_STRICT_WRITE_STATUS");
    d->ignore_write_status = !(strict && atoi(strict));
    int rc = init_common(d);
    if (rc != FLAC__STREAM_DECODER_INIT_STATUS_OK) {
        fclose(f);
        d->file = nullptr;
    }
    return rc;
}

BNFLAC_API FLAC__bool FLAC__stream_decoder_finish(FLAC__StreamDecoder *d) {
    if (!d) return 0;
    if (d->state == FLAC__STREAM_DECODER_UNINITIALIZED) return 1;
    if (d->file && d->file != stdin) fclose(d->file);
    d->file = nullptr;
    bool md5_failed = false;
    if (d->do_md5) {
        uint8_t sum[16];
        md5_final(d->md5, sum);
        md5_failed = memcmp(sum, d->stream_info.data.stream_info.md5sum, 16) != 0;
    }
    reset_fields(d);
    for (unsigned i = 0; i < FLAC__MAX_CHANNELS; i++) d->output[i].clear();
    d->output_capacity = d->output_channels = 0;
    d->md5_checking = false; /* set_defaults_ */
    d->state = FLAC__STREAM_DECODER_UNINITIALIZED;
    return md5_failed ? 0 : 1;
}

BNFLAC_API FLAC__bool FLAC__stream_decoder_set_md5_checking(FLAC__StreamDecoder *d, FLAC__bool value) {
    if (!d || d->state != FLAC__STREAM_DECODER_UNINITIALIZED) return 0;
    d->md5_checking = value != 0;
    return 1;
}

BNFLAC_API FLAC__bool FLAC__stream_decoder_get_md5_checking(const FLAC__StreamDecoder *d) {
    return (d && d->md5_checking) ? 1 : 0;
}

BNFLAC_API FLAC__bool FLAC__stream_decoder_delete(FLAC__StreamDecoder *d) {
    if (!d) return 1;
    FLAC__stream_decoder_finish(d);
    gpu_free(d);
    delete d;
    return 1;
}

BNFLAC_API FLAC__bool FLAC__stream_decoder_process_single(FLAC__StreamDecoder *d) {
    if (!d) return 0;
    bool got;
    for (;;) {
        switch (d->state) {
        case FLAC__STREAM_DECODER_SEARCH_FOR_METADATA:
            if (!find_metadata(d)) return 0;
            break;
        case FLAC__STREAM_DECODER_READ_METADATA:
            return read_metadata(d) ? 1 : 0;
        case FLAC__STREAM_DECODER_SEARCH_FOR_FRAME_SYNC:
            if (!frame_sync(d)) return 1;
            break;
        case FLAC__STREAM_DECODER_READ_FRAME:
            if (!read_frame(d, &got)) return 0;
            if (got) return 1;
            break;
        case FLAC__STREAM_DECODER_END_OF_STREAM:
        case FLAC__STREAM_DECODER_ABORTED:
            return 1;
        default:
            return 0;
        }
    }
}

BNFLAC_API FLAC__bool FLAC__stream_decoder_process_until_end_of_metadata(FLAC__StreamDecoder *d) {
    if (!d) return 0;
    for (;;) {
        switch (d->state) {
        case FLAC__STREAM_DECODER_SEARCH_FOR_METADATA:
            if (!find_metadata(d)) return 0;
            break;
        case FLAC__STREAM_DECODER_READ_METADATA:
            if (!read_metadata(d)) return 0;
            break;
        case FLAC__STREAM_DECODER_SEARCH_FOR_FRAME_SYNC:
        case FLAC__STREAM_DECODER_READ_FRAME:
        case FLAC__STREAM_DECODER_END_OF_STREAM:
        case FLAC__STREAM_DECODER_ABORTED:
            return 1;
        default:
            return 0;
        }
    }
}

BNFLAC_API FLAC__bool FLAC__stream_decoder_process_until_end_of_stream(FLAC__StreamDecoder *d) {
    if (!d) return 0;
    bool got;
    for (;;) {
        switch (d->state) {
        case FLAC__STREAM_DECODER_SEARCH_FOR_METADATA:
            if (!find_metadata(d)) return 0;
            break;
        case FLAC__STREAM_DECODER_READ_METADATA:
            if (!read_metadata(d)) return 0;
            break;
        case FLAC__STREAM_DECODER_SEARCH_FOR_FRAME_SYNC:
            if (!frame_sync(d)) return 1;
            break;
        case FLAC__STREAM_DECODER_READ_FRAME:
            if (!read_frame(d, &got)) return 0;
            break;
        case FLAC__STREAM_DECODER_END_OF_STREAM:
        case FLAC__STREAM_DECODER_ABORTED:
            return 1;
        default:
            return 0;
        }
    }
}

BNFLAC_API FLAC__bool FLAC__stream_decoder_seek_absolute(FLAC__StreamDecoder *d, FLAC__uint64 sample) {
    /* stream_decoder.c FLAC__stream_decoder_seek_absolute: states 0-4, a seek callback, the
     * target below STREAMINFO's total; is_seeking and MD5-off come BEFORE the metadata pass
     * (a seek before it suppresses the STREAMINFO callback), then the length callback. */
    if (!d) return 0;
    if (d->state > FLAC__STREAM_DECODER_END_OF_STREAM) return 0;
    if (!d->seek_cb) return 0;
    FLAC__uint64 total = FLAC__stream_decoder_get_total_samples(d);
    if (total > 0 && sample >= total) return 0;
    d->is_seeking = true;
    d->do_md5 = false; /* a seek turns MD5 checking off */
    FLAC__uint64 length = 0;
    if (d->length_cb(d, &length, d->client) != FLAC__STREAM_DECODER_LENGTH_STATUS_OK) {
        d->is_seeking = false;
        return 0;
    }
    if (d->state <= FLAC__STREAM_DECODER_READ_METADATA) {
        if (!FLAC__stream_decoder_process_until_end_of_metadata(d)) {
            d->is_seeking = false;
            return 0;
        }
        total = FLAC__stream_decoder_get_total_samples(d);
        if (total > 0 && sample >= total) {
            d->is_seeking = false;
            return 0;
        }
    }
    /* seek_to_absolute_sample_: find the frame holding `sample` (one decoded window when it
     * is already there, else an interpolation search over client seeks, each step one GPU
     * window), then decode from it: only that frame reaches the write callback, trimmed. */
    uint64_t start = 0;
    if (!seek_position(d, sample, length, &start)) {
        d->is_seeking = false;
        d->state = FLAC__STREAM_DECODER_SEEK_ERROR;
        return 0;
    }
    d->seek_target = sample;
    d->seek_done = 0;
    d->pos = start;
    d->cached = false;
    d->samples_decoded = 0;
    d->state = FLAC__STREAM_DECODER_SEARCH_FOR_FRAME_SYNC;
    bool got;
    for (int guard = 0; guard < 100000000 && !d->seek_done; guard++) {
        if (d->state == FLAC__STREAM_DECODER_SEARCH_FOR_FRAME_SYNC) {
            if (!frame_sync(d)) break;
        } else if (d->state == FLAC__STREAM_DECODER_READ_FRAME) {
            if (!read_frame(d, &got)) break;
        } else {
            break;
        }
    }
    d->is_seeking = false;
    if (d->seek_done == 1) return 1;
    d->state = FLAC__STREAM_DECODER_SEEK_ERROR;
    return 0;
}

BNFLAC_API FLAC__bool FLAC__stream_decoder_get_decode_position(const FLAC__StreamDecoder *d, FLAC__uint64 *position) {
    if (!d || !d->tell_cb) return 0;
    if (d->tell_cb(d, position, d->client) != FLAC__STREAM_DECODER_TELL_STATUS_OK) return 0;
    const uint64_t unconsumed = bend(d) - std::min<uint64_t>(d->pos, bend(d));
    *position -= unconsumed;
    return 1;
}

BNFLAC_API FLAC__uint64 FLAC__stream_decoder_get_total_samples(const FLAC__StreamDecoder *d) {
    return (d && d->has_stream_info) ? d->stream_info.data.stream_info.total_samples : 0;
}
BNFLAC_API unsigned FLAC__stream_decoder_get_channels(const FLAC__StreamDecoder *d) { return d ? d->channels : 0; }
BNFLAC_API unsigned FLAC__stream_decoder_get_bits_per_sample(const FLAC__StreamDecoder *d) { return d ? d->bits_per_sample : 0; }
BNFLAC_API unsigned FLAC__stream_decoder_get_sample_rate(const FLAC__StreamDecoder *d) { return d ? d->sample_rate : 0; }
BNFLAC_API FLAC__StreamDecoderState FLAC__stream_decoder_get_state(const FLAC__StreamDecoder *d) {
    return d ? d->state : FLAC__STREAM_DECODER_UNINITIALIZED;
}

BNFLAC_API FLAC__bool FLAC__stream_decoder_reset(FLAC__StreamDecoder *d) {
    if (!d || d->state == FLAC__STREAM_DECODER_UNINITIALIZED) return 0;
    if (d->file == stdin) return 0;
    if (d->seek_cb && d->seek_cb(d, 0, d->client) == FLAC__STREAM_DECODER_SEEK_STATUS_ERROR) return 0;
    reset_fields(d);
    d->state = FLAC__STREAM_DECODER_SEARCH_FOR_METADATA;
    return 1;
}

} /* extern "C" */
