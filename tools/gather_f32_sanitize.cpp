/*
 * gather_f32_sanitize.cpp -- the host rule of csrc/bnf_pcm_f32.h under AddressSanitizer and UBSan.
 * A stand-alone program: the PCM is a heap allocation of exactly round_up(pcm_bytes, 16) bytes and
 * the output one of exactly (nstreams * planes - 1) * plane_pitch + row_samples floats, so a read
 * or a write outside the contract is a sanitizer report.  Three parts:
 *   1. every layout x pcm_bytes % 16 in {0, 2, 15} x flags x pitch: bnf_gather_f32_host against
 *      the rule written out sample by sample (no tiles, no blocks), bit for bit, windows touching
 *      the last sample frame and bad windows among them;
 *   2. for every tile of every window, exactly the 16-byte block loads the header's block
 *      functions name, each out of the exact allocation;
 *   3. the enumerations the header's comments promise: the frame-of-sample multiply, the stage's
 *      size, and the banks the unpack step's 32-lane groups write.
 * Exit 0: no report, no mismatch.
 *
 *   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I birdnest/audio_amd/csrc tools/gather_f32_sanitize.cpp -o gather_f32_sanitize
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bnf_pcm_f32.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                           \
        }                                                         \
    } while (0)

struct Layout {
    const char *name;
    uint32_t channels, bps, unit;
};
/* FLACDECODER 1/2ch 16; FILEREADER 1/2ch 24, 3ch 16, 8ch 24; INTERLEAVED32 1ch 8, 2ch 16, 3ch 20, 8ch 32 */
static const Layout LAYOUTS[] = {{"fd 1x16", 1, 16, 2}, {"fd 2x16", 2, 16, 2}, {"fr 1x24", 1, 24, 3}, {"fr 2x24", 2, 24, 3},
                                 {"fr 3x16", 3, 16, 2}, {"fr 8x24", 8, 24, 3}, {"i32 1x8", 1, 8, 4},  {"i32 2x16", 2, 16, 4},
                                 {"i32 3x20", 3, 20, 4}, {"i32 8x32", 8, 32, 4}};

static int32_t sample_at(const uint8_t *p, uint32_t unit) { /* byte by byte */
    if (unit == 4) return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
    if (unit == 2) return (int16_t)(uint16_t)(p[0] | p[1] << 8);
    const uint32_t x = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    return (int32_t)(x ^ 0x800000u) - 0x800000;
}

static uint32_t bits(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

static const uint32_t CANARY = 0x7fc5a5a5u; /* a NaN no conversion yields */

static void one_case(const Layout &L, uint32_t tail16, uint32_t flags, uint32_t R, uint64_t pitch) {
    const uint32_t stride = L.unit * L.channels, planes = flags & BNF_F32_MONO ? 1u : L.channels;
    /* whole sample frames, then a partial one so that pcm_bytes % 16 == tail16 where the unit allows it */
    uint64_t nsmp = 3 * (uint64_t)bnf_f32_tile_frames(L.channels) / 2 + 37, pcm_bytes = nsmp * stride;
    while (pcm_bytes % 16 != tail16 && pcm_bytes < nsmp * stride + 64) pcm_bytes++;
    nsmp = pcm_bytes / stride;
    const size_t alloc = (size_t)((pcm_bytes + 15) & ~15ull);
    uint8_t *pcm = (uint8_t *)malloc(alloc);
    for (size_t i = 0; i < alloc; i++) pcm[i] = (uint8_t)rnd();
    std::vector<bnf_window> win;
    auto add = [&](uint64_t first, uint64_t n) {
        bnf_window w;
        memset(&w, 0, sizeof w);
        w.pcm_first = first;
        w.nsamples = n;
        win.push_back(w);
    };
    const uint64_t lens[] = {0, 1, 3, 4, 5, R ? R - 1 : 0, R, (uint64_t)R + 3};
    for (uint64_t n : lens)
        for (uint64_t first = 0; first < 4; first++)
            if (first + n <= nsmp) add(first, n);
    for (uint64_t n : lens)
        if (n && n <= nsmp) add(nsmp - n, n); /* ends at the last whole sample frame */
    add(nsmp, 0);
    add(nsmp - 1, 2);          /* one sample frame past it */
    add(nsmp + 1, 1);
    add(~0ull, 1);
    add(~0ull, 0);             /* empty, wherever it points */
    add(5, ~0ull);
    const uint32_t n = (uint32_t)win.size();
    bnf_window *wheap = (bnf_window *)malloc(sizeof(bnf_window) * n);
    memcpy(wheap, win.data(), sizeof(bnf_window) * n);
    const size_t nout = (size_t)(((uint64_t)n * planes - 1) * pitch + R);
    float *out = (float *)malloc(4 * (nout ? nout : 1));
    for (size_t i = 0; i < nout; i++) memcpy(out + i, &CANARY, 4);
    uint32_t status[4] = {9, 9, 9, 9};
    CHECK(bnf_gather_f32_host(pcm, pcm_bytes, stride, L.unit, L.bps, L.channels, flags, wheap, n, R, pitch, out, status) == 0);
    /* the rule sample by sample */
    const float k = bnf_f32_scale(L.bps);
    const double kd = bnf_f32_scale_d(L.bps);
    uint32_t nbad = 0, ncut = 0;
    std::vector<uint8_t> written(nout ? nout : 1, 0);
    for (uint32_t s = 0; s < n; s++) {
        const uint64_t first = win[s].pcm_first, want = win[s].nsamples;
        const bool bad = want != 0 && (first > nsmp || want > nsmp - first);
        nbad += bad;
        ncut += !bad && want > R;
        const uint64_t ncopy = bad ? 0 : want < R ? want : R;
        for (uint32_t c = 0; c < planes; c++)
            for (uint32_t i = 0; i < R; i++) {
                float f = 0.0f;
                if (i < ncopy) {
                    const uint8_t *fr = pcm + (first + i) * stride;
                    if (flags & BNF_F32_MONO) {
                        int64_t S = 0;
                        for (uint32_t ch = 0; ch < L.channels; ch++) S += sample_at(fr + ch * L.unit, L.unit);
                        f = (float)((double)S * kd / (double)L.channels);
                    } else {
                        f = (float)sample_at(fr + c * L.unit, L.unit) * k;
                    }
                }
                const size_t at = (size_t)(((uint64_t)s * planes + c) * pitch + i);
                written[at] = 1;
                if (bits(out[at]) != bits(f)) {
                    if (failures < 20)
                        fprintf(stderr, "%s flags %u R %u pitch %llu tail %u: window %u plane %u sample %u: %08x, want %08x\n",
                                L.name, flags, R, (unsigned long long)pitch, tail16, s, c, i, bits(out[at]), bits(f));
                    failures++;
                }
            }
    }
    for (size_t i = 0; i < nout; i++)
        if (!written[i]) CHECK(bits(out[i]) == CANARY);
    CHECK(status[0] == (nbad ? 1u : 0u) && status[1] == nbad && status[2] == ncut && status[3] == 0);
    /* 2. the block loads of every tile of every window, as the header names them */
    const uint32_t frames = bnf_f32_tile_frames(L.channels);
    const uint64_t last_blk = bnf_f32_last_block(pcm_bytes);
    uint64_t sum = 0;
    for (uint32_t s = 0; s < n; s++) {
        const bnf_f32_row row = bnf_f32_window(win[s].pcm_first, win[s].nsamples, pcm_bytes, stride, R);
        for (uint64_t t0 = 0; t0 < R; t0 += frames) {
            const bnf_f32_tile t = bnf_f32_tile_of(row, t0, frames, stride, R);
            CHECK(t.nblk <= BNF_F32_RAW_BLOCKS && t.nt <= frames && t.ndata <= t.nt);
            for (uint32_t j = 0; j < t.nblk; j++) {
                uint64_t blk[2];
                const uint64_t a = bnf_f32_block_addr(t, j, last_blk);
                CHECK(a == t.blk0 + 16ull * j); /* the clamp never acts on a checked window */
                memcpy(blk, pcm + a, 16);       /* ASan: inside the allocation */
                sum += blk[0] ^ blk[1];
            }
            if (t.ndata) { /* the blocks cover the tile's bytes and no block is idle */
                const uint64_t begin = row.src0 + t0 * stride, end = begin + (uint64_t)t.ndata * stride;
                CHECK(t.blk0 <= begin && begin < t.blk0 + 16 && t.blk0 + t.phase == begin);
                CHECK(t.blk0 + 16ull * t.nblk >= end && t.blk0 + 16ull * (t.nblk - 1) < end);
            }
        }
    }
    if (sum == 1) puts(""); /* keeps the loads */
    free(out);
    free(wheap);
    free(pcm);
}

int main() {
    /* 3. the enumerations */
    for (uint32_t ch = 1; ch <= 8; ch++) {
        const uint32_t frames = bnf_f32_tile_frames(ch), pitch = bnf_f32_pitch(ch), magic = bnf_f32_magic(ch);
        CHECK(frames % 4 == 0 && frames >= 4 && frames <= BNF_F32_TILE_MAX && frames * ch <= BNF_F32_TILE_SAMPLES);
        CHECK(pitch >= frames + 4);
        CHECK(bnf_f32_stage_words(ch) <= BNF_F32_STAGE_WORDS && bnf_f32_stage_words(ch) % 4 == 0);
        CHECK((ch - 1) * pitch + frames + 4 <= bnf_f32_stage_words(ch) + 0u);
        CHECK((uint64_t)frames * ch * 4 + 30 <= 16ull * BNF_F32_RAW_BLOCKS);
        for (uint32_t e = 0; e < (1u << 14); e++) CHECK(bnf_f32_frame_of(e, magic) == e / ch);
        /* the 32 lanes of a ds_write_b32 group take samples [32 g, 32 g + 32): slot c * pitch + i, bank = slot % 32 */
        uint32_t worst = 0;
        for (uint32_t g = 0; g * 32 < frames * ch; g++) {
            uint32_t count[32] = {0};
            for (uint32_t e = 32 * g; e < 32 * g + 32 && e < frames * ch; e++) {
                const uint32_t i = e / ch, c = e % ch;
                const uint32_t b = (c * pitch + i) % 32;
                count[b]++;
                if (count[b] > worst) worst = count[b];
            }
        }
        CHECK(worst == (ch == 6 ? 2u : 1u));
    }
    for (uint32_t bps = 1; bps <= 32; bps++) {
        float k = 1.0f;
        double kd = 1.0;
        for (uint32_t i = 1; i < bps; i++) k *= 0.5f, kd *= 0.5;
        CHECK(bits(bnf_f32_scale(bps)) == bits(k) && bnf_f32_scale_d(bps) == kd);
    }
    /* 1. and 2. */
    for (const Layout &L : LAYOUTS)
        for (uint32_t tail16 : {0u, 2u, 15u})
            for (uint32_t flags : {0u, (uint32_t)BNF_F32_MONO}) {
                const uint32_t frames = bnf_f32_tile_frames(L.channels);
                for (uint32_t R : {0u, 1u, 1000u, frames + 5u}) {
                    one_case(L, tail16, flags, R, R);
                    one_case(L, tail16, flags, R, (uint64_t)R + 5);
                }
            }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    puts("gather_f32_sanitize: ok");
    return 0;
}
