/*
 * gather_rs_sanitize.cpp -- the host rule of csrc/bnf_resample.h under AddressSanitizer and UBSan.
 * A stand-alone program: the PCM is a heap allocation of exactly round_up(pcm_bytes, 16) bytes, the
 * table one of exactly up * taps floats and the output one of exactly (nstreams * planes - 1) *
 * plane_pitch + row_out floats (the host twin's raw blocks, stage and store buffer are exact
 * allocations of its own), so a read or a write outside the contract is a sanitizer report.  Parts:
 *   1. layouts x ratios x pcm_bytes % 16 in {0, 2, 15} x flags x pitch: bnf_gather_f32_rs_host against
 *      the rule written out output by output (no tiles, no steps, no blocks; fmaf in the order the
 *      contract names), bit for bit, with windows touching the last sample frame, bad windows and
 *      out_first past the outputs among them;
 *   2. the enumerations the header's comments promise: the step's span fits the stage for every
 *      channel count and extreme ratio, and the design and request functions on exact allocations.
 * Exit 0: no report, no mismatch.
 *
 *   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I birdnest/audio_amd/csrc tools/gather_rs_sanitize.cpp -o gather_rs_sanitize
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bnf_resample.h"

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
static const Layout LAYOUTS[] = {{"fd 2x16", 2, 16, 2}, {"fr 1x24", 1, 24, 3}, {"fr 3x16", 3, 16, 2},
                                 {"fr 8x24", 8, 24, 3}, {"i32 1x32", 1, 32, 4}, {"i32 3x20", 3, 20, 4}};
struct Ratio {
    uint32_t up, down, taps;
};
static const Ratio RATIOS[] = {{160, 147, 32}, {147, 160, 36}, {1, 2, 64}, {3, 2, 4}, {1, 8, 8}, {1, 1, 4}, {1, 700, 512}, {4096, 1, 4}};

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

static const uint32_t CANARY = 0x7fc5a5a5u; /* a NaN: the tables below are finite, so no value is one */

static void one_case(const Layout &L, const Ratio &Q, uint32_t tail16, uint32_t flags, uint32_t R, uint64_t pitch,
                     uint32_t out_first) {
    const uint32_t stride = L.unit * L.channels, planes = flags & BNF_F32_MONO ? 1u : L.channels;
    bnf_rsmp_spec sp = {Q.up, Q.down, Q.taps, out_first};
    CHECK(bnf_rsmp_spec_refusal(sp, R) == nullptr);
    uint64_t full = ((uint64_t)(R + out_first) * Q.down + Q.up - 1) / Q.up; /* sample frames that give R outputs */
    if (full > 9000) full = 9000;                                           /* or as many as keep the case small */
    uint64_t nsmp = full + 40, pcm_bytes = nsmp * stride;
    while (pcm_bytes % 16 != tail16 && pcm_bytes < nsmp * stride + 64) pcm_bytes++;
    nsmp = pcm_bytes / stride;
    const size_t alloc = (size_t)((pcm_bytes + 15) & ~15ull);
    uint8_t *pcm = (uint8_t *)malloc(alloc);
    for (size_t i = 0; i < alloc; i++) pcm[i] = (uint8_t)rnd();
    float *taps = (float *)malloc(sizeof(float) * Q.up * Q.taps);
    for (uint32_t i = 0; i < Q.up * Q.taps; i++) taps[i] = (float)((double)(int64_t)(rnd() % 2001 - 1000) / 1000.0 / Q.taps);
    std::vector<bnf_window> win;
    auto add = [&](uint64_t first, uint64_t n) {
        bnf_window w;
        memset(&w, 0, sizeof w);
        w.pcm_first = first;
        w.nsamples = n;
        win.push_back(w);
    };
    const uint64_t lens[] = {0, 1, 3, Q.taps / 2, full > 2 ? full - 2 : 0, full, full + 7};
    for (uint64_t n : lens)
        for (uint64_t first = 0; first < 3; first++)
            if (first + n <= nsmp) add(first, n);
    add(nsmp - full, full); /* ends at the last whole sample frame */
    add(nsmp, 0);
    add(nsmp - 1, 2); /* one sample frame past it */
    add(~0ull, 1);
    add(~0ull, 0); /* empty, wherever it points */
    add(5, ~0ull);
    const uint32_t n = (uint32_t)win.size();
    bnf_window *wheap = (bnf_window *)malloc(sizeof(bnf_window) * n);
    memcpy(wheap, win.data(), sizeof(bnf_window) * n);
    const size_t nout = (size_t)(((uint64_t)n * planes - 1) * pitch + R);
    float *out = (float *)malloc(4 * (nout ? nout : 1));
    for (size_t i = 0; i < nout; i++) memcpy(out + i, &CANARY, 4);
    uint32_t status[4] = {9, 9, 9, 9};
    CHECK(bnf_gather_f32_rs_host(pcm, pcm_bytes, stride, L.unit, L.bps, L.channels, flags, wheap, n, sp, taps, R, pitch, out,
                                 status) == 0);
    /* the rule output by output */
    const float k = bnf_f32_scale(L.bps);
    const double kd = bnf_f32_scale_d(L.bps);
    const int64_t c0 = Q.taps / 2 - 1;
    uint32_t nbad = 0, ncut = 0;
    std::vector<uint8_t> written(nout ? nout : 1, 0);
    for (uint32_t s = 0; s < n; s++) {
        const uint64_t first = win[s].pcm_first, want = win[s].nsamples;
        const bool bad = want != 0 && (first > nsmp || want > nsmp - first);
        nbad += bad;
        const uint64_t total = bad ? 0 : (want * Q.up + Q.down - 1) / Q.down;
        const uint64_t n_out = total > out_first ? total - out_first : 0;
        ncut += n_out > R;
        const uint64_t ncopy = n_out < R ? n_out : R;
        for (uint32_t c = 0; c < planes; c++)
            for (uint32_t r = 0; r < R; r++) {
                float f = 0.0f;
                if (r < ncopy) {
                    const uint64_t jm = (uint64_t)(r + out_first) * Q.down;
                    const int64_t q = (int64_t)(jm / Q.up);
                    const float *h = taps + (jm % Q.up) * Q.taps;
                    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    for (uint32_t t = 0; t < Q.taps; t++) {
                        const int64_t i = q + (int64_t)t - c0;
                        float x = 0.0f;
                        if (i >= 0 && (uint64_t)i < want) {
                            const uint8_t *fr = pcm + (first + (uint64_t)i) * stride;
                            if (flags & BNF_F32_MONO) {
                                int64_t S = 0;
                                for (uint32_t ch = 0; ch < L.channels; ch++) S += sample_at(fr + ch * L.unit, L.unit);
                                x = (float)((double)S * kd / (double)L.channels);
                            } else {
                                x = (float)sample_at(fr + c * L.unit, L.unit) * k;
                            }
                        }
                        a[t & 3] = fmaf(h[t], x, a[t & 3]);
                    }
                    f = (a[0] + a[1]) + (a[2] + a[3]);
                }
                const size_t at = (size_t)(((uint64_t)s * planes + c) * pitch + r);
                written[at] = 1;
                if (bits(out[at]) != bits(f)) {
                    if (failures < 20)
                        fprintf(stderr, "%s %u/%u K %u flags %u R %u pitch %llu tail %u first %u: window %u plane %u output %u: %08x, want %08x\n",
                                L.name, Q.up, Q.down, Q.taps, flags, R, (unsigned long long)pitch, tail16, out_first, s, c, r,
                                bits(out[at]), bits(f));
                    failures++;
                }
            }
    }
    for (size_t i = 0; i < nout; i++)
        if (!written[i]) CHECK(bits(out[i]) == CANARY);
    CHECK(status[0] == (nbad ? 1u : 0u) && status[1] == nbad && status[2] == ncut && status[3] == 0);
    free(out);
    free(wheap);
    free(taps);
    free(pcm);
}

int main() {
    /* 2. the enumerations */
    for (uint32_t ch = 1; ch <= 8; ch++) {
        const uint32_t F = bnf_f32_tile_frames(ch);
        CHECK(F >= BNF_RSMP_MAX_TAPS);
        for (uint32_t K = 4; K <= BNF_RSMP_MAX_TAPS; K += 4)
            for (const uint32_t up : {1u, 2u, 3u, 147u, 160u, 4096u, 65535u})
                for (const uint32_t down : {1u, 2u, 7u, 147u, 160u, 65535u}) {
                    const bnf_rsmp_spec sp = {up, down, K, 0};
                    const uint32_t so = bnf_rsmp_step_outputs(sp, ch);
                    CHECK(so >= 1 && so <= BNF_RSMP_TILE);
                    /* the widest span of so outputs: ceil((so - 1) M / L) + K */
                    CHECK(((uint64_t)(so - 1) * down + up - 1) / up + K <= F);
                    CHECK((ch - 1) * bnf_f32_pitch(ch) + F <= bnf_f32_stage_words(ch));
                }
        CHECK(bnf_rsmp_tap_pitch(4 * ch) % 8 == 4 && bnf_rsmp_tap_pitch(4 * ch) >= 4 * ch);
    }
    CHECK(2 * BNF_RSMP_YBUF * 4 <= 16 * BNF_F32_RAW_BLOCKS);
    { /* the design and the request on exact allocations */
        bnf_rsmp_spec sp;
        uint64_t K = 0;
        CHECK(bnf_rsmp_design_spec(44100, 48000, 16.0, sp, K) == nullptr && sp.up == 160 && sp.down == 147 && sp.taps == 32);
        float *t = (float *)malloc(sizeof(float) * sp.up * sp.taps);
        bnf_rsmp_design_taps(sp, 0.945, 9.0, t);
        for (uint32_t ph = 0; ph < sp.up; ph++) {
            double sum = 0;
            for (uint32_t k = 0; k < sp.taps; k++) sum += t[ph * sp.taps + k];
            CHECK(fabs(sum - 1.0) < 32 * 6e-8);
        }
        free(t);
        CHECK(bnf_rsmp_design_spec(11025, 48000, 16.0, sp, K) != nullptr && K == 32 && sp.up == 640);
        CHECK(bnf_rsmp_design_spec(0, 48000, 16.0, sp, K) != nullptr);
        CHECK(bnf_rsmp_design_spec(5, 5, 16.0, sp, K) == nullptr && sp.taps == 4);
        float id[4];
        bnf_rsmp_design_taps(sp, 0.945, 9.0, id);
        CHECK(id[0] == 0 && id[1] == 1 && id[2] == 0 && id[3] == 0);
        const bnf_rsmp_spec q = {160, 147, 32, 0};
        uint64_t first, n, of;
        bnf_rsmp_request(q, 1000, 100, first, n, of);
        CHECK(first == 147 * 6 && of == 1000 - 160 * 6 && n == 1099 * 147 / 160 + 17 - first);
    }
    /* 1. */
    for (const Layout &L : LAYOUTS)
        for (const Ratio &Q : RATIOS)
            for (uint32_t flags : {0u, (uint32_t)BNF_F32_MONO}) {
                const uint32_t tail16 = L.unit == 3 ? 15u : L.unit == 2 ? 2u : 0u;
                one_case(L, Q, tail16, flags, BNF_RSMP_TILE + 5u, BNF_RSMP_TILE + 10u, 3);
                one_case(L, Q, 0, flags, 37, 37, 0);
                one_case(L, Q, tail16, flags, 0, 0, 0);
                one_case(L, Q, tail16, flags, 9, 9, 100000);
            }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    puts("gather_rs_sanitize: ok");
    return 0;
}
