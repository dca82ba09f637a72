/*
 * gather_mel_sanitize.cpp -- the host rule of csrc/bnf_mel.h under AddressSanitizer and UBSan.
 * A stand-alone program: the PCM is a heap allocation of exactly round_up(pcm_bytes, 16) bytes, the
 * float table one of exactly 2 n_fft + n_weights floats, the band table one of exactly 2 (n_mels + 1)
 * words and the output one of exactly (nstreams * planes * rows - 1) * frame_pitch + row_frames
 * floats (the host twin's raw blocks, work area and ybuf are exact allocations of its own), so a read
 * or a write outside the contract is a sanitizer report.  Parts:
 *   1. layouts x specs x pcm_bytes % 16 in {0, 2, 15} x flags x row_frames x pitch x origin:
 *      bnf_gather_mel_host against the rule written out frame by frame (no tiles, no steps, no
 *      blocks, one stage at a time; the operations in the order the contract names), bit for bit,
 *      with windows shorter than a frame, empty, touching the last sample frame and bad, origins
 *      past the window and below -n_fft, row_frames 0, 1, below and above n_valid, and band tables
 *      with descending, overlong and out-of-range bands among them;
 *   2. the enumerations the header's comments promise: the plan's LDS fits a CU and a step's span
 *      the raw stage for every layout and size, and the design and request functions on exact
 *      allocations.
 * Exit 0: no report, no mismatch.
 *
 *   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I birdnest/audio_amd/csrc tools/gather_mel_sanitize.cpp -o gather_mel_sanitize
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bnf_mel.h"

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
                                 {"fr 8x24", 8, 24, 3}, {"i32 1x32", 1, 32, 4}, {"i32 8x24", 8, 24, 4}};
struct Shape {
    uint32_t n_fft, hop, n_mels, n_weights;
    int bad_bands; /* spoil some bands */
};
static const Shape SHAPES[] = {{64, 16, 10, 70, 0},   {64, 1, 0, 0, 0},      {128, 37, 1, 65, 0},    {256, 300, 40, 500, 1},
                               {512, 128, 0, 0, 0},   {1024, 256, 128, 1008, 0}, {2048, 65535, 256, 8192, 1}, {2048, 700, 0, 0, 0}};

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

/* One frame by the contract's words: u -> rows (n_mels or N/2 + 1 floats). */
static void frame_rule(const std::vector<float> &u, const bnf_mel_spec &sp, const float *tab, const uint32_t *bands,
                       std::vector<float> &rows) {
    const uint32_t N = sp.n_fft, lg = bnf_mel_log2(N);
    const float *C = tab + N; /* pairs */
    std::vector<float> re(N), im(N, 0.0f);
    for (uint32_t i = 0; i < N; i++) {
        uint32_t r = 0;
        for (uint32_t b = 0; b < lg; b++)
            if (i & (1u << b)) r |= 1u << (lg - 1 - b);
        re[r] = u[i];
    }
    for (uint32_t h = 1; h < N; h *= 2)
        for (uint32_t b = 0; b < N; b += 2 * h)
            for (uint32_t j = 0; j < h; j++) {
                const uint32_t k = j * (N / (2 * h));
                const float c = C[2 * k], s = C[2 * k + 1];
                const float br = re[b + j + h], bi = im[b + j + h];
                volatile float pr = bi * s; /* kept apart from the fmaf */
                const float tr = fmaf(br, c, pr);
                volatile float pi = br * s;
                const float ti = fmaf(bi, c, -pi);
                const float ar = re[b + j], ai = im[b + j];
                re[b + j] = ar + tr;
                im[b + j] = ai + ti;
                re[b + j + h] = ar - tr;
                im[b + j + h] = ai - ti;
            }
    std::vector<float> P(N / 2 + 1);
    for (uint32_t k = 0; k <= N / 2; k++) {
        volatile float q = im[k] * im[k];
        P[k] = fmaf(re[k], re[k], q);
    }
    if (!sp.n_mels) {
        rows = P;
        return;
    }
    rows.assign(sp.n_mels, 0.0f);
    for (uint32_t m = 0; m < sp.n_mels; m++) {
        const uint64_t f = bands[2 * m], w0 = bands[2 * m + 1], w1 = bands[2 * m + 3];
        if (w1 < w0 || w1 > sp.n_weights || f + (w1 - w0) > N / 2 + 1) continue;
        float acc = 0.0f;
        for (uint64_t i = 0; i < w1 - w0; i++) acc = fmaf(tab[2 * N + w0 + i], P[f + i], acc);
        rows[m] = acc;
    }
}

static void one_case(const Layout &L, const Shape &Q, uint32_t tail16, uint32_t flags, uint32_t R, uint64_t pitch, int32_t origin) {
    const uint32_t stride = L.unit * L.channels, planes = flags & BNF_F32_MONO ? 1u : L.channels;
    const uint32_t N = Q.n_fft;
    bnf_mel_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.n_fft = N;
    sp.hop = Q.hop;
    sp.n_mels = Q.n_mels;
    sp.origin = origin;
    sp.n_weights = Q.n_weights;
    CHECK(bnf_mel_spec_refusal(sp, R, pitch) == nullptr);
    const uint32_t rows = Q.n_mels ? Q.n_mels : N / 2 + 1;
    uint64_t full = (uint64_t)(R ? R - 1 : 0) * Q.hop + N; /* sample frames that give about R frames */
    if (full > 6000) full = 6000;                            /* or as many as keep the case small */
    uint64_t nsmp = full + 40, pcm_bytes = nsmp * stride;
    while (pcm_bytes % 16 != tail16 && pcm_bytes < nsmp * stride + 64) pcm_bytes++;
    nsmp = pcm_bytes / stride;
    const size_t alloc = (size_t)((pcm_bytes + 15) & ~15ull);
    uint8_t *pcm = (uint8_t *)malloc(alloc);
    for (size_t i = 0; i < alloc; i++) pcm[i] = (uint8_t)rnd();
    /* the tables: a random window and weights, a design's twiddles */
    const size_t ntab = 2 * (size_t)N + Q.n_weights;
    float *tab = (float *)malloc(sizeof(float) * ntab);
    for (uint32_t i = 0; i < N; i++) tab[i] = (float)((double)(int64_t)(rnd() % 2001 - 1000) / 1000.0);
    for (uint32_t k = 0; k < N / 2; k++) {
        tab[N + 2 * k] = (float)cos(2.0 * 3.14159265358979323846 * k / N);
        tab[N + 2 * k + 1] = (float)sin(2.0 * 3.14159265358979323846 * k / N);
    }
    for (uint32_t i = 0; i < Q.n_weights; i++) tab[2 * N + i] = (float)((double)(int64_t)(rnd() % 2001 - 500) / 1000.0);
    uint32_t *bands = nullptr, nbadb = 0;
    if (Q.n_mels) {
        bands = (uint32_t *)malloc(sizeof(uint32_t) * 2 * (Q.n_mels + 1));
        for (uint32_t m = 0; m <= Q.n_mels; m++) {
            bands[2 * m + 1] = (uint32_t)((uint64_t)Q.n_weights * m / Q.n_mels);
            bands[2 * m] = (uint32_t)(rnd() % (N / 2 + 2 - (Q.n_weights + Q.n_mels - 1) / Q.n_mels));
        }
        if (Q.bad_bands) {
            bands[2 * 3 + 1] = bands[2 * 4 + 1] + 5;         /* band 3 descends */
            bands[2 * 7] = N / 2 + 1;                         /* band 7 starts behind the last bin */
            bands[2 * 9] = 0xffffffffu;                       /* band 9 starts nowhere */
            bands[2 * Q.n_mels + 1] = Q.n_weights + 1;        /* the last band runs past the weights */
            if (Q.n_mels > 20) bands[2 * 15 + 1] = 0xfffffff0u; /* band 14 overlong, band 15 descends */
        }
        for (uint32_t m = 0; m < Q.n_mels; m++) {
            uint32_t f, w, nb;
            nbadb += bnf_mel_band_of(bands, m, sp, f, w, nb);
        }
        CHECK(Q.bad_bands ? nbadb >= 4 : nbadb == 0);
    }
    std::vector<bnf_window> win;
    auto add = [&](uint64_t first, uint64_t n) {
        bnf_window w;
        memset(&w, 0, sizeof w);
        w.pcm_first = first;
        w.nsamples = n;
        win.push_back(w);
    };
    const uint64_t lens[] = {0, 1, N - 1, N, full > 2 * Q.hop && 2 * Q.hop < full ? full - 2 * (Q.hop < 100 ? Q.hop : 100) : 0, full, full + 7};
    for (uint64_t n : lens)
        for (uint64_t first = 0; first < 2; first++)
            if (first + n <= nsmp) add(first + 2 * (n & 1), n);
    add(nsmp - full, full); /* ends at the last whole sample frame */
    add(nsmp, 0);
    add(nsmp - 1, 2); /* one sample frame past it */
    add(~0ull, 1);
    add(~0ull, 0); /* empty, wherever it points */
    add(5, ~0ull);
    const uint32_t n = (uint32_t)win.size();
    bnf_window *wheap = (bnf_window *)malloc(sizeof(bnf_window) * n);
    memcpy(wheap, win.data(), sizeof(bnf_window) * n);
    const size_t nout = (size_t)(((uint64_t)n * planes * rows - 1) * pitch + R);
    float *out = (float *)malloc(4 * (nout ? nout : 1));
    for (size_t i = 0; i < nout; i++) memcpy(out + i, &CANARY, 4);
    uint32_t status[4] = {9, 9, 9, 9};
    CHECK(bnf_gather_mel_host(pcm, pcm_bytes, stride, L.unit, L.bps, L.channels, flags, wheap, n, sp, tab, bands, R, pitch, out,
                              status) == 0);
    /* the rule frame by frame */
    const float k = bnf_f32_scale(L.bps);
    const double kd = bnf_f32_scale_d(L.bps);
    uint32_t nbad = 0, ncut = 0;
    std::vector<uint8_t> written(nout ? nout : 1, 0);
    std::vector<float> u(N), val;
    for (uint32_t s = 0; s < n; s++) {
        const uint64_t first = win[s].pcm_first, want = win[s].nsamples;
        const bool bad = want != 0 && (first > nsmp || want > nsmp - first);
        nbad += bad;
        uint64_t nv = 0;
        if (!bad && want) {
            const int64_t c = (int64_t)want - (int64_t)(N / 2) - (int64_t)origin;
            if (c >= 0) nv = (uint64_t)c / Q.hop + 1;
        }
        ncut += nv > R;
        const uint64_t ncopy = nv < R ? nv : R;
        for (uint32_t c = 0; c < planes; c++)
            for (uint32_t t = 0; t < R; t++) {
                if (t < ncopy) {
                    const int64_t a = (int64_t)origin + (int64_t)t * Q.hop;
                    for (uint32_t i = 0; i < N; i++) {
                        const int64_t p = a + i;
                        float x = 0.0f;
                        if (p >= 0 && (uint64_t)p < want) {
                            const uint8_t *fr = pcm + (first + (uint64_t)p) * stride;
                            if (flags & BNF_F32_MONO) {
                                int64_t S = 0;
                                for (uint32_t ch = 0; ch < L.channels; ch++) S += sample_at(fr + ch * L.unit, L.unit);
                                x = (float)((double)S * kd / (double)L.channels);
                            } else {
                                x = (float)sample_at(fr + c * L.unit, L.unit) * k;
                            }
                        }
                        volatile float prod = tab[i] * x;
                        u[i] = prod;
                    }
                    frame_rule(u, sp, tab, bands, val);
                }
                for (uint32_t r = 0; r < rows; r++) {
                    const float f = t < ncopy ? val[r] : 0.0f;
                    const size_t at = (size_t)((((uint64_t)s * planes + c) * rows + r) * pitch + t);
                    written[at] = 1;
                    if (bits(out[at]) != bits(f)) {
                        if (failures < 20)
                            fprintf(stderr, "%s N %u hop %u mels %u flags %u R %u pitch %llu tail %u origin %d: window %u plane %u row %u frame %u: %08x, want %08x\n",
                                    L.name, N, Q.hop, Q.n_mels, flags, R, (unsigned long long)pitch, tail16, origin, s, c, r, t,
                                    bits(out[at]), bits(f));
                        failures++;
                    }
                }
            }
    }
    for (size_t i = 0; i < nout; i++)
        if (!written[i]) CHECK(bits(out[i]) == CANARY);
    CHECK(status[0] == ((nbad ? 1u : 0u) | (nbadb ? 2u : 0u)) && status[1] == nbad && status[2] == ncut && status[3] == nbadb);
    free(out);
    free(wheap);
    free(bands);
    free(tab);
    free(pcm);
}

int main() {
    /* 2. the enumerations */
    for (uint32_t N = BNF_MEL_MIN_FFT; N <= BNF_MEL_MAX_FFT; N *= 2)
        for (uint32_t ch = 1; ch <= 8; ch++)
            for (uint32_t unit = 2; unit <= 4; unit++)
                for (const uint32_t hop : {1u, 2u, 37u, N / 4, N, N + 1, 65535u})
                    for (const uint32_t mels : {0u, 1u, 40u, 256u}) {
                        bnf_mel_spec sp;
                        memset(&sp, 0, sizeof sp);
                        sp.n_fft = N;
                        sp.hop = hop;
                        sp.n_mels = mels;
                        sp.n_weights = mels ? BNF_MEL_MAX_WEIGHTS : 0;
                        for (const uint32_t planes : {1u, ch}) {
                            const bnf_mel_plan pl = bnf_mel_plan_of(sp, ch * unit, planes);
                            CHECK(pl.lds_bytes <= 160u * 1024u && pl.G * pl.tpf == BNF_MEL_THREADS && pl.sf >= 1 && pl.sf <= BNF_MEL_TF);
                            CHECK(((uint64_t)(pl.sf - 1) * hop + N) * ch * unit + 32 <= pl.raw_bytes); /* a step's span at any phase */
                            CHECK(!(pl.off_wt % 16) && !(pl.off_bands % 16) && !(pl.off_raw % 16) && !(pl.off_work % 16) && !(pl.off_ybuf % 16));
                            CHECK(pl.off_ybuf + 4 * pl.pass_rows * BNF_MEL_YPITCH <= pl.lds_bytes && (1u << pl.log2n) == N);
                            CHECK(pl.pass_rows >= 1 && pl.pass_rows <= pl.rows && (mels == 0 || pl.pass_rows == pl.rows));
                        }
                    }
    for (uint32_t a = 0; a < 4; a++) { /* the pieces of a row cover 32 floats at any phase, each float once */
        int seen[BNF_MEL_TF] = {0};
        for (uint32_t j = 0; j < BNF_MEL_PIECES; j++)
            for (int e = 0; e < 4; e++) {
                const int32_t p = bnf_mel_piece(a, j) + e;
                if (p >= 0 && p < (int32_t)BNF_MEL_TF) seen[p]++;
            }
        for (uint32_t p = 0; p < BNF_MEL_TF; p++) CHECK(seen[p] == 1);
    }
    { /* the design and the request on exact allocations */
        bnf_mel_spec sp;
        uint64_t nw = 0;
        CHECK(bnf_mel_design_spec(48000, 1024, 256, 128, 0.0, 24000.0, sp, nw) == nullptr && sp.n_mels == 128 && sp.origin == -512);
        CHECK(nw == sp.n_weights && nw > 128 && nw <= 2 * 513);
        float *t = (float *)malloc(sizeof(float) * (2 * 1024 + sp.n_weights));
        uint32_t *b = (uint32_t *)malloc(sizeof(uint32_t) * 2 * 129);
        bnf_mel_design_tables(48000, sp, 0.0, 24000.0, t, b);
        CHECK(t[0] == 0.0f && t[512] == 1.0f && t[1024] == 1.0f && t[1025] == 0.0f && b[2 * 128 + 1] == sp.n_weights && b[1] == 0);
        for (uint32_t m = 0; m < 128; m++) {
            uint32_t f, w, nb;
            CHECK(bnf_mel_band_of(b, m, sp, f, w, nb) == 0);
            for (uint32_t i = 0; i < nb; i++) CHECK(t[2048 + w + i] > 0.0f && t[2048 + w + i] <= 1.0f);
        }
        free(t);
        free(b);
        CHECK(bnf_mel_design_spec(48000, 1024, 256, 300, 0.0, 24000.0, sp, nw) != nullptr && nw > 300);
        CHECK(bnf_mel_design_spec(0, 1024, 256, 40, 0.0, 24000.0, sp, nw) != nullptr);
        CHECK(bnf_mel_design_spec(48000, 64, 1, 0, 0.0, 24000.0, sp, nw) == nullptr && sp.n_weights == 0);
        float t0[128];
        bnf_mel_design_tables(48000, sp, 0.0, 24000.0, t0, nullptr);
        const bnf_mel_spec q = {1024, 256, 0, -512, 0, {0, 0, 0}};
        uint64_t first, n;
        int32_t o;
        bnf_mel_request(q, 0, 10, first, n, o);
        CHECK(first == 0 && o == -512 && n == 9 * 256 + 512);
        bnf_mel_request(q, 100, 10, first, n, o);
        CHECK(first == 100 * 256 - 512 && o == 0 && n == 9 * 256 + 1024);
        bnf_mel_request(q, 1, 0, first, n, o);
        CHECK(n == 0);
    }
    /* 1. */
    for (const Layout &L : LAYOUTS)
        for (const Shape &Q : SHAPES)
            for (uint32_t flags : {0u, (uint32_t)BNF_F32_MONO}) {
                if (Q.n_fft >= 1024 && L.channels == 8 && !flags) continue; /* keeps the run short: 8 planes of large frames */
                const uint32_t tail16 = L.unit == 3 ? 15u : L.unit == 2 ? 2u : 0u;
                const int32_t half = -(int32_t)(Q.n_fft / 2);
                const uint32_t big = Q.n_fft >= 1024 ? 5u : BNF_MEL_TF + 5u;
                one_case(L, Q, tail16, flags, big, big + 3u, half);
                one_case(L, Q, 0, flags, 1, 1, 0);
                one_case(L, Q, tail16, flags, 0, 2, half);
                one_case(L, Q, tail16, flags, 3, 4, 17);                       /* positive, inside short windows' reach */
                one_case(L, Q, tail16, flags, 2, 2, 100000);                   /* past every window */
                one_case(L, Q, tail16, flags, 3, 3, -(int32_t)Q.n_fft - 1);    /* frame 0 wholly in front */
                if (Q.n_fft == 64) one_case(L, Q, tail16, flags, 2, 2, INT32_MIN);
            }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    puts("gather_mel_sanitize: ok");
    return 0;
}
