/*
 * select_ranges_sanitize.cpp -- the host rule of csrc/bnf_select.h under AddressSanitizer and
 * UBSan.  A stand-alone program: every table is a heap allocation of exactly the size the
 * contract names (cap records, nstreams + 1 prefixes, sel_cap outputs), so a read at cap or a
 * write at sel_cap is a sanitizer report.  Each case is also checked against the rule written
 * out frame by frame (no binary search).  Exit 0: no report, no mismatch.
 *
 *   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I birdnest/audio_amd/csrc tools/select_ranges_sanitize.cpp -o select_ranges_sanitize
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bnf_select.h"

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

struct Tables {
    uint32_t cap = 0, nstreams = 0;
    bnf_frame_info *info = nullptr;
    uint32_t *sf = nullptr;
    uint64_t *ss = nullptr;
    ~Tables() {
        free(info);
        free(sf);
        free(ss);
    }
};

/* streams of the given frame counts, blocksizes 1..4608 with a short last frame, records of random bytes */
static void make(Tables &t, const std::vector<uint32_t> &nframes) {
    t.nstreams = (uint32_t)nframes.size();
    t.cap = 0;
    for (uint32_t n : nframes) t.cap += n;
    t.info = (bnf_frame_info *)malloc(sizeof(bnf_frame_info) * (t.cap ? t.cap : 1));
    t.sf = (uint32_t *)malloc(4 * (t.nstreams + 1));
    t.ss = (uint64_t *)malloc(8 * (t.nstreams + 1));
    uint32_t f = 0;
    uint64_t smp = 0;
    for (uint32_t s = 0; s < t.nstreams; s++) {
        t.sf[s] = f;
        t.ss[s] = smp;
        for (uint32_t k = 0; k < nframes[s]; k++, f++) {
            uint8_t *b = (uint8_t *)&t.info[f];
            for (size_t i = 0; i < sizeof(bnf_frame_info); i++) b[i] = (uint8_t)rnd();
            t.info[f].blocksize = k + 1 == nframes[s] ? 1 + (uint32_t)(rnd() % 100) : 1 + (uint32_t)(rnd() % 4608);
            t.info[f].out_sample = smp;
            smp += t.info[f].blocksize;
        }
    }
    t.sf[t.nstreams] = f;
    t.ss[t.nstreams] = smp;
}

struct Out {
    uint32_t sel_cap;
    bnf_frame_info *sel;
    uint32_t *sel_frames;
    uint64_t *sel_samples;
    bnf_window *win;
    uint32_t status[4];
    Out(uint32_t nstreams, uint32_t cap) : sel_cap(cap) {
        sel = (bnf_frame_info *)malloc(sizeof(bnf_frame_info) * (cap ? cap : 1));
        sel_frames = (uint32_t *)malloc(4 * (nstreams + 1));
        sel_samples = (uint64_t *)malloc(8 * (nstreams + 1));
        win = (bnf_window *)malloc(sizeof(bnf_window) * (nstreams ? nstreams : 1));
    }
    ~Out() {
        free(sel);
        free(sel_frames);
        free(sel_samples);
        free(win);
    }
};

static void run(const Tables &t, const bnf_sample_range *r, Out &o) {
    bnf_select_ranges_host(nullptr, t.info, t.cap, t.sf, t.ss, t.nstreams, r, nullptr, o.sel, o.sel_cap, o.sel_frames,
                           o.sel_samples, o.win, o.status);
}

/* the rule frame by frame, against a finished call over consistent tables */
static void verify(const Tables &t, const bnf_sample_range *r, const Out &o) {
    uint32_t nf = 0, nonempty = 0, clipped = 0;
    uint64_t ns = 0;
    for (uint32_t s = 0; s < t.nstreams; s++) {
        const uint64_t T = t.ss[s + 1] - t.ss[s];
        const uint64_t lo = r[s].first_sample < T ? r[s].first_sample : T;
        const uint64_t end = lo + r[s].nsamples < lo ? ~0ull : lo + r[s].nsamples;
        const uint64_t hi = end < T ? end : T;
        const uint64_t want_end = r[s].first_sample + r[s].nsamples < r[s].first_sample ? ~0ull : r[s].first_sample + r[s].nsamples;
        uint32_t a = t.sf[s + 1], b = t.sf[s + 1];
        bool in = false;
        for (uint32_t i = t.sf[s]; i < t.sf[s + 1] && hi > lo; i++) {
            const uint64_t L = t.info[i].out_sample - t.ss[s];
            const bool sel = L < hi && L + t.info[i].blocksize > lo;
            if (sel && !in) a = i, in = true;
            if (sel) b = i + 1;
        }
        const bnf_window &w = o.win[s];
        CHECK(o.sel_frames[s] == nf && o.sel_samples[s] == ns);
        CHECK(((w.flags & BNF_WIN_CLIPPED) != 0) == (want_end > T));
        clipped += want_end > T;
        if (!in) {
            CHECK((w.flags & BNF_WIN_EMPTY) && w.nframes == 0 && w.skip == 0 && w.nsamples == 0 && w.pcm_first == ns &&
                  w.first_frame == t.sf[s]);
            continue;
        }
        const uint64_t La = t.info[a].out_sample - t.ss[s];
        CHECK(!(w.flags & BNF_WIN_EMPTY) && w.first_frame == a && w.nframes == b - a && w.skip == lo - La &&
              w.nsamples == hi - lo && w.pcm_first == ns + w.skip && w.skip < t.info[a].blocksize);
        for (uint32_t i = a; i < b; i++) {
            const uint64_t p = (uint64_t)nf + (i - a);
            if (p >= o.sel_cap) break;
            bnf_frame_info x = t.info[i];
            x.out_sample = ns + (t.info[i].out_sample - t.info[a].out_sample);
            CHECK(!memcmp(&x, &o.sel[p], sizeof x));
        }
        nf += b - a;
        ns += t.info[b - 1].out_sample + t.info[b - 1].blocksize - t.info[a].out_sample;
        nonempty++;
    }
    CHECK(o.sel_frames[t.nstreams] == nf && o.sel_samples[t.nstreams] == ns);
    CHECK(o.status[0] == (nf > o.sel_cap ? 1u : 0u) && o.status[1] == nf && o.status[2] == nonempty && o.status[3] == clipped);
    bnf_frame_info filler;
    memset(&filler, 0, sizeof filler);
    filler.status = BNF_ST_SKIPPED;
    filler.err = -1;
    for (uint32_t p = nf; p < o.sel_cap; p++) CHECK(!memcmp(&filler, &o.sel[p], sizeof filler));
}

int main() {
    /* 1. every kind of window on one table: 0, 1 and many frames */
    {
        Tables t;
        make(t, {12, 1, 0, 40, 7, 3, 1, 25, 9, 9, 9, 9, 9, 9});
        std::vector<bnf_sample_range> r(t.nstreams);
        auto T = [&](uint32_t s) { return t.ss[s + 1] - t.ss[s]; };
        auto L = [&](uint32_t s, uint32_t k) { return t.info[t.sf[s] + k].out_sample - t.ss[s]; };
        r[0] = {L(0, 3) + 1, 1};                         /* inside one frame */
        r[1] = {0, ~0ull};                               /* to the end */
        r[2] = {0, 10};                                  /* no frames at all */
        r[3] = {L(3, 5) - 2, t.info[t.sf[3] + 5].blocksize + 4}; /* across boundaries */
        r[4] = {L(4, 2), 5};                             /* lo on a frame start */
        r[5] = {0, L(5, 1)};                             /* hi on a frame start */
        r[6] = {T(6) - 1, 1};                            /* the last sample */
        r[7] = {T(7), 4};                                /* first_sample == T */
        r[8] = {T(8) + 9, 4};                            /* first_sample > T */
        r[9] = {3, 0};                                   /* nsamples == 0 */
        r[10] = {5, ~0ull - 2};                          /* the sum wraps */
        r[11] = {~0ull, ~0ull};
        r[12] = {T(12) - 1, 2};                          /* clipped by one */
        r[13] = {0, T(13)};                              /* the whole stream, not clipped */
        for (uint32_t sel_cap : {t.cap + 5u, t.cap, 0u}) {
            Out o(t.nstreams, sel_cap);
            run(t, r.data(), o);
            verify(t, r.data(), o);
        }
        Out full(t.nstreams, t.cap);
        run(t, r.data(), full);
        const uint32_t total = full.status[1];
        Out shortby1(t.nstreams, total - 1); /* one short: nothing at sel_cap is written (the allocation ends there) */
        run(t, r.data(), shortby1);
        verify(t, r.data(), shortby1);
        CHECK(shortby1.status[0] == BNF_SEL_OVERFLOW);
    }
    /* 2. stream counts around the scan block, random windows */
    for (uint32_t n : {0u, 1u, 1025u}) {
        Tables t;
        std::vector<uint32_t> nf(n);
        for (auto &x : nf) x = (uint32_t)(rnd() % 6);
        make(t, nf);
        std::vector<bnf_sample_range> r(n ? n : 1);
        for (uint32_t s = 0; s < n; s++) {
            const uint64_t T = t.ss[s + 1] - t.ss[s];
            r[s] = {rnd() % (T + 3), rnd() % (T + 3)};
        }
        Out o(n, t.cap + 3);
        run(t, r.data(), o);
        verify(t, r.data(), o);
    }
    /* 3. unusable tables: the total above cap, then each table descending */
    for (int kind = 0; kind < 3; kind++) {
        Tables t;
        make(t, {4, 6, 2});
        std::vector<bnf_sample_range> r(3, bnf_sample_range{0, ~0ull});
        if (kind == 0) t.cap -= 1; /* the allocation keeps its size: a read at the new cap would still be inside it,
                                      so the check is the status and the filler */
        if (kind == 1) t.sf[1] = t.sf[2] + 1;
        if (kind == 2) t.ss[2] = t.ss[1] - 1;
        Out o(3, 16);
        run(t, r.data(), o);
        CHECK(o.status[0] == BNF_SEL_BAD_TABLES && !o.status[1] && !o.status[2] && !o.status[3]);
        for (uint32_t s = 0; s <= 3; s++) CHECK(o.sel_frames[s] == 0 && o.sel_samples[s] == 0);
        for (uint32_t s = 0; s < 3; s++) CHECK(o.win[s].flags == BNF_WIN_EMPTY && !o.win[s].nframes && !o.win[s].nsamples);
        for (uint32_t p = 0; p < 16; p++) CHECK(o.sel[p].status == BNF_ST_SKIPPED && o.sel[p].err == -1);
    }
    /* 4. out_sample values no index wrote: the call returns and stays inside each stream */
    for (int round = 0; round < 200; round++) {
        Tables t;
        make(t, {9, 1, 30, 0, 5});
        for (uint32_t i = 0; i < t.cap; i++) {
            const uint64_t x = rnd();
            t.info[i].out_sample = round & 1 ? x : x % 20000; /* anywhere, or shuffled nearby */
            if (round & 2) t.info[i].blocksize = (uint32_t)rnd();
        }
        std::vector<bnf_sample_range> r(t.nstreams);
        for (auto &x : r) x = {rnd() % 9000, round & 4 ? ~0ull : rnd() % 9000};
        Out o(t.nstreams, t.cap);
        run(t, r.data(), o);
        for (uint32_t s = 0; s < t.nstreams; s++) {
            const bnf_window &w = o.win[s];
            CHECK(w.first_frame >= t.sf[s] && w.first_frame <= t.sf[s + 1] && w.nframes <= t.sf[s + 1] - w.first_frame);
        }
        CHECK(o.status[1] <= t.cap);
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    puts("select_ranges_sanitize: ok");
    return 0;
}
