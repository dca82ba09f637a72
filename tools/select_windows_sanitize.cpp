/*
 * select_windows_sanitize.cpp -- the host rule of bnflac_select_windows (csrc/bnf_select.h) under
 * AddressSanitizer and UBSan.  A stand-alone program: every table is a heap allocation of exactly
 * the size the contract names (cap records, nstreams + 1 prefixes, nwindows requests and windows,
 * nwindows + 1 output prefixes, sel_cap records), so a read at cap, a table entry read for a
 * request that names no stream, or a write at sel_cap is a sanitizer report.  Each case over
 * consistent tables is also checked against the rule written out frame by frame per request (no
 * binary search).  Exit 0: no report, no mismatch.
 *
 *   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I birdnest/audio_amd/csrc tools/select_windows_sanitize.cpp -o select_windows_sanitize
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bnf_select.h"

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
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

/* streams of the given frame counts, records of random bytes; blocksizes 1..4608 with a short last
 * frame, or all 1 */
static void make(Tables &t, const std::vector<uint32_t> &nframes, bool unit = false) {
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
            t.info[f].blocksize = unit ? 1u : k + 1 == nframes[s] ? 1 + (uint32_t)(rnd() % 100) : 1 + (uint32_t)(rnd() % 4608);
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
    Out(uint32_t nwindows, uint32_t cap) : sel_cap(cap) {
        sel = (bnf_frame_info *)malloc(sizeof(bnf_frame_info) * (cap ? cap : 1));
        sel_frames = (uint32_t *)malloc(4 * ((size_t)nwindows + 1));
        sel_samples = (uint64_t *)malloc(8 * ((size_t)nwindows + 1));
        win = (bnf_window *)malloc(sizeof(bnf_window) * (nwindows ? nwindows : 1));
    }
    ~Out() {
        free(sel);
        free(sel_frames);
        free(sel_samples);
        free(win);
    }
};

/* the requests as an exact allocation too */
struct Requests {
    uint32_t n;
    bnf_window_request *q;
    explicit Requests(const std::vector<bnf_window_request> &v) : n((uint32_t)v.size()) {
        q = (bnf_window_request *)malloc(sizeof(bnf_window_request) * (n ? n : 1));
        if (n) memcpy(q, v.data(), sizeof(bnf_window_request) * n);
    }
    ~Requests() { free(q); }
};

static void run(const Tables &t, const Requests &r, Out &o) {
    bnf_select_windows_host(nullptr, t.info, t.cap, t.sf, t.ss, t.nstreams, r.q, r.n, nullptr, o.sel, o.sel_cap, o.sel_frames,
                            o.sel_samples, o.win, o.status);
}

static bool is_filler(const bnf_frame_info &x) {
    bnf_frame_info filler;
    memset(&filler, 0, sizeof filler);
    filler.status = BNF_ST_SKIPPED;
    filler.err = -1;
    return !memcmp(&filler, &x, sizeof filler);
}

/* the rule frame by frame per request, against a finished call whose named slices are consistent */
static void verify(const Tables &t, const Requests &r, const Out &o) {
    uint64_t nf = 0, ns = 0;
    uint32_t nonempty = 0, clipped = 0;
    bool none = false;
    for (uint32_t w = 0; w < r.n; w++) {
        const bnf_window &win = o.win[w];
        CHECK(o.sel_frames[w] == (nf > 0xffffffffull ? 0xffffffffu : (uint32_t)nf) && o.sel_samples[w] == ns);
        const uint64_t s = r.q[w].stream, first = r.q[w].first_sample, want = r.q[w].nsamples;
        if (s >= t.nstreams) {
            none = true;
            CHECK(win.flags == (BNF_WIN_EMPTY | BNF_WIN_NO_STREAM) && !win.first_frame && !win.nframes && !win.skip &&
                  !win.nsamples && win.pcm_first == ns);
            continue;
        }
        const uint64_t T = t.ss[s + 1] - t.ss[s];
        const uint64_t lo = first < T ? first : T;
        const uint64_t end = lo + want < lo ? ~0ull : lo + want;
        const uint64_t hi = end < T ? end : T;
        const uint64_t want_end = first + want < first ? ~0ull : first + want;
        uint32_t a = t.sf[s + 1], b = t.sf[s + 1];
        bool in = false;
        for (uint32_t i = t.sf[s]; i < t.sf[s + 1] && hi > lo; i++) {
            const uint64_t L = t.info[i].out_sample - t.ss[s];
            const bool sel = L < hi && L + t.info[i].blocksize > lo;
            if (sel && !in) a = i, in = true;
            if (sel) b = i + 1;
        }
        CHECK(!(win.flags & BNF_WIN_NO_STREAM) && ((win.flags & BNF_WIN_CLIPPED) != 0) == (want_end > T));
        clipped += want_end > T;
        if (!in) {
            CHECK((win.flags & BNF_WIN_EMPTY) && win.nframes == 0 && win.skip == 0 && win.nsamples == 0 && win.pcm_first == ns &&
                  win.first_frame == t.sf[s]);
            continue;
        }
        const uint64_t La = t.info[a].out_sample - t.ss[s];
        CHECK(!(win.flags & BNF_WIN_EMPTY) && win.first_frame == a && win.nframes == b - a && win.skip == lo - La &&
              win.nsamples == hi - lo && win.pcm_first == ns + win.skip && win.skip < t.info[a].blocksize);
        for (uint32_t i = a; i < b; i++) {
            const uint64_t p = nf + (i - a);
            if (p >= o.sel_cap) break;
            bnf_frame_info x = t.info[i];
            x.out_sample = ns + (t.info[i].out_sample - t.info[a].out_sample);
            CHECK(!memcmp(&x, &o.sel[p], sizeof x));
        }
        nf += b - a;
        ns += t.info[b - 1].out_sample + t.info[b - 1].blocksize - t.info[a].out_sample;
        nonempty++;
    }
    const uint32_t sat = nf > 0xffffffffull ? 0xffffffffu : (uint32_t)nf;
    CHECK(o.sel_frames[r.n] == sat && o.sel_samples[r.n] == ns);
    CHECK(o.status[0] == ((nf > o.sel_cap ? BNF_SEL_OVERFLOW : 0u) | (none ? BNF_SEL_NO_STREAM : 0u)) && o.status[1] == sat &&
          o.status[2] == nonempty && o.status[3] == clipped);
    for (uint64_t p = nf; p < o.sel_cap; p++) CHECK(is_filler(o.sel[p]));
}

int main() {
    /* 1. duplicates, overlaps, any order, streams nobody names, ids that name no stream */
    {
        Tables t;
        make(t, {12, 1, 0, 40, 7, 3, 1, 25});
        auto T = [&](uint32_t s) { return t.ss[s + 1] - t.ss[s]; };
        auto L = [&](uint32_t s, uint32_t k) { return t.info[t.sf[s] + k].out_sample - t.ss[s]; };
        std::vector<bnf_window_request> v = {
            {3, L(3, 10) + 1, L(3, 14) - L(3, 10)}, /* frames 10..14 of the 40-frame stream */
            {3, L(3, 12) - 1, L(3, 20) - L(3, 12)}, /* overlaps it */
            {3, L(3, 10) + 1, L(3, 14) - L(3, 10)}, /* the first one again */
            {7, 0, ~0ull},                          /* to the end */
            {0, L(0, 3), 5},                        /* lo on a frame start */
            {8, 0, 5},                              /* stream id == nstreams */
            {0, 0, L(0, 1)},                        /* hi on a frame start, stream 0 again and out of order */
            {0xffffffffull, 1, 1},                  /* 2^32 - 1 */
            {0x100000000ull, 0, ~0ull},             /* 2^32: the low word alone would name stream 0 */
            {1ull << 63, 3, 3},
            {~0ull, ~0ull, ~0ull},
            {2, 0, 10},                             /* a stream without frames */
            {6, T(6) - 1, 2},                       /* clipped by one */
            {4, T(4), 4},                           /* first_sample == T */
            {5, 5, ~0ull - 2},                      /* the sum wraps */
            {1, 0, 0},                              /* nsamples == 0 */
        };
        Requests r(v);
        Out full(r.n, 4 * t.cap);
        run(t, r, full);
        verify(t, r, full);
        CHECK(full.status[0] == BNF_SEL_NO_STREAM);
        const uint32_t total = full.status[1];
        for (uint32_t sel_cap : {total, total - 1, 0u}) { /* one short: nothing at sel_cap is written (the allocation ends there) */
            Out o(r.n, sel_cap);
            run(t, r, o);
            verify(t, r, o);
            CHECK((o.status[0] & BNF_SEL_OVERFLOW) == (sel_cap < total ? BNF_SEL_OVERFLOW : 0u));
        }
    }
    /* 2. window counts around the scan block over three streams, random requests; then no streams at all */
    for (uint32_t n : {0u, 1u, 1023u, 1024u, 1025u}) {
        Tables t;
        make(t, {5, 0, 3});
        std::vector<bnf_window_request> v(n);
        for (auto &q : v) {
            q.stream = rnd() % 4; /* 3: no such stream */
            const uint64_t T = q.stream < 3 ? t.ss[q.stream + 1] - t.ss[q.stream] : 9;
            q.first_sample = rnd() % (T + 3);
            q.nsamples = rnd() % (T + 3);
        }
        Requests r(v);
        Out o(n, 2 * n + 3);
        run(t, r, o);
        verify(t, r, o);
    }
    {
        Tables t;
        make(t, {});
        free(t.info); /* nstreams == 0: no record and no prefix may be read; the one-entry tables stay */
        t.info = nullptr;
        Requests r({{0, 0, 5}, {1, 2, 3}, {~0ull, ~0ull, ~0ull}});
        Out o(r.n, 2);
        run(t, r, o);
        verify(t, r, o);
        CHECK(o.status[0] == BNF_SEL_NO_STREAM && !o.status[1] && !o.status[2] && !o.status[3]);
    }
    /* 3. bad slices: a descending slice and one past cap.  Unnamed, they are not read and are no error
     *    (the tables' tail past the last named stream is not even allocated); named, nothing is selected. */
    {
        Tables t;
        make(t, {4, 6, 2, 5, 3});
        Requests good({{0, 0, ~0ull}, {0, 0, 1}, {9, 0, 1}, {0, 0, ~0ull}});
        {
            Tables cut; /* entries [0, 1] only: stream 0's slice */
            cut.nstreams = t.nstreams;
            cut.cap = t.cap;
            cut.info = (bnf_frame_info *)malloc(sizeof(bnf_frame_info) * t.sf[1]);
            memcpy(cut.info, t.info, sizeof(bnf_frame_info) * t.sf[1]);
            cut.sf = (uint32_t *)malloc(8);
            cut.ss = (uint64_t *)malloc(16);
            memcpy(cut.sf, t.sf, 8);
            memcpy(cut.ss, t.ss, 16);
            Out o(good.n, 16);
            run(cut, good, o);
            CHECK(o.status[0] == BNF_SEL_NO_STREAM && o.status[1] == 4 + 1 + 4 && o.status[2] == 3);
            CHECK(o.win[0].first_frame == 0 && o.win[0].nframes == 4 && o.win[3].nframes == 4 && o.win[2].flags == 6u);
        }
        for (int kind = 0; kind < 3; kind++) {
            Tables u;
            make(u, {4, 6, 2, 5, 3});
            if (kind == 0) u.sf[2] = u.sf[3] + 1;           /* stream 2's slice descends */
            if (kind == 1) u.cap = u.sf[4] - 1;             /* stream 3 passes cap, streams 0..2 do not */
            if (kind == 2) u.ss[4] = u.ss[3] - 1;           /* stream 3's samples descend */
            const uint64_t named = kind == 0 ? 2 : 3;
            Requests ok({{0, 0, ~0ull}, {kind == 0 ? 4ull : 1ull, 0, ~0ull}, {77, 0, 1}});
            Out o1(ok.n, 16);
            run(u, ok, o1);
            CHECK(o1.status[0] == BNF_SEL_NO_STREAM && o1.status[2] == 2);
            Requests bad({{0, 0, ~0ull}, {named, 0, ~0ull}, {77, 0, 1}});
            Out o(bad.n, 16);
            run(u, bad, o);
            CHECK(o.status[0] == (BNF_SEL_BAD_TABLES | BNF_SEL_NO_STREAM) && !o.status[1] && !o.status[2] && !o.status[3]);
            for (uint32_t w = 0; w <= bad.n; w++) CHECK(o.sel_frames[w] == 0 && o.sel_samples[w] == 0);
            CHECK(o.win[0].flags == BNF_WIN_EMPTY && o.win[0].first_frame == u.sf[0] && !o.win[0].nframes && !o.win[0].nsamples);
            CHECK(o.win[1].flags == BNF_WIN_EMPTY && o.win[1].first_frame == u.sf[named] && !o.win[1].pcm_first);
            CHECK(o.win[2].flags == (BNF_WIN_EMPTY | BNF_WIN_NO_STREAM) && o.win[2].first_frame == 0);
            for (uint32_t p = 0; p < 16; p++) CHECK(is_filler(o.sel[p]));
        }
    }
    /* 4. the saturating total: 65,537 whole-stream requests over one stream of 65,536 frames */
    {
        Tables t;
        make(t, {65536}, true);
        Requests r(std::vector<bnf_window_request>(65537, bnf_window_request{0, 0, 65536}));
        Out o(r.n, 8);
        run(t, r, o);
        verify(t, r, o);
        CHECK(o.status[0] == BNF_SEL_OVERFLOW && o.status[1] == 0xffffffffu && o.status[2] == 65537 && o.status[3] == 0);
        CHECK(o.sel_frames[65535] == 0xffff0000u && o.sel_frames[65536] == 0xffffffffu && o.sel_frames[65537] == 0xffffffffu);
        CHECK(o.sel_samples[65537] == 65537ull * 65536ull);
        for (uint32_t p = 0; p < 8; p++) CHECK(o.sel[p].out_sample == p && o.sel[p].crc8 == t.info[p].crc8);
    }
    /* 5. out_sample values no index wrote: the call returns and every window stays inside its stream */
    for (int round = 0; round < 200; round++) {
        Tables t;
        make(t, {9, 1, 30, 0, 5});
        for (uint32_t i = 0; i < t.cap; i++) {
            const uint64_t x = rnd();
            t.info[i].out_sample = round & 1 ? x : x % 20000; /* anywhere, or shuffled nearby */
            if (round & 2) t.info[i].blocksize = (uint32_t)rnd();
        }
        std::vector<bnf_window_request> v(24);
        for (auto &q : v) q = {rnd() % 6, rnd() % 9000, round & 4 ? ~0ull : rnd() % 9000};
        Requests r(v);
        Out o(r.n, 24 * 30);
        run(t, r, o);
        for (uint32_t w = 0; w < r.n; w++) {
            const bnf_window &win = o.win[w];
            const uint64_t s = v[w].stream;
            if (s >= t.nstreams) {
                CHECK(win.flags == (BNF_WIN_EMPTY | BNF_WIN_NO_STREAM) && !win.nframes);
                continue;
            }
            CHECK(win.first_frame >= t.sf[s] && win.first_frame <= t.sf[s + 1] && win.nframes <= t.sf[s + 1] - win.first_frame);
            CHECK(o.sel_frames[w + 1] - o.sel_frames[w] == win.nframes);
        }
        CHECK(!(o.status[0] & (BNF_SEL_OVERFLOW | BNF_SEL_BAD_TABLES)) && o.status[1] <= 24 * 30);
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    puts("select_windows_sanitize: ok");
    return 0;
}
