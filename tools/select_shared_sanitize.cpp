/*
 * select_shared_sanitize.cpp -- the host rule of bnflac_select_windows_shared (csrc/bnf_select.h)
 * under AddressSanitizer and UBSan.  A stand-alone program: every table is a heap allocation of
 * exactly the size the contract names (cap records, nstreams + 1 prefixes, nwindows requests, windows
 * and first ranks, sel_cap records, two totals), and the rule's own difference array has exactly
 * cap + 1 entries, so a read at cap, a table entry read for a request that names no stream, a mark
 * behind the end slot delta[cap] or a write at sel_cap is a sanitizer report.  Each case over
 * consistent tables is also checked against the union written out position by position (a mark per
 * position, no difference array, no binary search).  Exit 0: no report, no mismatch.
 *
 *   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I birdnest/audio_amd/csrc tools/select_shared_sanitize.cpp -o select_shared_sanitize
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

/* streams of the given frame counts, records of random bytes; blocksizes 1..4608 with a short last frame */
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
    bnf_window *win;
    uint32_t *first;
    uint64_t *totals;
    uint32_t status[4];
    Out(uint32_t nwindows, uint32_t cap) : sel_cap(cap) {
        sel = (bnf_frame_info *)malloc(sizeof(bnf_frame_info) * (cap ? cap : 1));
        win = (bnf_window *)malloc(sizeof(bnf_window) * (nwindows ? nwindows : 1));
        first = (uint32_t *)malloc(4 * (nwindows ? nwindows : 1));
        totals = (uint64_t *)malloc(16);
    }
    ~Out() {
        free(sel);
        free(win);
        free(first);
        free(totals);
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
    CHECK(bnf_select_windows_shared_host(nullptr, t.info, t.cap, t.sf, t.ss, t.nstreams, r.q, r.n, nullptr, o.sel, o.sel_cap,
                                         o.win, o.first, o.totals, o.status));
}

static bool is_filler(const bnf_frame_info &x) {
    bnf_frame_info filler;
    memset(&filler, 0, sizeof filler);
    filler.status = BNF_ST_SKIPPED;
    filler.err = -1;
    return !memcmp(&filler, &x, sizeof filler);
}

/* the rule frame by frame per request and the union position by position, against a finished call
 * whose named slices are consistent */
static void verify(const Tables &t, const Requests &r, const Out &o) {
    std::vector<uint8_t> mark(t.cap + 1u, 0);
    std::vector<uint32_t> a_of(r.n, 0), n_of(r.n, 0);
    uint32_t nonempty = 0, clipped = 0;
    bool none = false;
    for (uint32_t w = 0; w < r.n; w++) {
        const bnf_window &win = o.win[w];
        const uint64_t s = r.q[w].stream, first = r.q[w].first_sample, want = r.q[w].nsamples;
        if (s >= t.nstreams) {
            none = true;
            CHECK(win.flags == (BNF_WIN_EMPTY | BNF_WIN_NO_STREAM) && !win.first_frame && !win.nframes && !win.skip &&
                  !win.nsamples && !win.pcm_first && !o.first[w]);
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
            CHECK((win.flags & BNF_WIN_EMPTY) && win.nframes == 0 && win.skip == 0 && win.nsamples == 0 && win.pcm_first == 0 &&
                  win.first_frame == t.sf[s] && o.first[w] == 0);
            continue;
        }
        const uint64_t La = t.info[a].out_sample - t.ss[s];
        CHECK(!(win.flags & BNF_WIN_EMPTY) && win.first_frame == a && win.nframes == b - a && win.skip == lo - La &&
              win.nsamples == hi - lo && win.skip < t.info[a].blocksize);
        for (uint32_t i = a; i < b; i++) mark[i] = 1;
        a_of[w] = a;
        n_of[w] = b - a;
        nonempty++;
    }
    std::vector<uint32_t> rank(t.cap + 1u, 0);
    std::vector<uint64_t> pos(t.cap + 1u, 0);
    uint32_t nf = 0;
    uint64_t ns = 0;
    for (uint32_t i = 0; i < t.cap; i++) {
        if (!mark[i]) continue;
        rank[i] = nf;
        pos[i] = ns;
        if (nf < o.sel_cap) {
            bnf_frame_info x = t.info[i];
            x.out_sample = ns;
            CHECK(!memcmp(&x, &o.sel[nf], sizeof x));
        }
        nf++;
        ns += t.info[i].blocksize;
    }
    for (uint32_t w = 0; w < r.n; w++) {
        if (!n_of[w]) continue;
        CHECK(o.first[w] == rank[a_of[w]] && o.win[w].pcm_first == pos[a_of[w]] + o.win[w].skip);
        /* the frames tile their stream: the window's records are consecutive, spaced as out_sample was */
        for (uint32_t k = 0; k < n_of[w] && o.first[w] + k < o.sel_cap; k++)
            CHECK(o.sel[o.first[w] + k].out_sample - pos[a_of[w]] == t.info[a_of[w] + k].out_sample - t.info[a_of[w]].out_sample);
    }
    CHECK(o.totals[0] == nf && o.totals[1] == ns);
    CHECK(o.status[0] == ((nf > o.sel_cap ? BNF_SEL_OVERFLOW : 0u) | (none ? BNF_SEL_NO_STREAM : 0u)) && o.status[1] == nf &&
          o.status[2] == nonempty && o.status[3] == clipped);
    for (uint64_t p = nf; p < o.sel_cap; p++) CHECK(is_filler(o.sel[p]));
}

/* windows of `window` samples every `hop` over every whole stream */
static std::vector<bnf_window_request> sliding(const Tables &t, uint64_t window, uint64_t hop) {
    std::vector<bnf_window_request> v;
    for (uint32_t s = 0; s < t.nstreams; s++) {
        const uint64_t T = t.ss[s + 1] - t.ss[s];
        for (uint64_t first = 0; first < (T ? T : 1); first += hop) v.push_back({s, first, window});
    }
    return v;
}

int main() {
    /* 1. sliding windows at a third of the window over streams of 0, 1 and many frames, in order,
     *    reversed and with duplicates and ids that name no stream; sel_cap exact, one short and 0.
     *    The last stream's last window ends in the index's last frame: its -1 goes to delta[cap]. */
    {
        Tables t;
        make(t, {12, 1, 0, 40, 7, 3, 1, 25});
        std::vector<bnf_window_request> v = sliding(t, 3000, 1000);
        CHECK(v.back().stream == 7);
        std::vector<bnf_window_request> rev(v.rbegin(), v.rend());
        std::vector<bnf_window_request> dup = v;
        for (size_t i = 0; i < v.size(); i += 5) dup.push_back(v[i]);
        dup.insert(dup.begin() + 3, {8, 0, 5});            /* stream id == nstreams */
        dup.push_back({0x100000000ull, 0, ~0ull});         /* 2^32: the low word alone would name stream 0 */
        dup.push_back({~0ull, ~0ull, ~0ull});
        for (const auto &set : {v, rev, dup}) {
            Requests r(set);
            Out full(r.n, t.cap + 5);
            run(t, r, full);
            verify(t, r, full);
            CHECK(full.totals[0] == t.cap && full.totals[1] == t.ss[t.nstreams]); /* every frame once */
            const uint32_t total = full.status[1];
            for (uint32_t sel_cap : {total, total - 1, 0u}) { /* nothing at sel_cap is written: the allocation ends there */
                Out o(r.n, sel_cap);
                run(t, r, o);
                verify(t, r, o);
                CHECK((o.status[0] & BNF_SEL_OVERFLOW) == (sel_cap < total ? BNF_SEL_OVERFLOW : 0u));
                for (uint32_t w = 0; w < r.n; w++) CHECK(!memcmp(&o.win[w], &full.win[w], sizeof(bnf_window)) && o.first[w] == full.first[w]);
            }
        }
        /* a single window on the very last frame: delta[cap - 1] and delta[cap] are the only marks */
        Requests last({{7, t.ss[8] - t.ss[7] - 1, 1}});
        Out o(1, 1);
        run(t, last, o);
        verify(t, last, o);
        CHECK(o.win[0].first_frame == t.cap - 1 && o.win[0].nframes == 1 && o.totals[0] == 1);
        /* win_sel_first may be NULL */
        uint32_t st[4];
        CHECK(bnf_select_windows_shared_host(nullptr, t.info, t.cap, t.sf, t.ss, t.nstreams, last.q, 1, nullptr, o.sel, 1, o.win,
                                             nullptr, o.totals, st) && st[1] == 1);
    }
    /* 2. random overlapping requests, window counts around the scan block; then none at all, no streams at all */
    for (uint32_t n : {0u, 1u, 1023u, 1024u, 1025u, 2049u}) {
        Tables t;
        make(t, {5, 0, 3, 9});
        std::vector<bnf_window_request> v(n);
        for (auto &q : v) {
            q.stream = rnd() % 5; /* 4: no such stream */
            const uint64_t T = q.stream < 4 ? t.ss[q.stream + 1] - t.ss[q.stream] : 9;
            q.first_sample = rnd() % (T + 3);
            q.nsamples = rnd() % (T + 3);
        }
        Requests r(v);
        Out o(n, t.cap);
        run(t, r, o);
        verify(t, r, o);
        if (!n) CHECK(!o.status[0] && !o.status[1] && !o.status[2] && !o.status[3] && !o.totals[0] && !o.totals[1]);
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
     *    (the tables' tail right behind the last named stream is not even allocated); named, nothing is
     *    selected. */
    {
        Tables t;
        make(t, {4, 6, 2, 5, 3});
        Requests good({{0, 0, ~0ull}, {0, 0, 1}, {9, 0, 1}, {0, 1, ~0ull}});
        {
            Tables cut; /* entries [0, 1] only: stream 0's slice, and cap records claimed while 4 exist */
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
            CHECK(o.status[0] == BNF_SEL_NO_STREAM && o.status[1] == 4 && o.status[2] == 3 && o.totals[0] == 4);
            CHECK(o.win[0].first_frame == 0 && o.win[0].nframes == 4 && o.win[1].nframes == 1 && o.win[2].flags == 6u);
            CHECK(o.first[0] == 0 && o.first[1] == 0 && o.first[2] == 0 && o.totals[1] == t.ss[1]);
            for (uint32_t p = 0; p < 4; p++) CHECK(o.sel[p].out_sample == t.info[p].out_sample && o.sel[p].crc8 == t.info[p].crc8);
            for (uint32_t p = 4; p < 16; p++) CHECK(is_filler(o.sel[p]));
        }
        for (int kind = 0; kind < 3; kind++) {
            Tables u;
            make(u, {4, 6, 2, 5, 3});
            if (kind == 0) u.sf[2] = u.sf[3] + 1;           /* stream 2's slice descends */
            if (kind == 1) u.cap = u.sf[4] - 1;             /* stream 3 passes cap, streams 0..2 do not */
            if (kind == 2) u.ss[4] = u.ss[3] - 1;           /* stream 3's samples descend */
            const uint64_t named = kind == 0 ? 2 : 3;
            Requests ok({{0, 0, ~0ull}, {kind == 0 ? 4ull : 1ull, 0, ~0ull}, {77, 0, 1}, {0, 5, 9}});
            Out o1(ok.n, 16);
            run(u, ok, o1);
            CHECK(o1.status[0] == BNF_SEL_NO_STREAM && o1.status[2] == 3);
            Requests bad({{0, 0, ~0ull}, {named, 0, ~0ull}, {77, 0, 1}, {0, 5, 9}});
            Out o(bad.n, 16);
            run(u, bad, o);
            CHECK(o.status[0] == (BNF_SEL_BAD_TABLES | BNF_SEL_NO_STREAM) && !o.status[1] && !o.status[2] && !o.status[3]);
            CHECK(!o.totals[0] && !o.totals[1]);
            for (uint32_t w = 0; w < bad.n; w++) CHECK(o.first[w] == 0 && !o.win[w].pcm_first && !o.win[w].nframes);
            CHECK(o.win[0].flags == BNF_WIN_EMPTY && o.win[0].first_frame == u.sf[0] && !o.win[0].nsamples);
            CHECK(o.win[1].flags == BNF_WIN_EMPTY && o.win[1].first_frame == u.sf[named]);
            CHECK(o.win[2].flags == (BNF_WIN_EMPTY | BNF_WIN_NO_STREAM) && o.win[2].first_frame == 0);
            for (uint32_t p = 0; p < 16; p++) CHECK(is_filler(o.sel[p]));
        }
    }
    /* 4. out_sample values no index wrote: the call returns, every window stays inside its stream, and the
     *    records are those of the positions the windows' runs cover, in position order */
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
        Out o(r.n, t.cap);
        run(t, r, o);
        std::vector<uint8_t> mark(t.cap + 1u, 0);
        for (uint32_t w = 0; w < r.n; w++) {
            const bnf_window &win = o.win[w];
            const uint64_t s = v[w].stream;
            if (s >= t.nstreams) {
                CHECK(win.flags == (BNF_WIN_EMPTY | BNF_WIN_NO_STREAM) && !win.nframes);
                continue;
            }
            CHECK(win.first_frame >= t.sf[s] && win.first_frame <= t.sf[s + 1] && win.nframes <= t.sf[s + 1] - win.first_frame);
            for (uint32_t k = 0; k < win.nframes; k++) mark[win.first_frame + k] = 1;
        }
        uint32_t nf = 0;
        uint64_t ns = 0;
        for (uint32_t i = 0; i < t.cap; i++) {
            if (!mark[i]) continue;
            CHECK(o.sel[nf].out_sample == ns && o.sel[nf].crc8 == t.info[i].crc8 && o.sel[nf].blocksize == t.info[i].blocksize);
            nf++;
            ns += t.info[i].blocksize;
        }
        CHECK(!(o.status[0] & (BNF_SEL_OVERFLOW | BNF_SEL_BAD_TABLES)) && o.status[1] == nf && o.totals[0] == nf && o.totals[1] == ns);
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    puts("select_shared_sanitize: ok");
    return 0;
}
