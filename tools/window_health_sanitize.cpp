/*
 * window_health_sanitize.cpp -- the host rule of bnflac_window_health (csrc/bnf_health.h) under
 * AddressSanitizer and UBSan.  A stand-alone program: every table is a heap allocation of exactly
 * the size the contract names (sel_cap records, nwindows windows, first positions, requests and
 * health records, nstreams descriptors, nstreams + 1 sample bounds, 4 status words), and the rule's
 * own prefixes have exactly sel_cap + 1 entries, so a record read at sel_cap, a table entry read for
 * a request that names no stream, a prefix read past sel_cap or a record written at nwindows is a
 * sanitizer report.  Every call is also checked against the rule written out with a loop over the
 * window's run, record by record.  Exit 0: no report, no mismatch.
 *
 *   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I birdnest/audio_amd/csrc tools/window_health_sanitize.cpp -o window_health_sanitize
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bnf_health.h"

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

/* an exact allocation of n entries (one byte when n is 0: a pointer that is not null and must not be read) */
template <class T>
struct Exact {
    uint32_t n;
    T *p;
    explicit Exact(uint32_t count) : n(count) { p = (T *)malloc(count ? sizeof(T) * (size_t)count : 1); }
    explicit Exact(const std::vector<T> &v) : Exact((uint32_t)v.size()) {
        if (n) memcpy(p, v.data(), sizeof(T) * n);
    }
    ~Exact() { free(p); }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
};

static bool is_bad(const bnf_frame_info &r) { return r.status != 0 || r.crc_ok == 0; }

/* the rule with a loop over the run, against a finished call */
static void verify(const Exact<bnf_frame_info> &sel, const Exact<bnf_window> &win, const Exact<uint32_t> &first,
                   const Exact<bnf_window_request> *req, const Exact<bnf_stream_desc> *sd, const Exact<uint64_t> *ss,
                   const Exact<bnf_window_health> &out, const uint32_t status[4]) {
    const uint32_t sel_cap = sel.n;
    uint32_t damaged = 0, brief = 0, unknown = 0;
    for (uint32_t w = 0; w < win.n; w++) {
        const bnf_window &W = win.p[w];
        const uint64_t f = first.p[w], n = W.nframes, end = f + n;
        const uint64_t lo = f < sel_cap ? f : sel_cap, hi = end < sel_cap ? end : sel_cap;
        uint32_t bad = 0, crc = 0;
        uint64_t A = 0, B = 0;
        for (uint64_t p = lo; p < hi; p++) {
            A += sel.p[p].blocksize;
            if (!is_bad(sel.p[p])) continue;
            bad++;
            crc += sel.p[p].status == 0;
            B += sel.p[p].blocksize;
        }
        const uint64_t head = n && f < sel_cap && is_bad(sel.p[f]) ? W.skip : 0;
        const uint64_t tail = n && end <= sel_cap && is_bad(sel.p[end - 1]) ? A - W.skip - W.nsamples : 0;
        uint32_t flags = (bad ? BNF_HEALTH_DAMAGED : 0u) | (n && end > sel_cap ? BNF_HEALTH_UNKNOWN : 0u) |
                         ((W.flags & 2u) ? BNF_HEALTH_EMPTY : 0u);
        uint64_t missing = 0;
        if (req) {
            const bnf_window_request &q = req->p[w];
            if (q.stream >= sd->n) {
                flags |= BNF_HEALTH_NO_STREAM;
            } else {
                const uint64_t total = sd->p[q.stream].total_samples, T = ss->p[q.stream + 1] - ss->p[q.stream];
                const uint64_t a = q.first_sample, b = a + q.nsamples < a ? ~0ull : a + q.nsamples;
                const uint64_t promised = (b < total ? b : total) - (a < total ? a : total);
                const uint64_t have = (b < T ? b : T) - (a < T ? a : T);
                if (total > T && promised > have) missing = promised - have;
                if (missing) flags |= BNF_HEALTH_SHORT;
            }
        }
        const bnf_window_health &h = out.p[w];
        CHECK(h.flags == flags && h.bad_frames == bad && h.crc_frames == crc && h.reserved == 0 &&
              h.bad_samples == B - head - tail && h.missing == missing);
        damaged += (flags & BNF_HEALTH_DAMAGED) != 0;
        brief += (flags & BNF_HEALTH_SHORT) != 0;
        unknown += (flags & BNF_HEALTH_UNKNOWN) != 0;
    }
    CHECK(status[0] == ((damaged ? 1u : 0u) | (brief ? 2u : 0u) | (unknown ? 4u : 0u)) && status[1] == damaged &&
          status[2] == brief && status[3] == unknown);
}

static void run(const Exact<bnf_frame_info> &sel, const Exact<bnf_window> &win, const Exact<uint32_t> &first,
                const Exact<bnf_window_request> *req, const Exact<bnf_stream_desc> *sd, const Exact<uint64_t> *ss) {
    Exact<bnf_window_health> out(win.n);
    Exact<uint32_t> status(4);
    CHECK(bnf_window_health_host(sel.p, sel.n, win.p, first.p, win.n, req ? req->p : nullptr, sd ? sd->p : nullptr,
                                 ss ? ss->p : nullptr, sd ? sd->n : 0u, out.p, status.p));
    verify(sel, win, first, req, sd, ss, out, status.p);
}

static void fill_records(Exact<bnf_frame_info> &sel, bool wide) {
    static const uint32_t st[] = {0, 0, 0, 0, 1, 2, 3, 0xffffffffu}, ok[] = {1, 1, 1, 0, 0xffffffffu};
    for (uint32_t p = 0; p < sel.n; p++) {
        uint8_t *b = (uint8_t *)&sel.p[p];
        for (size_t i = 0; i < sizeof(bnf_frame_info); i++) b[i] = (uint8_t)rnd();
        sel.p[p].status = st[rnd() % 8];
        sel.p[p].crc_ok = ok[rnd() % 5];
        sel.p[p].blocksize = wide ? (rnd() % 3 ? (uint32_t)rnd() : rnd() % 2 ? 0u : 0xffffffffu) : 1 + (uint32_t)(rnd() % 4608);
    }
}

int main() {
    /* 1. random runs around every edge of [0, sel_cap], with and without the request tables; sel_cap 0, 1 and
     *    sizes around nothing in particular: the host rule has no blocks */
    for (uint32_t sel_cap : {0u, 1u, 2u, 37u, 300u}) {
        for (int round = 0; round < 8; round++) {
            Exact<bnf_frame_info> sel(sel_cap);
            fill_records(sel, round & 1);
            const uint32_t k = round == 7 ? 0u : 200u;
            Exact<bnf_window> win(k);
            Exact<uint32_t> first(k);
            Exact<bnf_window_request> req(k);
            const uint32_t nstreams = round & 2 ? 5u : 0u;
            Exact<bnf_stream_desc> sd(nstreams);
            Exact<uint64_t> ss(nstreams + 1);
            ss.p[0] = rnd() % 1000;
            for (uint32_t s = 0; s < nstreams; s++) {
                ss.p[s + 1] = ss.p[s] + rnd() % 30000;
                const uint64_t T = ss.p[s + 1] - ss.p[s];
                const uint64_t totals[] = {0, T, T + 1 + rnd() % 30000, T / 2, ~0ull};
                sd.p[s] = {rnd(), rnd(), rnd(), totals[rnd() % 5]};
            }
            for (uint32_t w = 0; w < k; w++) {
                uint8_t *b = (uint8_t *)&win.p[w];
                for (size_t i = 0; i < sizeof(bnf_window); i++) b[i] = (uint8_t)rnd();
                win.p[w].nframes = (uint32_t)(rnd() % 12);
                first.p[w] = (uint32_t)(rnd() % (sel_cap + 3));
                if (w % 9 == 0) win.p[w].nframes = sel_cap - (first.p[w] < sel_cap ? first.p[w] : sel_cap); /* ends at sel_cap */
                if (w % 9 == 1) win.p[w].nframes = sel_cap + 1 - (first.p[w] < sel_cap ? first.p[w] : sel_cap); /* one past */
                if (w % 50 == 2) first.p[w] = win.p[w].nframes = 0xffffffffu;
                if (w % 50 == 3) first.p[w] = 0, win.p[w].nframes = sel_cap;
                if (!(round & 1)) win.p[w].skip = (uint32_t)(rnd() % 4608), win.p[w].nsamples = rnd() % 40000;
                const uint64_t wants[] = {0, 1, rnd() % 50000, ~0ull, ~0ull - 5};
                req.p[w] = {rnd() % (nstreams + 2), rnd() % 4 ? rnd() % 70000 : ~0ull - rnd() % 9, wants[rnd() % 5]};
                if (w % 50 == 4) req.p[w].stream = 0x100000000ull; /* the low word alone would name stream 0 */
            }
            run(sel, win, first, &req, &sd, &ss);
            run(sel, win, first, nullptr, nullptr, nullptr);
        }
    }
    /* 2. the geometry of a stream cut at its damage: frames of 4096, 6 of 12 kept, the sixth bad */
    {
        Exact<bnf_frame_info> sel(2);
        memset(sel.p, 0, sizeof(bnf_frame_info) * 2);
        sel.p[0].blocksize = sel.p[1].blocksize = 4096;
        sel.p[0].crc_ok = 1; /* record 1: status 0, crc_ok 0 */
        std::vector<bnf_window> wv = {{1616, 6000, 1616, 4, 2, 0}, {4096 + 1520, 2576, 1520, 5, 1, 1}, {0, 0, 0, 0, 0, 3}};
        std::vector<uint32_t> fv = {0, 1, 2};
        std::vector<bnf_window_request> rv = {{0, 18000, 6000}, {0, 22000, 6000}, {0, 30000, 6000}};
        Exact<bnf_window> win(wv);
        Exact<uint32_t> first(fv);
        Exact<bnf_window_request> req(rv);
        Exact<bnf_stream_desc> sd(1);
        sd.p[0] = {0, 0, 0, 49152};
        Exact<uint64_t> ss(2);
        ss.p[0] = 7, ss.p[1] = 7 + 24576;
        Exact<bnf_window_health> out(3);
        Exact<uint32_t> status(4);
        CHECK(bnf_window_health_host(sel.p, 2, win.p, first.p, 3, req.p, sd.p, ss.p, 1, out.p, status.p));
        verify(sel, win, first, &req, &sd, &ss, out, status.p);
        CHECK(out.p[0].flags == BNF_HEALTH_DAMAGED && out.p[0].bad_frames == 1 && out.p[0].crc_frames == 1 &&
              out.p[0].bad_samples == 3520 && out.p[0].missing == 0);
        CHECK(out.p[1].flags == (BNF_HEALTH_DAMAGED | BNF_HEALTH_SHORT) && out.p[1].bad_samples == 2576 && out.p[1].missing == 3424);
        CHECK(out.p[2].flags == (BNF_HEALTH_SHORT | BNF_HEALTH_EMPTY) && out.p[2].bad_samples == 0 && out.p[2].missing == 6000);
        CHECK(status.p[0] == 3 && status.p[1] == 2 && status.p[2] == 2 && status.p[3] == 0);
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    puts("window_health_sanitize: ok");
    return 0;
}
