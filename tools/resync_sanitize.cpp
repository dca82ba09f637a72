/*
 * resync_sanitize.cpp -- the host rule of bnflac_index_streams_resync (csrc/bnf_resync.h) under
 * AddressSanitizer and UBSan.  A stand-alone program: every table is a heap allocation of exactly
 * the size the contract names (ncand candidates, nstreams descriptors and resync records, nstreams + 1
 * prefix entries, cap slots, 4 status words), so a candidate read at ncand, a descriptor read for a
 * stream id outside the table, or a slot written at cap is a sanitizer report.  The tables are hostile
 * on purpose: successors and stream ids anywhere in int32, numbers up to 2^64, gaps of 2^40 frames.
 * Every call is also checked for what must hold whatever the input: the slots of a stream tile its
 * samples in position order, a placeholder names the frame behind its gap, the prefixes and the
 * status words agree with the slots.  Exit 0: no report, no mismatch.
 *
 *   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I birdnest/audio_amd/csrc tools/resync_sanitize.cpp -o resync_sanitize
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bnf_resync.h"

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

/* wild: successors, stream ids and numbers anywhere; else a plausible damaged corpus */
static void make_tables(bool wild, uint32_t B, std::vector<bnf_index_cand> &cands, std::vector<bnf_stream_desc> &streams) {
    const uint32_t nstreams = (uint32_t)(rnd() % 5);
    uint64_t off = 0;
    for (uint32_t s = 0; s < nstreams; s++) {
        bnf_stream_desc d;
        d.begin = off;
        d.first_offset = off + rnd() % 100;
        uint64_t num = rnd() % 3;
        const uint32_t nruns = (uint32_t)(rnd() % 5);
        for (uint32_t r = 0; r < nruns; r++) {
            const uint32_t len = 1 + (uint32_t)(rnd() % 6);
            for (uint32_t k = 0; k < len; k++) {
                bnf_index_cand c;
                c.offset = off + 10;
                c.flags = (rnd() % 10 ? BNF_CAND_VALID : 0u) | (rnd() % 3 ? 0u : BNF_CAND_SAMPLE_NUMBER);
                c.number = (c.flags & BNF_CAND_SAMPLE_NUMBER) ? num * B : num;
                c.succ = k + 1 < len ? (int32_t)cands.size() + 1 : -1;
                c.stream = (int32_t)s;
                c.blocksize = rnd() % 12 ? B : 1 + (uint32_t)(rnd() % B);
                if (wild && rnd() % 6 == 0) c.succ = (int32_t)(uint32_t)rnd();
                if (wild && rnd() % 8 == 0) c.stream = (int32_t)(uint32_t)rnd();
                if (wild && rnd() % 8 == 0) c.number = rnd();
                cands.push_back(c);
                off += 60;
                num++;
            }
            const uint64_t j = rnd() % 8;
            num += j < 3 ? 0 : j < 6 ? rnd() % 5 : j == 6 ? (1ull << 40) : (uint64_t)0 - rnd() % 3;
        }
        off += 50;
        d.end = off;
        d.total_samples = rnd() % 3 ? (rnd() % 40) * B + rnd() % B : 0;
        if (wild && rnd() % 4 == 0) d.total_samples = rnd();
        streams.push_back(d);
    }
}

static void run_case(bool wild) {
    const uint32_t Bs[] = {1, 2, 16, 256, 4608, 65535};
    const uint32_t B = Bs[rnd() % 6];
    std::vector<bnf_index_cand> vc;
    std::vector<bnf_stream_desc> vs;
    make_tables(wild, B, vc, vs);
    const Exact<bnf_index_cand> cands(vc);
    const Exact<bnf_stream_desc> streams(vs);
    const uint32_t cap = (uint32_t)(rnd() % 4 ? rnd() % 64 : 0);
    Exact<bnf_resync_slot> slots(cap);
    Exact<uint32_t> sf(streams.n + 1);
    Exact<uint64_t> ss(streams.n + 1);
    Exact<bnf_resync_rec> rec(streams.n);
    Exact<uint32_t> status(4);
    const bool with_slots = rnd() % 8 != 0, with_rec = rnd() % 8 != 0;
    CHECK(bnf_resync_plan_host(cands.p, cands.n, streams.p, streams.n, B, with_slots ? slots.p : nullptr, cap, sf.p, ss.p,
                               with_rec ? rec.p : nullptr, status.p));
    CHECK(sf.p[0] == 0 && ss.p[0] == 0 && status.p[1] == cands.n && status.p[2] == sf.p[streams.n]);
    CHECK(((status.p[0] & 2u) != 0) == (status.p[2] > cap) || status.p[2] == 0xFFFFFFFFu);
    CHECK((status.p[0] & ~(2u | 8u | 16u)) == 0);
    uint64_t gaps_seen = 0;
    bool all_written = status.p[2] <= cap && with_slots;
    for (uint32_t s = 0; s < streams.n; s++) {
        CHECK(sf.p[s] <= sf.p[s + 1]);
        if (!all_written) continue;
        /* the stream's slots tile [0, T) in position order */
        uint64_t at = 0;
        for (uint32_t q = sf.p[s]; q < sf.p[s + 1]; q++) {
            const bnf_resync_slot &x = slots.p[q];
            CHECK(x.cand < cands.n && cands.p[x.cand].stream == (int32_t)s); /* (a successor is taken as the table gives it) */
            CHECK(x.position == at && x.gap <= 1);
            at += x.gap ? B : cands.p[x.cand].blocksize;
            gaps_seen += x.gap;
            if (x.gap) CHECK(q + 1 < sf.p[s + 1] && slots.p[q + 1].cand == x.cand); /* the frame behind the gap follows */
            const bnf_stream_params sp = {1, B, B, 44100, 2, 16, 0};
            const bnf_frame_info r = bnf_rs_placeholder(cands.p[x.cand].offset, x.position, ss.p[s] + x.position, sp, B);
            CHECK(r.status == BNF_ST_ERROR && r.sub_start[0] == 1 && r.blocksize == B && r.flags == BNF_FL_GAP);
        }
        CHECK(ss.p[s + 1] - ss.p[s] == at);
        if (with_rec) {
            CHECK(rec.p[s].reserved == 0 && rec.p[s].gap_samples == (uint64_t)rec.p[s].gap_frames * B);
            if (sf.p[s + 1] == sf.p[s]) CHECK(rec.p[s].segments == 0 && rec.p[s].gap_frames == 0);
            if (rec.p[s].flags & BNF_RESYNC_HEAD) CHECK(sf.p[s + 1] == sf.p[s]);
        }
    }
    if (all_written) CHECK(gaps_seen == status.p[3]);
}

int main() {
    for (int k = 0; k < 20000; k++) run_case(k % 2 != 0);
    /* no streams, no candidates */
    {
        Exact<bnf_index_cand> cands(0);
        Exact<bnf_stream_desc> streams(0);
        Exact<uint32_t> sf(1), status(4);
        Exact<uint64_t> ss(1);
        CHECK(bnf_resync_plan_host(cands.p, 0, streams.p, 0, 16, nullptr, 0, sf.p, ss.p, nullptr, status.p));
        CHECK(sf.p[0] == 0 && ss.p[0] == 0 && status.p[0] == 0 && status.p[2] == 0);
    }
    if (failures) {
        fprintf(stderr, "resync_sanitize: %d failures\n", failures);
        return 1;
    }
    printf("resync_sanitize: ok\n");
    return 0;
}
