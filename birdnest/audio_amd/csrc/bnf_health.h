/*
 * bnf_health.h -- the rule of bnflac_window_health: which windows of a decoded selection hold
 * damaged or missing audio.  One definition, callable from host and device, as bnf_select.h is
 * for the selections: k_hl_prefix / k_hl_windows (bnflac_health.hip), bnflac_window_health_host
 * (bnflac_runtime.cpp) and tools/window_health_sanitize.cpp are the same code.  The header needs
 * no HIP: a plain C++ compiler takes it too.
 *
 * A record is good iff status == 0 && crc_ok != 0, else bad; a bad record with status == 0 is a
 * crc record.  The rule reads status, crc_ok and blocksize of the records and nothing else.  It is
 * written over the exclusive prefixes P(p), p in [0, sel_cap], of the per-record terms
 * (bad, crc, blocksize, bad ? blocksize : 0): a window's run of records is two positions, so no
 * trip count is a table value.  Window w with W = windows[w], f = first[w], n = W.nframes:
 *   the run R = [min(f, sel_cap), min(f + n, sel_cap)), the sum in 64 bits;
 *   bad_frames, crc_frames, A = the blocksizes of R, B = those of R's bad records: P(end) - P(begin);
 *   head = W.skip if n > 0, f < sel_cap and record f is bad (P(f + 1) - P(f) counts one), else 0;
 *   tail = A - W.skip - W.nsamples if n > 0, f + n <= sel_cap and record f + n - 1 is bad, else 0;
 *   bad_samples = B - head - tail.  All sample arithmetic is modulo 2^64.
 *   UNKNOWN iff n > 0 and f + n > sel_cap, EMPTY = W.flags bit 1, DAMAGED iff bad_frames != 0.
 * With the request tables, t = requests[w].stream:  t >= nstreams: NO_STREAM, nothing read for t.
 *   Else total = streams[t].total_samples, T = stream_samples[t + 1] - stream_samples[t],
 *   lo = first_sample, hi = lo + nsamples (saturating), promised = min(hi, total) - min(lo, total),
 *   have = min(hi, T) - min(lo, T), missing = promised - have if total > T and promised > have,
 *   else 0; SHORT iff missing != 0.
 */
#ifndef BNF_HEALTH_H
#define BNF_HEALTH_H

#include "bnf_select.h"

/* == bnflac_window_health_rec */
typedef struct {
    uint32_t flags, bad_frames, crc_frames, reserved;
    uint64_t bad_samples, missing;
} bnf_window_health;

enum {
    BNF_HEALTH_DAMAGED = 1u,
    BNF_HEALTH_SHORT = 2u,
    BNF_HEALTH_UNKNOWN = 4u,
    BNF_HEALTH_EMPTY = 8u,
    BNF_HEALTH_NO_STREAM = 16u
}; /* bnf_window_health.flags; bits 0..2 are also the bits of status word 0 */

/* The terms of one record, or their sum over records [0, p).  counts: bad records in the low word, crc
 * records in the high one; each is at most sel_cap < 2^32, so the words never carry into each other and
 * the difference of two prefixes is the difference of each word. */
typedef struct {
    uint64_t counts, all, bad;
} bnf_health_sums;

BNF_SEL_HD inline bnf_health_sums bnf_health_terms(uint32_t status, uint32_t crc_ok, uint32_t blocksize) {
    const bool bad = status != BNF_ST_OK || crc_ok == 0;
    bnf_health_sums t;
    t.counts = bad ? (status == BNF_ST_OK ? 0x100000001ull : 1ull) : 0ull;
    t.all = blocksize;
    t.bad = bad ? blocksize : 0u;
    return t;
}

BNF_SEL_HD inline bnf_health_sums bnf_health_sub(const bnf_health_sums &a, const bnf_health_sums &b) {
    bnf_health_sums d;
    d.counts = a.counts - b.counts;
    d.all = a.all - b.all;
    d.bad = a.bad - b.bad;
    return d;
}

/* The records' part of the rule for one window.  prefix(p), p in [0, sel_cap], is P(p); it is called
 * for at most four positions, none above sel_cap.  Sets every field of h; missing is 0. */
template <class Prefix>
BNF_SEL_HD inline void bnf_health_window(const bnf_window &W, uint32_t f, uint32_t sel_cap, Prefix prefix,
                                         bnf_window_health &h) {
    const uint64_t end = (uint64_t)f + W.nframes; /* f = n = 2^32 - 1 does not wrap */
    const uint32_t lo = f < sel_cap ? f : sel_cap;
    const uint32_t hi = end < sel_cap ? (uint32_t)end : sel_cap;
    const bnf_health_sums p_lo = prefix(lo), p_hi = prefix(hi);
    const bnf_health_sums d = bnf_health_sub(p_hi, p_lo);
    uint64_t head = 0, tail = 0;
    if (W.nframes && f < sel_cap && (uint32_t)(prefix(f + 1u).counts - p_lo.counts) != 0u) head = W.skip;
    if (W.nframes && end <= sel_cap && (uint32_t)(p_hi.counts - prefix(hi - 1u).counts) != 0u)
        tail = d.all - W.skip - W.nsamples;
    h.bad_frames = (uint32_t)d.counts;
    h.crc_frames = (uint32_t)(d.counts >> 32);
    h.reserved = 0;
    h.bad_samples = d.bad - head - tail;
    h.missing = 0;
    h.flags = (h.bad_frames ? BNF_HEALTH_DAMAGED : 0u) | (W.nframes && end > sel_cap ? BNF_HEALTH_UNKNOWN : 0u) |
              ((W.flags & BNF_WIN_EMPTY) ? BNF_HEALTH_EMPTY : 0u);
}

/* The request's part: missing, SHORT and NO_STREAM.  No entry of streams or stream_samples is read for
 * a request that names no stream. */
BNF_SEL_HD inline void bnf_health_request(const bnf_window_request &q, const bnf_stream_desc *streams,
                                          const uint64_t *stream_samples, uint32_t nstreams, bnf_window_health &h) {
    if (q.stream >= nstreams) {
        h.flags |= BNF_HEALTH_NO_STREAM;
        return;
    }
    const uint64_t total = streams[q.stream].total_samples;
    const uint64_t T = stream_samples[q.stream + 1] - stream_samples[q.stream];
    const uint64_t lo = q.first_sample, hi = bnf_sel_sat_add(q.first_sample, q.nsamples);
    const uint64_t promised = (hi < total ? hi : total) - (lo < total ? lo : total);
    const uint64_t have = (hi < T ? hi : T) - (lo < T ? lo : T);
    if (total > T && promised > have) {
        h.missing = promised - have;
        h.flags |= BNF_HEALTH_SHORT;
    }
}

/* The whole bnflac_window_health call on host tables: what k_hl_prefix / k_hl_scan / k_hl_windows
 * compute.  requests, streams and stream_samples are all NULL or all given.  false: no memory for the
 * sel_cap + 1 prefixes, nothing written. */
inline bool bnf_window_health_host(const bnf_frame_info *sel_info, uint32_t sel_cap, const bnf_window *windows,
                                   const uint32_t *first, uint32_t nwindows, const bnf_window_request *requests,
                                   const bnf_stream_desc *streams, const uint64_t *stream_samples, uint32_t nstreams,
                                   bnf_window_health *health, uint32_t status[4]) {
    bnf_health_sums *pre = nullptr;
    if (nwindows) {
        pre = (bnf_health_sums *)malloc(sizeof(bnf_health_sums) * ((size_t)sel_cap + 1));
        if (!pre) return false;
        bnf_health_sums run = {0, 0, 0};
        for (uint32_t p = 0; p < sel_cap; p++) {
            pre[p] = run;
            const bnf_health_sums t = bnf_health_terms(sel_info[p].status, sel_info[p].crc_ok, sel_info[p].blocksize);
            run.counts += t.counts;
            run.all += t.all;
            run.bad += t.bad;
        }
        pre[sel_cap] = run;
    }
    uint32_t damaged = 0, brief = 0, unknown = 0;
    for (uint32_t w = 0; w < nwindows; w++) {
        bnf_window_health h;
        bnf_health_window(windows[w], first[w], sel_cap, [pre](uint32_t p) { return pre[p]; }, h);
        if (requests) bnf_health_request(requests[w], streams, stream_samples, nstreams, h);
        health[w] = h;
        damaged += (h.flags & BNF_HEALTH_DAMAGED) ? 1u : 0u;
        brief += (h.flags & BNF_HEALTH_SHORT) ? 1u : 0u;
        unknown += (h.flags & BNF_HEALTH_UNKNOWN) ? 1u : 0u;
    }
    free(pre);
    status[0] = (damaged ? BNF_HEALTH_DAMAGED : 0u) | (brief ? BNF_HEALTH_SHORT : 0u) | (unknown ? BNF_HEALTH_UNKNOWN : 0u);
    status[1] = damaged;
    status[2] = brief;
    status[3] = unknown;
    return true;
}

#endif
