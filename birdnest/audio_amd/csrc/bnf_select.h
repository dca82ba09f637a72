/*
 * bnf_select.h -- the rule of bnflac_select_ranges: which frames of a stream a sample window
 * needs, and what the window looks like in the compact PCM those frames decode into.  One
 * function over the index's tables, callable from host and device: k_sel_streams
 * (bnflac_select.hip, one lane per stream) and bnflac_select_ranges_host (bnflac_runtime.cpp)
 * are the same code, as bnf_metadata.h is for the scan.  The header needs no HIP: a plain C++
 * compiler takes it too (tools/select_ranges_sanitize.cpp builds it with the sanitizers).
 * bnflac_select_windows applies the same rule per window request, each naming its stream
 * (bnf_select_request below: k_win_select, bnflac_select_windows_host and
 * tools/select_windows_sanitize.cpp).  bnflac_select_windows_shared takes the same requests and
 * selects the union of their frames, each once (bnf_select_windows_shared_host below: k_shr_*,
 * bnflac_select_windows_shared_host and tools/select_shared_sanitize.cpp).
 *
 * Stream s, T = its samples, frame i of [f0, f1) at local start L_i = out_sample_i - s0 with
 * blocksize b_i:  lo = min(first_sample, T), hi = min(lo + nsamples, T) (saturating);
 * hi == lo: empty.  Else the frames with L_i < hi and L_i + b_i > lo, found by two binary
 * searches: a = the first frame with L_i + b_i > lo, b = the first frame of [a, f1) with
 * L_i >= hi.  Both predicates are monotone over the tables bnflac_index_streams writes (L_i
 * ascends, the frames tile [0, T)), so [a, b) is the contiguous run the rule names.  Over any
 * other contents the searches still halve an interval of [f0, f1): at most 32 steps each, every
 * index read inside the stream's range, and a run that comes out empty is an empty window.  All
 * sample arithmetic is modulo 2^64, so such contents give some window, never a fault.
 */
#ifndef BNF_SELECT_H
#define BNF_SELECT_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BNF_SEL_HD __host__ __device__
#else
#define BNF_SEL_HD
#endif

#include "bnflac_device.h"

/* == bnflac_sample_range, bnflac_window (include/bnflac.h) */
typedef struct {
    uint64_t first_sample, nsamples;
} bnf_sample_range;

typedef struct {
    uint64_t pcm_first;
    uint64_t nsamples;
    uint32_t skip, first_frame, nframes, flags;
} bnf_window;

/* == bnflac_window_request */
typedef struct {
    uint64_t stream, first_sample, nsamples;
} bnf_window_request;

enum { BNF_WIN_CLIPPED = 1u, BNF_WIN_EMPTY = 2u, BNF_WIN_NO_STREAM = 4u };           /* bnf_window.flags */
enum { BNF_SEL_OVERFLOW = 1u, BNF_SEL_BAD_TABLES = 2u, BNF_SEL_NO_STREAM = 4u };    /* status word 0 */

/* One stream's selection before the prefixes over the streams are known. */
typedef struct {
    uint64_t nsamples; /* of the window, clipped */
    uint64_t hull;     /* samples of the selected frames: the stream's share of the compact PCM */
    uint32_t skip, first_frame, nframes, flags;
} bnf_sel_stream;

BNF_SEL_HD inline uint64_t bnf_sel_sat_add(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;
    return s < a ? ~(uint64_t)0 : s;
}

/* Stream s's slice of the index's tables can be searched: ascending, and nothing at or past cap. */
BNF_SEL_HD inline bool bnf_select_tables_ok(uint32_t f0, uint32_t f1, uint64_t s0, uint64_t s1, uint32_t cap) {
    return f0 <= f1 && f1 <= cap && s0 <= s1;
}

/* The rule for one stream whose tables are ok: frames [f0, f1) of info, samples [s0, s1). */
BNF_SEL_HD inline void bnf_select_stream(const bnf_frame_info *info, uint32_t f0, uint32_t f1, uint64_t s0, uint64_t s1,
                                         bnf_sample_range r, bnf_sel_stream &o) {
    const uint64_t T = s1 - s0;
    const uint64_t lo = r.first_sample < T ? r.first_sample : T;
    const uint64_t end = bnf_sel_sat_add(lo, r.nsamples);
    const uint64_t hi = end < T ? end : T;
    o.nsamples = o.hull = 0;
    o.skip = 0;
    o.first_frame = f0;
    o.nframes = 0;
    o.flags = bnf_sel_sat_add(r.first_sample, r.nsamples) > T ? BNF_WIN_CLIPPED : 0u;
    if (hi == lo) {
        o.flags |= BNF_WIN_EMPTY;
        return;
    }
    uint32_t a = f0, n = f1 - f0; /* the first frame with L_i + b_i > lo */
    while (n) {
        const uint32_t h = n >> 1, m = a + h;
        if (info[m].out_sample - s0 + info[m].blocksize > lo) {
            n = h;
        } else {
            a = m + 1;
            n -= h + 1;
        }
    }
    uint32_t b = a; /* the first frame of [a, f1) with L_i >= hi */
    n = f1 - a;
    while (n) {
        const uint32_t h = n >> 1, m = b + h;
        if (info[m].out_sample - s0 >= hi) {
            n = h;
        } else {
            b = m + 1;
            n -= h + 1;
        }
    }
    if (b == a) { /* only over tables the index did not write */
        o.flags |= BNF_WIN_EMPTY;
        return;
    }
    const uint64_t first = info[a].out_sample;
    o.nsamples = hi - lo;
    o.hull = info[b - 1].out_sample + info[b - 1].blocksize - first;
    o.skip = (uint32_t)(lo - (first - s0));
    o.first_frame = a;
    o.nframes = b - a;
}

/* The window record of stream s once its prefix in the compact PCM is known. */
BNF_SEL_HD inline bnf_window bnf_select_window(const bnf_sel_stream &o, uint64_t sel_samples) {
    bnf_window w;
    w.pcm_first = sel_samples + o.skip;
    w.nsamples = o.nsamples;
    w.skip = o.skip;
    w.first_frame = o.first_frame;
    w.nframes = o.nframes;
    w.flags = o.flags;
    return w;
}

/* The window of every stream when the tables are unusable. */
BNF_SEL_HD inline bnf_window bnf_select_no_window(uint32_t f0) {
    bnf_window w;
    w.pcm_first = w.nsamples = 0;
    w.skip = 0;
    w.first_frame = f0;
    w.nframes = 0;
    w.flags = BNF_WIN_EMPTY;
    return w;
}

/* ---- bnflac_select_windows: the same rule per window request, each naming its stream */
enum { BNF_REQ_OK = 0, BNF_REQ_NO_STREAM = 1, BNF_REQ_BAD_SLICE = 2 };

/* The window of a request when nothing is selected for it: a stream it does not name leaves
 * first_frame 0 and no table entry read, else bnf_select_no_window of its stream. */
BNF_SEL_HD inline bnf_window bnf_select_no_request(const uint32_t *stream_frames, uint32_t nstreams, uint64_t stream) {
    bnf_window w = bnf_select_no_window(stream < nstreams ? stream_frames[stream] : 0u);
    if (stream >= nstreams) w.flags |= BNF_WIN_NO_STREAM;
    return w;
}

/* The rule for one request: bnf_select_stream over the slice of the stream it names.  A request
 * that names no stream, or a slice that cannot be searched, reads nothing more and leaves o empty. */
BNF_SEL_HD inline uint32_t bnf_select_request(const bnf_frame_info *info, uint32_t cap, const uint32_t *stream_frames,
                                              const uint64_t *stream_samples, uint32_t nstreams, bnf_window_request q,
                                              bnf_sel_stream &o) {
    o.nsamples = o.hull = 0;
    o.skip = o.first_frame = o.nframes = 0;
    o.flags = BNF_WIN_EMPTY;
    if (q.stream >= nstreams) {
        o.flags |= BNF_WIN_NO_STREAM;
        return BNF_REQ_NO_STREAM;
    }
    const uint32_t f0 = stream_frames[q.stream], f1 = stream_frames[q.stream + 1];
    const uint64_t s0 = stream_samples[q.stream], s1 = stream_samples[q.stream + 1];
    o.first_frame = f0;
    if (!bnf_select_tables_ok(f0, f1, s0, s1, cap)) return BNF_REQ_BAD_SLICE;
    bnf_sample_range r;
    r.first_sample = q.first_sample;
    r.nsamples = q.nsamples;
    bnf_select_stream(info, f0, f1, s0, s1, r, o);
    return BNF_REQ_OK;
}

/* A frame prefix as the 32-bit tables hold it */
BNF_SEL_HD inline uint32_t bnf_sel_sat32(uint64_t frames) {
    return frames > 0xffffffffull ? 0xffffffffu : (uint32_t)frames;
}

/* The whole bnflac_select_windows call on host tables: what k_win_select / k_win_scan /
 * k_win_apply / k_sel_emit compute.  offsets and sel_offsets may be NULL. */
inline void bnf_select_windows_host(const uint64_t *offsets, const bnf_frame_info *info, uint32_t cap,
                                    const uint32_t *stream_frames, const uint64_t *stream_samples, uint32_t nstreams,
                                    const bnf_window_request *requests, uint32_t nwindows, uint64_t *sel_offsets,
                                    bnf_frame_info *sel_info, uint32_t sel_cap, uint32_t *sel_frames, uint64_t *sel_samples,
                                    bnf_window *windows, uint32_t status[4]) {
    bool bad = false, no_stream = false;
    for (uint32_t w = 0; w < nwindows; w++) { /* only the slices some request names are judged */
        const uint64_t t = requests[w].stream;
        if (t >= nstreams)
            no_stream = true;
        else
            bad = bad || !bnf_select_tables_ok(stream_frames[t], stream_frames[t + 1], stream_samples[t], stream_samples[t + 1], cap);
    }
    uint64_t nf = 0, ns = 0; /* the frame total is not bounded by cap: windows may share frames */
    uint32_t nonempty = 0, clipped = 0;
    for (uint32_t w = 0; w < nwindows; w++) {
        sel_frames[w] = bnf_sel_sat32(nf);
        sel_samples[w] = ns;
        if (bad) {
            windows[w] = bnf_select_no_request(stream_frames, nstreams, requests[w].stream);
            continue;
        }
        bnf_sel_stream o;
        bnf_select_request(info, cap, stream_frames, stream_samples, nstreams, requests[w], o);
        windows[w] = bnf_select_window(o, ns);
        const uint64_t first = o.nframes ? info[o.first_frame].out_sample : 0;
        for (uint32_t k = 0; k < o.nframes; k++) {
            const uint64_t p = nf + k;
            if (p >= sel_cap) break;
            sel_info[p] = info[o.first_frame + k];
            sel_info[p].out_sample = ns + (info[o.first_frame + k].out_sample - first);
            if (sel_offsets) sel_offsets[p] = offsets ? offsets[o.first_frame + k] : 0;
        }
        nf += o.nframes;
        ns += o.hull;
        nonempty += (o.flags & BNF_WIN_EMPTY) ? 0u : 1u;
        clipped += (o.flags & BNF_WIN_CLIPPED) ? 1u : 0u;
    }
    sel_frames[nwindows] = bnf_sel_sat32(nf);
    sel_samples[nwindows] = ns;
    for (uint64_t p = nf; p < sel_cap; p++) { /* filler: zeros, skipped, no error */
        memset(&sel_info[p], 0, sizeof sel_info[p]);
        sel_info[p].status = BNF_ST_SKIPPED;
        sel_info[p].err = -1;
        if (sel_offsets) sel_offsets[p] = 0;
    }
    status[0] = (bad ? BNF_SEL_BAD_TABLES : nf > sel_cap ? BNF_SEL_OVERFLOW : 0u) | (no_stream ? BNF_SEL_NO_STREAM : 0u);
    status[1] = bnf_sel_sat32(nf);
    status[2] = nonempty;
    status[3] = clipped;
}

/* ---- bnflac_select_windows_shared: the requests of bnflac_select_windows, every frame selected once.
 * Per window the rule is bnf_select_request's, unchanged.  M = the index positions some window's run
 * [a_w, a_w + n_w) covers; in ascending position order, rank_i = the members of M below i and pos_i =
 * the sum of their blocksizes (modulo 2^64).  Record rank_i is info[i] with out_sample = pos_i, and a
 * window that is not empty starts at pos_{a_w} + skip_w of the shared compact PCM.  Over tables
 * bnflac_index_streams wrote, a stream's frames tile it, so a run is contiguous in rank and in pos with
 * the spacing out_sample had, and a window read through its record is what bnflac_select_windows'
 * own copy yields.  M is found with a difference array over the positions: +1 at a_w, -1 at
 * a_w + n_w (at most cap: the array has cap + 1 entries), a position is covered while the running sum
 * is positive.  Every trip count is nwindows, cap or sel_cap. */

/* The window of a request before the shared positions are known: pcm_first holds skip (0 when empty). */
BNF_SEL_HD inline bnf_window bnf_select_shared_window(const bnf_sel_stream &o) { return bnf_select_window(o, 0); }

/* The whole bnflac_select_windows_shared call on host tables: what the k_shr_* kernels compute.
 * offsets, sel_offsets and win_sel_first may be NULL.  false: out of memory, nothing written. */
inline bool bnf_select_windows_shared_host(const uint64_t *offsets, const bnf_frame_info *info, uint32_t cap,
                                           const uint32_t *stream_frames, const uint64_t *stream_samples,
                                           uint32_t nstreams, const bnf_window_request *requests, uint32_t nwindows,
                                           uint64_t *sel_offsets, bnf_frame_info *sel_info, uint32_t sel_cap,
                                           bnf_window *windows, uint32_t *win_sel_first, uint64_t totals[2],
                                           uint32_t status[4]) {
    bool bad = false, no_stream = false;
    for (uint32_t w = 0; w < nwindows; w++) { /* only the slices some request names are judged */
        const uint64_t t = requests[w].stream;
        if (t >= nstreams)
            no_stream = true;
        else
            bad = bad || !bnf_select_tables_ok(stream_frames[t], stream_frames[t + 1], stream_samples[t], stream_samples[t + 1], cap);
    }
    const uint32_t npos = nwindows && !bad ? cap : 0u;
    int32_t *delta = (int32_t *)calloc((size_t)npos + 1, sizeof(int32_t)); /* the difference array, its end slot included */
    uint32_t *rank = (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)npos + 1));
    uint64_t *pos = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)npos + 1));
    if (!delta || !rank || !pos) {
        free(delta);
        free(rank);
        free(pos);
        return false;
    }
    uint32_t nonempty = 0, clipped = 0, high = 0; /* high: one past the last position a window covers */
    for (uint32_t w = 0; w < nwindows; w++) {
        if (bad) {
            windows[w] = bnf_select_no_request(stream_frames, nstreams, requests[w].stream);
            continue;
        }
        bnf_sel_stream o;
        bnf_select_request(info, cap, stream_frames, stream_samples, nstreams, requests[w], o);
        windows[w] = bnf_select_shared_window(o);
        if (o.nframes) {
            delta[o.first_frame] += 1;
            delta[o.first_frame + o.nframes] -= 1;
            if (o.first_frame + o.nframes > high) high = o.first_frame + o.nframes;
        }
        nonempty += (o.flags & BNF_WIN_EMPTY) ? 0u : 1u;
        clipped += (o.flags & BNF_WIN_CLIPPED) ? 1u : 0u;
    }
    uint32_t nf = 0; /* at most cap */
    uint64_t ns = 0;
    int32_t cover = 0;
    for (uint32_t i = 0; i < high; i++) { /* info is read at covered positions only */
        cover += delta[i];
        if (cover <= 0) continue;
        rank[i] = nf;
        pos[i] = ns;
        if (nf < sel_cap) {
            sel_info[nf] = info[i];
            sel_info[nf].out_sample = ns;
            if (sel_offsets) sel_offsets[nf] = offsets ? offsets[i] : 0;
        }
        nf++;
        ns += info[i].blocksize;
    }
    for (uint32_t w = 0; w < nwindows; w++) {
        const bool some = !bad && windows[w].nframes != 0;
        if (some) windows[w].pcm_first += pos[windows[w].first_frame];
        if (win_sel_first) win_sel_first[w] = some ? rank[windows[w].first_frame] : 0u;
    }
    for (uint32_t p = nf; p < sel_cap; p++) { /* filler: zeros, skipped, no error */
        memset(&sel_info[p], 0, sizeof sel_info[p]);
        sel_info[p].status = BNF_ST_SKIPPED;
        sel_info[p].err = -1;
        if (sel_offsets) sel_offsets[p] = 0;
    }
    totals[0] = nf;
    totals[1] = ns;
    status[0] = (bad ? BNF_SEL_BAD_TABLES : nf > sel_cap ? BNF_SEL_OVERFLOW : 0u) | (no_stream ? BNF_SEL_NO_STREAM : 0u);
    status[1] = nf;
    status[2] = nonempty;
    status[3] = clipped;
    free(delta);
    free(rank);
    free(pos);
    return true;
}

/* The whole bnflac_select_ranges call on host tables: what the k_sel_* kernels of bnflac_select.hip
 * compute.  offsets and sel_offsets may be NULL. */
inline void bnf_select_ranges_host(const uint64_t *offsets, const bnf_frame_info *info, uint32_t cap,
                                   const uint32_t *stream_frames, const uint64_t *stream_samples, uint32_t nstreams,
                                   const bnf_sample_range *ranges, uint64_t *sel_offsets, bnf_frame_info *sel_info,
                                   uint32_t sel_cap, uint32_t *sel_frames, uint64_t *sel_samples, bnf_window *windows,
                                   uint32_t status[4]) {
    bool bad = false;
    for (uint32_t s = 0; s < nstreams; s++)
        bad = bad || !bnf_select_tables_ok(stream_frames[s], stream_frames[s + 1], stream_samples[s], stream_samples[s + 1], cap);
    uint32_t nf = 0, nonempty = 0, clipped = 0;
    uint64_t ns = 0;
    for (uint32_t s = 0; s < nstreams; s++) {
        sel_frames[s] = nf;
        sel_samples[s] = ns;
        if (bad) {
            windows[s] = bnf_select_no_window(stream_frames[s]);
            continue;
        }
        bnf_sel_stream o;
        bnf_select_stream(info, stream_frames[s], stream_frames[s + 1], stream_samples[s], stream_samples[s + 1], ranges[s], o);
        windows[s] = bnf_select_window(o, ns);
        const uint64_t first = o.nframes ? info[o.first_frame].out_sample : 0;
        for (uint32_t k = 0; k < o.nframes; k++) {
            const uint64_t p = (uint64_t)nf + k;
            if (p >= sel_cap) break;
            sel_info[p] = info[o.first_frame + k];
            sel_info[p].out_sample = ns + (info[o.first_frame + k].out_sample - first);
            if (sel_offsets) sel_offsets[p] = offsets ? offsets[o.first_frame + k] : 0;
        }
        nf += o.nframes;
        ns += o.hull;
        nonempty += (o.flags & BNF_WIN_EMPTY) ? 0u : 1u;
        clipped += (o.flags & BNF_WIN_CLIPPED) ? 1u : 0u;
    }
    sel_frames[nstreams] = nf;
    sel_samples[nstreams] = ns;
    for (uint32_t p = nf; p < sel_cap; p++) { /* filler: zeros, skipped, no error */
        memset(&sel_info[p], 0, sizeof sel_info[p]);
        sel_info[p].status = BNF_ST_SKIPPED;
        sel_info[p].err = -1;
        if (sel_offsets) sel_offsets[p] = 0;
    }
    status[0] = bad ? BNF_SEL_BAD_TABLES : nf > sel_cap ? BNF_SEL_OVERFLOW : 0u;
    status[1] = nf;
    status[2] = nonempty;
    status[3] = clipped;
}

#endif
