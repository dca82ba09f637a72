/*
 * bnf_resync.h -- the rule of bnflac_index_streams_resync: how a fixed-blocksize stream's frame
 * chain goes on past its damage, and which placeholder records keep its frames tiling its samples.
 * One definition, callable from host and device, as bnf_select.h and bnf_health.h are for theirs:
 * the k_rs_* kernels (bnflac_resync.hip), bnflac_resync_plan_host (bnflac_runtime.cpp) and
 * tools/resync_sanitize.cpp are the same code.  The header needs no HIP: a plain C++ compiler
 * takes it too.
 *
 * B is the stream blocksize (STREAMINFO min == max, >= 1).  The candidates of stream s are the
 * entries of the candidate table with stream == s, in table (= offset) order.  For candidate i:
 *   valid(i)   flags bit 0: it parsed as a frame start inside its stream;
 *   P(i)       number * B when the header codes a frame number (flags bit 1 clear), else number;
 *   succ(i)    the table's successor j -- the first later valid candidate of the stream at which the
 *              CRC-16 from i closes -- when P(j) == P(i) + blocksize(i), else none.  The CRC-16 of a
 *              run of zero bytes is zero, so a frame in front of zeroed frames closes at the next
 *              surviving frame start as well; the header numbers tell that link from a true one, and
 *              in an intact stream they always agree.  (On host tables a successor that does not
 *              point forward inside the stream is none too.)
 *   h          the head: the first valid candidate of s at or after first_offset;
 *   total      the descriptor's total_samples (0: unknown).
 * base = 0 when total != 0, else P(h).  The head is unusable when total != 0 and (P(h) % B != 0 or
 * P(h) >= total): no records, flag HEAD.
 * start_ok(j): valid(j), succ(j) exists, offset(j) >= first_offset, blocksize(j) == B, P(j) >= base,
 *   (P(j) - base) % B == 0, and total == 0 or P(j) < total.
 * Chain: x0 = h; x(k+1) = succ(xk) when it exists, else the first start_ok candidate of the stream
 *   after xk (a resync step), else the chain ends.
 * Positions: L(x0) = P(h) - base, and L(x0) / B placeholders stand in front of it at t * B.  Over a
 *   succ link L(x(k+1)) = E = L(xk) + blocksize(xk).  Over a resync step, with L' = P(x(k+1)) - base:
 *   L' < E or (L' - E) % B != 0 ends the chain before x(k+1) with flag CONTRADICTION; else
 *   L(x(k+1)) = L' and (L' - E) / B placeholders stand at E + t * B.
 * EOS: with total != 0 the first frame at or past total ends the chain before it (a placeholder
 *   always lies below the position of a frame that start_ok or the head test put below total).
 * T, the stream's length, is the end of the last kept record.  All arithmetic is modulo 2^64;
 * record counts are 64-bit and saturate to 32 bits where a table holds them.
 */
#ifndef BNF_RESYNC_H
#define BNF_RESYNC_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bnf_select.h"

/* == bnflac_index_cand */
typedef struct {
    uint64_t offset, number;
    int32_t succ, stream; /* -1: none */
    uint32_t blocksize, flags;
} bnf_index_cand;

enum { BNF_CAND_VALID = 1u, BNF_CAND_SAMPLE_NUMBER = 2u };

/* == bnflac_resync_slot */
typedef struct {
    uint32_t cand, gap; /* gap 1: a placeholder in front of frame cand */
    uint64_t position;  /* first sample of the record inside its stream */
} bnf_resync_slot;

/* == bnflac_resync_rec */
typedef struct {
    uint32_t flags, segments, gap_frames, reserved;
    uint64_t gap_samples, base;
} bnf_resync_rec;

enum { BNF_RESYNC_RESYNCED = 1u, BNF_RESYNC_CONTRADICTION = 2u, BNF_RESYNC_HEAD = 4u, BNF_RESYNC_LEADING = 8u };
enum { BNF_RESYNC_ST_GAPS = 8u, BNF_RESYNC_ST_ENDED = 16u }; /* status word 0, bits 3 and 4 */

BNF_SEL_HD inline uint64_t bnf_rs_pos(uint32_t cand_flags, uint64_t number, uint32_t B) {
    return (cand_flags & BNF_CAND_SAMPLE_NUMBER) ? number : number * B;
}

/* whether the table's successor (at p_next) continues the frame at p: see succ(i) above */
BNF_SEL_HD inline bool bnf_rs_linked(uint64_t p, uint32_t blocksize, uint64_t p_next) { return p + blocksize == p_next; }

BNF_SEL_HD inline uint64_t bnf_rs_base(uint64_t total, uint64_t p_head) { return total ? 0ull : p_head; }

BNF_SEL_HD inline bool bnf_rs_head_bad(uint64_t total, uint64_t p_head, uint32_t B) {
    return total != 0 && (p_head % B != 0 || p_head >= total);
}

BNF_SEL_HD inline bool bnf_rs_start_ok(bool valid, bool has_succ, uint64_t offset, uint64_t first_offset,
                                       uint32_t blocksize, uint64_t p, uint64_t base, uint64_t total, uint32_t B) {
    return valid && has_succ && offset >= first_offset && blocksize == B && p >= base && (p - base) % B == 0 &&
           (total == 0 || p < total);
}

/* A resync step from a record that ends at E to a start at L'.  false: contradiction; else *gap
 * placeholders stand at E + t * B. */
BNF_SEL_HD inline bool bnf_rs_step(uint64_t E, uint64_t l_new, uint32_t B, uint64_t *gap) {
    if (l_new < E || (l_new - E) % B != 0) return false;
    *gap = (l_new - E) / B;
    return true;
}

BNF_SEL_HD inline bool bnf_rs_eos(uint64_t total, uint64_t L) { return total != 0 && L >= total; }

BNF_SEL_HD inline uint32_t bnf_rs_sat32(uint64_t n) { return n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n; }

/* The placeholder record at stream position `position`: a lost-sync error record of one blocksize
 * whose header counts as parsed (sub_start[0] = 1), so the decode's fill pass zeroes its range. */
BNF_SEL_HD inline bnf_frame_info bnf_rs_placeholder(uint64_t next_frame_off, uint64_t position, uint64_t out_sample,
                                                    const bnf_stream_params &sp, uint32_t B) {
    bnf_frame_info r;
    r.status = BNF_ST_ERROR;
    r.err = 0; /* FLAC__STREAM_DECODER_ERROR_STATUS_LOST_SYNC */
    r.frame_off = next_frame_off;
    r.resume_bit = 0;
    r.cached = -1;
    r.blocksize = B;
    r.sample_rate = sp.sample_rate;
    r.channels = sp.channels;
    r.assignment = 0;
    r.bps = sp.bps;
    r.number_type = 0;
    r.unparseable = 0;
    r.number = position / B;
    r.out_sample = out_sample;
    r.crc8 = r.crc16_calc = r.crc16_read = r.crc_ok = 0;
    for (int k = 0; k < 8; k++) r.sub_start[k] = 0;
    r.sub_start[0] = 1;
    r.flags = BNF_FL_GAP;
    r.reserved = 0;
    return r;
}

/* The whole rule on host tables, as a plain walk: what the k_rs_* kernels compute from the same
 * candidate table.  slots (cap entries; may be NULL) gets one entry per record position below cap,
 * stream_frames / stream_samples (nstreams + 1 each) the exclusive prefixes of the records and
 * samples per stream, resync (may be NULL) one record per stream, status: [0] bit 1 more records
 * than cap, bit 3 placeholders or a resync step, bit 4 CONTRADICTION or HEAD; [1] ncand; [2] records;
 * [3] placeholders.  false: no memory, nothing written. */
inline bool bnf_resync_plan_host(const bnf_index_cand *cands, uint32_t ncand, const bnf_stream_desc *streams,
                                 uint32_t nstreams, uint32_t B, bnf_resync_slot *slots, uint32_t cap,
                                 uint32_t *stream_frames, uint64_t *stream_samples, bnf_resync_rec *resync,
                                 uint32_t status[4]) {
    /* per stream: the head; per candidate: the next start_ok candidate of its stream */
    int64_t *head = (int64_t *)malloc(sizeof(int64_t) * ((size_t)nstreams + 1));
    int64_t *last = (int64_t *)malloc(sizeof(int64_t) * ((size_t)nstreams + 1));
    int64_t *next_ok = (int64_t *)malloc(sizeof(int64_t) * ((size_t)ncand + 1));
    if (!head || !last || !next_ok) {
        free(head);
        free(last);
        free(next_ok);
        return false;
    }
    auto owned = [&](uint32_t i) { return cands[i].stream >= 0 && (uint32_t)cands[i].stream < nstreams; };
    auto succ_of = [&](uint32_t i) -> int64_t {
        const int32_t a = cands[i].succ;
        if (a < 0 || (uint32_t)a >= ncand || (uint32_t)a <= i || cands[a].stream != cands[i].stream) return -1;
        if (!bnf_rs_linked(bnf_rs_pos(cands[i].flags, cands[i].number, B), cands[i].blocksize,
                           bnf_rs_pos(cands[a].flags, cands[a].number, B)))
            return -1;
        return a;
    };
    for (uint32_t s = 0; s < nstreams; s++) head[s] = last[s] = -1;
    for (uint32_t i = 0; i < ncand; i++) {
        if (!owned(i) || !(cands[i].flags & BNF_CAND_VALID)) continue;
        const uint32_t s = (uint32_t)cands[i].stream;
        if (head[s] < 0 && cands[i].offset >= streams[s].first_offset) head[s] = i;
    }
    for (uint32_t k = ncand; k-- > 0;) {
        next_ok[k] = -1;
        if (!owned(k)) continue;
        const uint32_t s = (uint32_t)cands[k].stream;
        next_ok[k] = last[s];
        if (head[s] < 0) continue;
        const uint64_t total = streams[s].total_samples;
        const uint64_t base = bnf_rs_base(total, bnf_rs_pos(cands[head[s]].flags, cands[head[s]].number, B));
        if (bnf_rs_start_ok((cands[k].flags & BNF_CAND_VALID) != 0, succ_of(k) >= 0, cands[k].offset,
                            streams[s].first_offset, cands[k].blocksize, bnf_rs_pos(cands[k].flags, cands[k].number, B),
                            base, total, B))
            last[s] = k;
    }
    uint64_t nrec = 0, nsmp = 0, nph = 0; /* records, samples and placeholders so far, all streams */
    uint32_t bits = 0;
    for (uint32_t s = 0; s < nstreams; s++) {
        stream_frames[s] = bnf_rs_sat32(nrec);
        stream_samples[s] = nsmp;
        bnf_resync_rec r;
        memset(&r, 0, sizeof r);
        uint64_t gaps = 0;
        if (head[s] >= 0) {
            const uint64_t total = streams[s].total_samples;
            uint32_t x = (uint32_t)head[s];
            const uint64_t p_head = bnf_rs_pos(cands[x].flags, cands[x].number, B);
            r.base = bnf_rs_base(total, p_head);
            if (bnf_rs_head_bad(total, p_head, B)) {
                r.flags |= BNF_RESYNC_HEAD;
            } else {
                uint64_t L = p_head - r.base, gap = L / B;
                if (gap) r.flags |= BNF_RESYNC_LEADING;
                r.segments = 1;
                for (;;) {
                    if (bnf_rs_eos(total, L)) break;
                    for (uint64_t t = 0; t < gap && nrec + t < cap; t++)
                        if (slots) slots[nrec + t] = bnf_resync_slot{x, 1u, L - (gap - t) * B};
                    nrec += gap;
                    gaps += gap;
                    if (nrec < cap && slots) slots[nrec] = bnf_resync_slot{x, 0u, L};
                    nrec++;
                    const uint64_t E = L + cands[x].blocksize;
                    nsmp = stream_samples[s] + E;
                    const int64_t a = succ_of(x);
                    if (a >= 0) {
                        x = (uint32_t)a;
                        L = E;
                        gap = 0;
                        continue;
                    }
                    const int64_t j = next_ok[x];
                    if (j < 0) break;
                    const uint64_t l_new = bnf_rs_pos(cands[j].flags, cands[j].number, B) - r.base;
                    if (!bnf_rs_step(E, l_new, B, &gap)) {
                        r.flags |= BNF_RESYNC_CONTRADICTION;
                        break;
                    }
                    r.flags |= BNF_RESYNC_RESYNCED;
                    r.segments++;
                    x = (uint32_t)j;
                    L = l_new;
                }
            }
        }
        r.gap_frames = bnf_rs_sat32(gaps);
        r.gap_samples = gaps * B;
        nph += gaps;
        if (gaps || (r.flags & BNF_RESYNC_RESYNCED)) bits |= BNF_RESYNC_ST_GAPS;
        if (r.flags & (BNF_RESYNC_CONTRADICTION | BNF_RESYNC_HEAD)) bits |= BNF_RESYNC_ST_ENDED;
        if (resync) resync[s] = r;
    }
    stream_frames[nstreams] = bnf_rs_sat32(nrec);
    stream_samples[nstreams] = nsmp;
    status[0] = bits | (nrec > cap ? 2u : 0u);
    status[1] = ncand;
    status[2] = bnf_rs_sat32(nrec);
    status[3] = bnf_rs_sat32(nph);
    free(head);
    free(last);
    free(next_ok);
    return true;
}

#endif
