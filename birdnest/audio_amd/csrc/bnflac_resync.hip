/*
 * bnflac_resync.hip -- the frame chain of bnflac_index_streams_resync: k_rs_* after the unchanged
 * front of the batched chain (bnf_launch_chain_front: candidates, owners, parsed records, keys,
 * CRC-16 successors, heads).  No CRC tables, no g_stats, no ablate word.
 *
 * The rule is bnf_resync.h's.  Nothing here walks a chain or a gap: every step is one lane per
 * candidate, per stream or per output position, and prefix scans between them.  n is the candidate
 * count the front left in ctl (0 when the table is bad or the capacity overflowed), C the capacity.
 *   k_rs_heads     per stream: base, and the head as the first segment start.
 *   k_rs_prep      per candidate: its row of the candidate table (kept for the debug export), P, the
 *                  successor dropped from w.jump where the header numbers do not run on
 *                  (bnf_rs_linked), start_ok -> va = C - i where it holds, else 0.
 *   scan           reverse max-scan of va: the first start_ok candidate after i is C - vb[i].
 *   k_rs_link      per candidate: a valid one without successor gets that candidate as its link when
 *                  it lies inside the stream (below chi[s]); w.jump[0, C) = successor or link.
 *   bnf_launch_chain_jump  the existing pointer doubling over that array: the marked set.
 *   k_rs_marked    per marked candidate: its blocksize into va, and its link target becomes a segment
 *                  start (vs[j] = j + 1; only chain members make starts).
 *   scans          add-scan of va -> w.smp (samples of the marked before i), max-scan of vs -> vb (the
 *                  last segment start before i).
 *   k_rs_pos       per marked candidate: its segment start st, L = P[st] - base + smp[i] - smp[st];
 *                  a start checks its step against the end of the segment before it; the head checks
 *                  itself.  An unusable head, a contradiction and a frame at or past total each give
 *                  atomicMin(cut[s], i): the chain is kept below the stream's first such candidate.
 *   k_rs_count     per candidate: records (1 + gap) and samples of the kept ones; segments, gaps and
 *                  flags per stream by integer atomics (adds and ors: no result depends on their order).
 *   scans          add-scans -> rp, sq: the output position and out_sample of every candidate's first
 *                  record.  The streams ascend, so these are also the prefixes over the streams.
 *   k_rs_frames    per kept candidate: its record at rp[i] + gap.
 *   k_rs_gaps      per output position below cap: the candidate whose records cover it, by a binary
 *                  search over rp; a position in front of the candidate's own is a placeholder.
 *   k_rs_streams, k_rs_status   the two prefix tables, d_resync, the status words.
 * All scans are three launches (workgroup totals, their scan, apply), launch boundaries the only
 * ordering between workgroups.  Grids, loop bounds and scratch depend on cand_cap, nstreams, nbytes
 * and cap only: a gap's length is never a trip count.  A candidate entry is read only below n, a
 * stream entry below nstreams, an output written only below cap (nstreams + 1, nstreams).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bnf_resync.h"
#include "bnflac_launch.h"

#define RS_SCAN 1024u
#define RS_ADD 0
#define RS_MAX 1
#define RS_WHY_EOS 1u

static_assert(sizeof(bnf_index_cand) == 32 && sizeof(bnf_resync_rec) == 32 && sizeof(bnf_resync_slot) == 16, "record sizes");
static_assert(sizeof(bnf_frame_info) == 128 && sizeof(bnf_stream_desc) == 32, "table record sizes");

#define RS_DEV __device__ __forceinline__

RS_DEV uint32_t rs_n(const uint32_t *__restrict__ ctl) { return ctl[BNF_MS_N]; }

template <int OP>
RS_DEV uint64_t rs_op(uint64_t a, uint64_t b) {
    return OP == RS_ADD ? a + b : (a > b ? a : b);
}

/* Exclusive prefix of x over the workgroup's 1,024 lanes (identity 0 for both operations); tot: the
 * workgroup's total, in every lane.  ws: 16 words of LDS, free again after the next barrier. */
template <int OP>
RS_DEV uint64_t rs_block_excl(uint64_t x, uint64_t *ws, uint64_t &tot) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint64_t incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = __shfl_up(incl, o);
        if (lane >= (unsigned)o) incl = rs_op<OP>(incl, y);
    }
    const uint64_t below = __shfl_up(incl, 1);
    if (lane == 63u) ws[wv] = incl;
    __syncthreads();
    uint64_t pre = 0, all = 0;
    for (uint32_t k = 0; k < 16u; k++) {
        const uint64_t t = ws[k];
        if (k < wv) pre = rs_op<OP>(pre, t);
        all = rs_op<OP>(all, t);
    }
    tot = all;
    return lane ? rs_op<OP>(pre, below) : pre;
}

/* count of a scan: min(*n_ptr, cap) elements, or cap when the host knows it */
RS_DEV uint32_t rs_count(const uint32_t *__restrict__ n_ptr, uint32_t cap) { return n_ptr ? min(*n_ptr, cap) : cap; }

/* Scan position t holds element t, or element n - 1 - t of a reverse scan. */
template <int OP, bool REV>
__global__ void __launch_bounds__(RS_SCAN) k_rs_scan_reduce(const uint64_t *__restrict__ v, const uint32_t *__restrict__ n_ptr,
                                                            uint32_t cap, uint64_t *__restrict__ bsum) {
    __shared__ uint64_t ws[16];
    const uint32_t t = blockIdx.x * RS_SCAN + threadIdx.x, n = rs_count(n_ptr, cap);
    uint64_t tot;
    (void)rs_block_excl<OP>(t < n ? v[REV ? n - 1u - t : t] : 0ull, ws, tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

/* the workgroup totals' own exclusive scan, in place (one workgroup; nb comes from the capacity) */
template <int OP>
__global__ void __launch_bounds__(RS_SCAN) k_rs_scan_sums(uint64_t *__restrict__ bsum, uint32_t nb) {
    __shared__ uint64_t ws[16];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < nb; base += RS_SCAN) {
        const uint32_t i = base + threadIdx.x;
        uint64_t tot;
        const uint64_t ex = rs_block_excl<OP>(i < nb ? bsum[i] : 0ull, ws, tot);
        if (i < nb) bsum[i] = rs_op<OP>(carry, ex);
        carry = rs_op<OP>(carry, tot);
        __syncthreads(); /* ws is written again */
    }
}

/* out: the exclusive prefixes; a forward scan also writes the total as entry n */
template <int OP, bool REV>
__global__ void __launch_bounds__(RS_SCAN) k_rs_scan_apply(const uint64_t *__restrict__ v, const uint32_t *__restrict__ n_ptr,
                                                           uint32_t cap, const uint64_t *__restrict__ bsum,
                                                           uint64_t *__restrict__ out) {
    __shared__ uint64_t ws[16];
    const uint32_t t = blockIdx.x * RS_SCAN + threadIdx.x, n = rs_count(n_ptr, cap);
    uint64_t tot;
    const uint64_t ex = rs_op<OP>(bsum[blockIdx.x], rs_block_excl<OP>(t < n ? v[REV ? n - 1u - t : t] : 0ull, ws, tot));
    if (t < n) out[REV ? n - 1u - t : t] = ex;
    else if (!REV && t == n) out[n] = ex;
}

/* v[0, n) -> out[0, n] (n = min(*n_ptr, cap)); nb covers element cap */
template <int OP, bool REV>
static void rs_scan(const uint64_t *v, const uint32_t *n_ptr, uint32_t cap, uint64_t *bsum, uint64_t *out, hipStream_t s) {
    const uint32_t nb = cap / RS_SCAN + 1u;
    hipLaunchKernelGGL((k_rs_scan_reduce<OP, REV>), dim3(nb), dim3(RS_SCAN), 0, s, v, n_ptr, cap, bsum);
    hipLaunchKernelGGL((k_rs_scan_sums<OP>), dim3(1), dim3(RS_SCAN), 0, s, bsum, nb);
    hipLaunchKernelGGL((k_rs_scan_apply<OP, REV>), dim3(nb), dim3(RS_SCAN), 0, s, v, n_ptr, cap, bsum, out);
}

RS_DEV uint32_t rs_cand_flags(uint32_t key, uint32_t number_type) {
    return (key & BNF_MS_KEY_OK) ? (BNF_CAND_VALID | (number_type ? BNF_CAND_SAMPLE_NUMBER : 0u)) : 0u;
}

/* base[s] and the head as a segment start.  A head is a valid candidate, so its record is parsed. */
__global__ void __launch_bounds__(256) k_rs_heads(const int32_t *__restrict__ head, uint32_t nstreams,
                                                  const uint32_t *__restrict__ ctl, const bnf_frame_info *__restrict__ info,
                                                  const bnf_stream_desc *__restrict__ sd, uint32_t B,
                                                  uint64_t *__restrict__ base, uint64_t *__restrict__ vs) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= nstreams) return;
    const int32_t h = head[s];
    uint64_t b = 0;
    if (h >= 0 && (uint32_t)h < rs_n(ctl)) {
        const uint32_t fl = info[h].number_type ? BNF_CAND_SAMPLE_NUMBER : 0u;
        b = bnf_rs_base(sd[s].total_samples, bnf_rs_pos(fl, info[h].number, B));
        vs[h] = (uint64_t)h + 1u;
    }
    base[s] = b;
}

__global__ void __launch_bounds__(256) k_rs_prep(const uint64_t *__restrict__ cand, const uint32_t *__restrict__ ctl,
                                                 const bnf_frame_info *__restrict__ info, const int32_t *__restrict__ seg,
                                                 const uint32_t *__restrict__ key, int32_t *__restrict__ succ,
                                                 const bnf_stream_desc *__restrict__ sd, const uint64_t *__restrict__ base,
                                                 uint32_t B, uint32_t C, bnf_index_cand *__restrict__ ct,
                                                 uint64_t *__restrict__ p, uint64_t *__restrict__ va) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= rs_n(ctl)) return;
    const uint32_t k = key[i];
    const bool valid = (k & BNF_MS_KEY_OK) != 0u; /* implies an owner and a parsed record */
    bnf_index_cand c;
    c.offset = cand[i];
    c.number = valid ? info[i].number : 0ull;
    c.succ = succ[i];
    c.stream = seg[i];
    c.blocksize = valid ? info[i].blocksize : 0u;
    c.flags = valid ? rs_cand_flags(k, info[i].number_type) : 0u;
    ct[i] = c;
    uint64_t pos = 0;
    bool ok = false;
    if (valid) {
        const bnf_stream_desc d = sd[c.stream];
        pos = bnf_rs_pos(c.flags, c.number, B);
        bool linked = false;
        if (c.succ >= 0) { /* a successor is a valid candidate of the same stream: its record is parsed */
            const bnf_frame_info &nx = info[c.succ];
            linked = bnf_rs_linked(pos, c.blocksize, bnf_rs_pos(nx.number_type ? BNF_CAND_SAMPLE_NUMBER : 0u, nx.number, B));
            if (!linked) succ[i] = -1; /* this lane's own entry */
        }
        ok = bnf_rs_start_ok(true, linked, c.offset, d.first_offset, c.blocksize, pos, base[c.stream], d.total_samples, B);
    }
    p[i] = pos;
    va[i] = ok ? (uint64_t)(C - i) : 0ull;
}

/* jump[i]: the successor, or the link of a valid candidate without one; ext[i]: the link alone */
__global__ void __launch_bounds__(256) k_rs_link(const uint32_t *__restrict__ ctl, const bnf_index_cand *__restrict__ ct,
                                                 const uint64_t *__restrict__ vb, const uint32_t *__restrict__ chi, uint32_t C,
                                                 int32_t *jump, int32_t *__restrict__ ext) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= rs_n(ctl)) return;
    int32_t link = -1;
    if ((ct[i].flags & BNF_CAND_VALID) && jump[i] < 0) {
        const uint64_t v = vb[i];
        if (v != 0) {
            const uint32_t j = C - (uint32_t)v; /* i < j < n */
            if (j < chi[ct[i].stream]) link = (int32_t)j;
        }
    }
    ext[i] = link;
    if (link >= 0) jump[i] = link;
}

__global__ void __launch_bounds__(256) k_rs_marked(const uint32_t *__restrict__ ctl, const uint32_t *__restrict__ mark,
                                                   const bnf_index_cand *__restrict__ ct, const int32_t *__restrict__ ext,
                                                   uint64_t *__restrict__ va, uint64_t *__restrict__ vs) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= rs_n(ctl)) return;
    const bool m = mark[i] != 0u;
    va[i] = m ? ct[i].blocksize : 0u;
    const int32_t j = ext[i];
    if (m && j >= 0) vs[j] = (uint64_t)j + 1u; /* one writer per target: a chain member has one predecessor */
}

__global__ void __launch_bounds__(256) k_rs_pos(const uint32_t *__restrict__ ctl, const uint32_t *__restrict__ mark,
                                                const bnf_index_cand *__restrict__ ct, const int32_t *__restrict__ head,
                                                const bnf_stream_desc *__restrict__ sd, const uint64_t *__restrict__ base,
                                                const uint64_t *__restrict__ p, const uint64_t *__restrict__ smp,
                                                const uint64_t *__restrict__ vs, const uint64_t *__restrict__ vb, uint32_t B,
                                                uint64_t *__restrict__ lv, uint64_t *__restrict__ gapv,
                                                uint32_t *__restrict__ why, int32_t *__restrict__ cut) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= rs_n(ctl) || !mark[i]) return;
    const int32_t s = ct[i].stream;
    const uint64_t b = base[s], total = sd[s].total_samples;
    const bool start = vs[i] != 0;
    /* the segment's start: a marked candidate lies at or after its stream's head, which is one, so
     * vb[i] >= 1 whenever it is read (the test keeps an index below 0 out of the tables regardless) */
    if (vb[i] == 0 && (!start || (int32_t)i != head[s])) {
        lv[i] = gapv[i] = 0;
        why[i] = RS_WHY_EOS;
        atomicMin(&cut[s], (int32_t)i);
        return;
    }
    const uint32_t st = start ? i : (uint32_t)vb[i] - 1u;
    const uint64_t L = (p[st] - b) + (smp[i] - smp[st]);
    uint64_t gap = 0;
    uint32_t y = 0;
    if (start) {
        if ((int32_t)i == head[s]) {
            if (bnf_rs_head_bad(total, p[i], B)) y = BNF_RESYNC_HEAD;
            else gap = L / B;
        } else { /* reached by a link from the segment before, which starts at vb[i] - 1 and ends at E */
            const uint32_t pv = (uint32_t)vb[i] - 1u;
            const uint64_t E = (p[pv] - b) + (smp[i] - smp[pv]);
            if (!bnf_rs_step(E, L, B, &gap)) y = BNF_RESYNC_CONTRADICTION;
        }
    }
    if (!y && bnf_rs_eos(total, L)) y = RS_WHY_EOS;
    lv[i] = L;
    gapv[i] = gap;
    why[i] = y;
    if (y) atomicMin(&cut[s], (int32_t)i);
}

__global__ void __launch_bounds__(256) k_rs_count(const uint32_t *__restrict__ ctl, const uint32_t *__restrict__ mark,
                                                  const bnf_index_cand *__restrict__ ct, const int32_t *__restrict__ head,
                                                  const int32_t *__restrict__ cut, const uint64_t *__restrict__ vs,
                                                  const uint64_t *__restrict__ gapv, const uint32_t *__restrict__ why,
                                                  uint32_t B, uint64_t *__restrict__ rc, uint64_t *__restrict__ sc,
                                                  uint32_t *__restrict__ segs, uint32_t *__restrict__ rflags,
                                                  uint64_t *__restrict__ gapc, uint64_t *__restrict__ acc) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= rs_n(ctl)) return;
    uint64_t recs = 0, smps = 0;
    if (mark[i]) {
        const int32_t s = ct[i].stream, c = cut[s];
        if ((int32_t)i < c) {
            const uint64_t gap = gapv[i];
            recs = 1u + gap;
            smps = ct[i].blocksize + gap * B;
            if (vs[i] != 0) {
                atomicAdd(&segs[s], 1u);
                if (gap) {
                    atomicAdd((unsigned long long *)&gapc[s], (unsigned long long)gap);
                    atomicAdd((unsigned long long *)&acc[0], (unsigned long long)gap);
                    if ((int32_t)i == head[s]) atomicOr(&rflags[s], (uint32_t)BNF_RESYNC_LEADING);
                }
            }
        } else if ((int32_t)i == c && (why[i] & (BNF_RESYNC_HEAD | BNF_RESYNC_CONTRADICTION))) {
            atomicOr(&rflags[s], why[i]);
        }
    }
    rc[i] = recs;
    sc[i] = smps;
}

__global__ void __launch_bounds__(256) k_rs_frames(const uint32_t *__restrict__ ctl, const uint32_t *__restrict__ mark,
                                                   const bnf_index_cand *__restrict__ ct, const int32_t *__restrict__ cut,
                                                   const bnf_frame_info *__restrict__ info, const uint64_t *__restrict__ gapv,
                                                   const uint64_t *__restrict__ rp, const uint64_t *__restrict__ sq, uint32_t B,
                                                   uint64_t *__restrict__ d_offs, uint64_t *__restrict__ d_os,
                                                   bnf_frame_info *__restrict__ d_info, uint32_t cap) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= rs_n(ctl) || !mark[i]) return;
    if ((int32_t)i >= cut[ct[i].stream]) return;
    const uint64_t gap = gapv[i], at = rp[i] + gap;
    if (at >= cap) return;
    const uint64_t os = sq[i] + gap * B;
    d_offs[at] = ct[i].offset;
    if (d_os) d_os[at] = os;
    if (d_info) {
        bnf_frame_info fi = info[i];
        fi.out_sample = os;
        d_info[at] = fi;
    }
}

/* One lane per output position.  rp[0, n] ascends from 0 to the record total; the candidate that covers
 * position q is the last one with rp[i] <= q, found in at most 32 halvings of [0, n]. */
__global__ void __launch_bounds__(256) k_rs_gaps(const uint32_t *__restrict__ ctl, const bnf_index_cand *__restrict__ ct,
                                                 const uint64_t *__restrict__ gapv, const uint64_t *__restrict__ lv,
                                                 const uint64_t *__restrict__ rp, const uint64_t *__restrict__ sq,
                                                 const uint64_t *__restrict__ acc, bnf_stream_params sp, uint32_t B,
                                                 uint64_t *__restrict__ d_offs, uint64_t *__restrict__ d_os,
                                                 bnf_frame_info *__restrict__ d_info, uint32_t cap) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n = rs_n(ctl);
    if (q >= cap || acc[0] == 0 || q >= rp[n]) return;
    uint32_t lo = 0, hi = n; /* rp[lo] <= q < rp[hi] */
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (rp[mid] <= q) lo = mid;
        else hi = mid;
    }
    const uint64_t t = q - rp[lo], gap = gapv[lo];
    if (t >= gap) return; /* the candidate's own record */
    const uint64_t os = sq[lo] + t * B;
    d_offs[q] = ct[lo].offset;
    if (d_os) d_os[q] = os;
    if (d_info) d_info[q] = bnf_rs_placeholder(ct[lo].offset, lv[lo] - (gap - t) * B, os, sp, B);
}

/* entry s of the two prefix tables (s <= nstreams) and the stream's resync record */
__global__ void __launch_bounds__(256) k_rs_streams(const uint32_t *__restrict__ ctl, const uint32_t *__restrict__ clo,
                                                    uint32_t nstreams, const uint64_t *__restrict__ rp,
                                                    const uint64_t *__restrict__ sq, const uint32_t *__restrict__ segs,
                                                    const uint32_t *__restrict__ rflags, const uint64_t *__restrict__ gapc,
                                                    const uint64_t *__restrict__ base, uint32_t B, uint32_t *__restrict__ d_sf,
                                                    uint64_t *__restrict__ d_ss, bnf_resync_rec *__restrict__ d_resync,
                                                    uint64_t *__restrict__ acc) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s > nstreams) return;
    const uint32_t at = s < nstreams ? clo[s] : rs_n(ctl); /* clo is 0 when n is */
    d_sf[s] = bnf_rs_sat32(rp[at]);
    if (d_ss) d_ss[s] = sq[at];
    if (s == nstreams) return;
    bnf_resync_rec r;
    r.flags = rflags[s] | (segs[s] >= 2u ? (uint32_t)BNF_RESYNC_RESYNCED : 0u);
    r.segments = segs[s];
    r.gap_frames = bnf_rs_sat32(gapc[s]);
    r.reserved = 0;
    r.gap_samples = gapc[s] * B;
    r.base = base[s];
    if (d_resync) d_resync[s] = r;
    const uint32_t bits = ((gapc[s] || (r.flags & BNF_RESYNC_RESYNCED)) ? (uint32_t)BNF_RESYNC_ST_GAPS : 0u) |
                          ((r.flags & (BNF_RESYNC_CONTRADICTION | BNF_RESYNC_HEAD)) ? (uint32_t)BNF_RESYNC_ST_ENDED : 0u);
    if (bits) atomicOr((unsigned long long *)&acc[1], (unsigned long long)bits);
}

__global__ void k_rs_status(const uint32_t *__restrict__ ctl, uint32_t cand_cap, const uint64_t *__restrict__ rp,
                            const uint64_t *__restrict__ acc, uint32_t cap, uint32_t *__restrict__ status) {
    const uint64_t total = rp[rs_n(ctl)];
    status[0] = (ctl[BNF_MS_NCAND] > cand_cap ? 1u : 0u) | (total > cap ? 2u : 0u) | (ctl[BNF_MS_BAD] ? 4u : 0u) |
                (uint32_t)acc[1];
    status[1] = ctl[BNF_MS_NCAND];
    status[2] = bnf_rs_sat32(total);
    status[3] = bnf_rs_sat32(acc[0]);
}

/* ------------------------------------------------------------------ scratch and launch */
static size_t rs_round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

struct rs_layout {
    size_t ct, v[10], bsum, ext, why, cut, segs, rflags, gapc, base, acc, end;
};

static rs_layout rs_lay(uint32_t cand_cap, uint32_t nstreams) {
    const size_t C = cand_cap, S = nstreams, nsum = std::max(C, S) / RS_SCAN + 2;
    rs_layout l;
    size_t off = 0;
    auto take = [&off](size_t bytes) {
        const size_t at = off;
        off += rs_round16(bytes);
        return at;
    };
    l.ct = take(sizeof(bnf_index_cand) * C);
    for (int k = 0; k < 10; k++) l.v[k] = take(8 * (C + 1));
    l.bsum = take(8 * nsum);
    l.ext = take(4 * C);
    l.why = take(4 * C);
    l.cut = take(4 * S);
    l.segs = take(4 * S);
    l.rflags = take(4 * S);
    l.gapc = take(8 * S);
    l.base = take(8 * S);
    l.acc = take(16);
    l.end = off;
    return l;
}

extern "C" uint64_t bnf_resync_scratch_bytes(uint32_t cand_cap, uint32_t nstreams) { return rs_lay(cand_cap, nstreams).end; }

extern "C" bnf_rs_scratch bnf_resync_carve(void *mem, uint32_t cand_cap, uint32_t nstreams) {
    const rs_layout l = rs_lay(cand_cap, nstreams);
    uint8_t *m = (uint8_t *)mem;
    bnf_rs_scratch r;
    r.ct = (bnf_index_cand *)(m + l.ct);
    uint64_t **v[10] = {&r.p, &r.va, &r.vb, &r.vs, &r.gapv, &r.lv, &r.rc, &r.sc, &r.rp, &r.sq};
    for (int k = 0; k < 10; k++) *v[k] = (uint64_t *)(m + l.v[k]);
    r.bsum = (uint64_t *)(m + l.bsum);
    r.ext = (int32_t *)(m + l.ext);
    r.why = (uint32_t *)(m + l.why);
    r.cut = (int32_t *)(m + l.cut);
    r.segs = (uint32_t *)(m + l.segs);
    r.rflags = (uint32_t *)(m + l.rflags);
    r.gapc = (uint64_t *)(m + l.gapc);
    r.base = (uint64_t *)(m + l.base);
    r.acc = (uint64_t *)(m + l.acc);
    return r;
}

extern "C" hipError_t bnf_launch_chain_streams_resync(const uint8_t *bytes, uint64_t nbytes, const bnf_stream_desc *sd,
                                                      uint32_t nstreams, bnf_stream_params sp, uint32_t cand_cap,
                                                      bnf_ms_scratch w, bnf_rs_scratch r, uint64_t *d_offs, uint64_t *d_os,
                                                      bnf_frame_info *d_info, uint32_t cap, uint32_t *d_sf, uint64_t *d_ss,
                                                      bnf_resync_rec *d_resync, uint32_t *d_status, hipStream_t s) {
    const uint32_t C = cand_cap, S = nstreams, B = sp.min_blocksize;
    const dim3 gc((C + 255u) / 256u), gs((S + 255u) / 256u), t256(256);
    const uint32_t *ctl = w.ctl, *n_ptr = w.ctl + BNF_MS_N;
    const rs_layout l = rs_lay(C, S);
    /* presets: no segment start, no cut, no segment, flag or gap counted (cut .. acc are adjacent) */
    hipError_t e = hipMemsetAsync(r.vs, 0, 8 * ((size_t)C + 1), s);
    if (e == hipSuccess) e = hipMemsetAsync(r.cut, 0x7f, 4 * (size_t)S, s);
    if (e == hipSuccess) e = hipMemsetAsync(r.segs, 0, l.end - l.segs, s);
    if (e == hipSuccess) e = bnf_launch_chain_front(bytes, nbytes, sd, S, sp, C, w, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rs_heads, gs, t256, 0, s, w.head, S, ctl, w.info, sd, B, r.base, r.vs);
    hipLaunchKernelGGL(k_rs_prep, gc, t256, 0, s, w.cand, ctl, w.info, w.seg, w.key, w.jump, sd, r.base, B, C, r.ct, r.p, r.va);
    rs_scan<RS_MAX, true>(r.va, n_ptr, C, r.bsum, r.vb, s);
    hipLaunchKernelGGL(k_rs_link, gc, t256, 0, s, ctl, r.ct, r.vb, w.chi, C, w.jump, r.ext);
    e = bnf_launch_chain_jump(C, w, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rs_marked, gc, t256, 0, s, ctl, w.mark, r.ct, r.ext, r.va, r.vs);
    rs_scan<RS_ADD, false>(r.va, n_ptr, C, r.bsum, w.smp, s);
    rs_scan<RS_MAX, false>(r.vs, n_ptr, C, r.bsum, r.vb, s);
    hipLaunchKernelGGL(k_rs_pos, gc, t256, 0, s, ctl, w.mark, r.ct, w.head, sd, r.base, r.p, w.smp, r.vs, r.vb, B, r.lv, r.gapv,
                       r.why, r.cut);
    hipLaunchKernelGGL(k_rs_count, gc, t256, 0, s, ctl, w.mark, r.ct, w.head, r.cut, r.vs, r.gapv, r.why, B, r.rc, r.sc, r.segs,
                       r.rflags, r.gapc, r.acc);
    rs_scan<RS_ADD, false>(r.rc, n_ptr, C, r.bsum, r.rp, s);
    rs_scan<RS_ADD, false>(r.sc, n_ptr, C, r.bsum, r.sq, s);
    if (cap) {
        hipLaunchKernelGGL(k_rs_frames, gc, t256, 0, s, ctl, w.mark, r.ct, r.cut, w.info, r.gapv, r.rp, r.sq, B, d_offs, d_os,
                           d_info, cap);
        hipLaunchKernelGGL(k_rs_gaps, dim3((uint32_t)(((uint64_t)cap + 255u) / 256u)), t256, 0, s, ctl, r.ct, r.gapv, r.lv, r.rp,
                           r.sq, r.acc, sp, B, d_offs, d_os, d_info, cap);
    }
    hipLaunchKernelGGL(k_rs_streams, dim3((uint32_t)(((uint64_t)S + 256u) / 256u)), t256, 0, s, ctl, w.clo, S, r.rp, r.sq, r.segs,
                       r.rflags, r.gapc, r.base, B, d_sf, d_ss, d_resync, r.acc);
    hipLaunchKernelGGL(k_rs_status, dim3(1), dim3(1), 0, s, ctl, C, r.rp, r.acc, cap, d_status);
    return hipGetLastError();
}
