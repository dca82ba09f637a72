/* bnf_residual.h -- the residual reader of k_decode<W> and of k_decode_sys's producer */
#ifndef BNF_RESIDUAL_H
#define BNF_RESIDUAL_H
#include "bnf_bitreader.h"

/* ================================================================== k_decode */
#define DEC_LANES 64
#define RP 72 /* row-buffer stride (dwords) between samples: [sample][lane]; 4*RP = 32 mod 64 banks */

struct RS { /* residual reader state */
    uint32_t verb;   /* 1: VERBATIM raw values of `k` bits */
    uint32_t k, esc, left, pidx, nparts, psamples, order, plen, pesc, porder;
};

/* Rice partition header (read_residual_partitioned_rice_ @0x10012da0) */
template <bool CHECK = true>
DEV void read_partition(BR &b, RS &s) {
    const uint32_t kk = br_read<CHECK>(b, s.plen);
    s.left = (s.porder == 0 || s.pidx > 0) ? s.psamples : s.psamples - s.order;
    if (kk < s.pesc) {
        s.k = kk;
        s.esc = 0;
    } else {
        s.k = br_read<CHECK>(b, 5);
        s.esc = 1;
    }
    s.pidx++;
}

/* One Rice codeword (the block reader @0x10001b30/@0x1001aed0: u = (q << k) | lsb in
 * 32-bit unsigned, zig-zag). */
template <bool CHECK = true> /* false: the caller made sure the ring holds the word this reads */
DEV int32_t rice_one(BR &b, uint32_t k, uint64_t limit, uint32_t &trunc, PendW *pw = nullptr) {
    const uint32_t w = br_peek(b);
    /* v_ffbh gives ~0u for w == 0, which fails the unsigned test below like any prefix
     * too long for the window: the slow path then reads it */
    const uint32_t q0 = ffbh(w);
    const bool fast = q0 <= 31u - k;
    uint32_t u = (q0 << k) | __builtin_amdgcn_ubfe(w, 31u - k - q0, k);
    const bool slow = any_lane(!fast); /* wave-uniform, taken before the advance (stays in SGPRs) */
    br_adv<CHECK>(b, fast ? q0 + 1u + k : 0u, pw);
    if (__builtin_expect(slow, 0)) { /* the work is per lane */
        STAT(b.stats, 3);
        if (!fast) { /* long unary prefix: read_unary_unsigned, then the k low bits */
            uint32_t q;
            if (!br_unary(b, q, limit)) trunc = 1;
            u = (q << k) | br_read(b, k);
        }
    }
    return (int32_t)((u >> 1) ^ (0u - (u & 1u)));
}

/* next residual on the fused paths: a new partition's header and escaped (raw) partitions
 * inline behind wave-uniform tests, so a chunk need not lie inside one partition; Rice
 * codewords as rice_one.  An escaped lane issues its pending row write itself. */
DEV int32_t rice_fused(BR &b, RS &rs, uint64_t limit, uint32_t &trunc, PendW *pw) {
    /* one landing check per residual: with words wi .. wi+2 in the landed ring, the up to two
     * partition headers and one value below (<= 49 bits) advance unchecked; only a long
     * unary prefix (rice_one's slow path) reads on with checks */
    if (__builtin_expect(any_lane(b.wi + 2u >= b.vendw), 0)) {
        br_land(b, 2u);
        b.nx = ring_word(b, b.wi);
    }
    const bool np = rs.left == 0;
    if (__builtin_expect(any_lane(np), 0)) {
        if (np) {
            do { /* partition 0 holds no samples when the order equals the partition size */
                if (rs.pidx < rs.nparts) {
                    read_partition<false>(b, rs);
                } else { /* more samples than the partitions carry: a damaged frame */
                    trunc = 1;
                    rs.left = 0x7fffffffu;
                }
            } while (rs.left == 0);
        }
    }
    rs.left--;
    if (__builtin_expect(any_lane(rs.esc != 0u), 0)) {
        if (rs.esc) {
            if (pw && pw->on) *pw->at = pw->v;
            if (pw) pw->on = false;
            return br_read_s<false>(b, rs.k);
        }
    }
    return rice_one<false>(b, rs.k, limit, trunc, pw);
}

DEV void finish_partitions(BR &b, RS &s) {
    if (s.verb) return;
    while (s.pidx < s.nparts) {
        uint32_t kk = br_read(b, s.plen);
        if (kk >= s.pesc) br_read(b, 5);
        s.pidx++;
    }
}
#endif /* BNF_RESIDUAL_H */
