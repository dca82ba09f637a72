/* bnf_crc16.h -- the table-free CRC-16 that k_parse's prefix and the stereo kernels' tails share */
#ifndef BNF_CRC16_H
#define BNF_CRC16_H
#include "bnf_bitreader.h"

DEV uint32_t st_hmask(uint32_t h, uint32_t o) { /* little-endian dword at line offset o: bytes below h cleared */
    return h <= o ? ~0u : (h >= o + 4u ? 0u : (~0u << (8u * (h - o))));
}
/* ------------------------------------------------- CRC-16 remainder arithmetic
 * (the table-free zero test, st_crc16_ok below, and k_parse's prefix of it) */
struct CrcZ {
    uint32_t r0, r1, px; /* remainder mod T^4; XOR of every word (parity) */
};
DEV void crcz_w(CrcZ &c, uint32_t le) { /* one little-endian stream word */
    const uint32_t W = __builtin_bswap32(le);
    const uint32_t H = __builtin_amdgcn_alignbit(c.r1, c.r0, 28);
    const uint32_t n0 = W ^ H ^ (H << 4);
    c.r1 = c.r0 ^ (H >> 28);
    c.r0 = n0;
}
DEV void crcz_blk(CrcZ &c, uint4 v) {
    c.px ^= v.x ^ v.y ^ v.z ^ v.w;
    crcz_w(c, v.x);
    crcz_w(c, v.y);
    crcz_w(c, v.z);
    crcz_w(c, v.w);
}
/* k_parse's part of a 2-channel frame's CRC-16 (round 6).  The decode kernels' tail re-reads
 * the whole frame for the CRC-16, and every wave of a CU reaches its tail together, so those
 * bytes go at the HBM rate with nothing beside them.  k_parse walks subframe 0 anyway: its ring
 * holds those bytes, so it folds every whole 64-byte line before subframe 1's line into the
 * same T^4 remainder (from the ring while the line is one of its two, else one reload, L2-warm),
 * one 16-byte block at a time (three live state words: k_parse's occupancy is LDS-bound at 5
 * waves per SIMD, ~100 VGPRs), and the decode tail continues from there, re-reading only the
 * rest of the frame. */
/* The prefix state: the remainder mod Q(y) = y^15 + y + 1, y = x^32, in 15 words.  Q(y) =
 * T(x^32) = T(x)^32 is a multiple of T, so it keeps M mod T; with whole words as the
 * coefficients a 64-byte line is 18 word XORs at once (S y^16 + sum W[i] y^(15-i): y^15 = y + 1,
 * y^16 = y^2 + y; checked against bit-serial division mod T in Python while writing this)
 * against 96 VALU through the T^4 form, and the words are taken as loaded (little-endian): a
 * byte swap permutes the bits of every word alike, so it is applied to the 15 state words
 * once, at the hand-off (crcp_z).  k_parse<1> 128 VGPRs, 4 waves per SIMD: C2 k_parse 2.52 ->
 * 2.16 ms against the T^4 form (1.95 without a prefix), C3 the same as with it (10.43 vs
 * 10.47 ms per step; a build at 146 VGPRs, 3 waves, had cost C3's plain walk 0.5 ms). */
struct CrcP {
    uint32_t s[15]; /* s[k]: the coefficient of y^k (little-endian words) */
    uint32_t px;    /* XOR of every word (parity) */
    uint32_t wc;    /* next line to fold (absolute 64-byte line index); ~0: no prefix for this frame */
};
DEV void crcp_init(CrcP &c) {
#pragma unroll
    for (int k = 0; k < 15; k++) c.s[k] = 0u;
    c.px = 0u;
    c.wc = ~0u;
}
DEV void crcp_fold(CrcP &c, const u32x4 (&v)[4]) {
    const uint32_t W[16] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w,
                            v[2].x, v[2].y, v[2].z, v[2].w, v[3].x, v[3].y, v[3].z, v[3].w};
    c.px ^= W[0] ^ W[1] ^ W[2] ^ W[3] ^ W[4] ^ W[5] ^ W[6] ^ W[7] ^ W[8] ^ W[9] ^ W[10] ^ W[11] ^ W[12] ^ W[13] ^
            W[14] ^ W[15];
    const uint32_t r0 = c.s[13] ^ c.s[14] ^ W[15] ^ W[0], r1 = c.s[0] ^ c.s[13] ^ W[14] ^ W[0],
                   r2 = c.s[0] ^ c.s[1] ^ c.s[14] ^ W[13];
#pragma unroll
    for (int d = 14; d >= 3; d--) c.s[d] = c.s[d - 2] ^ c.s[d - 1] ^ W[15 - d]; /* descending: old s[d-2], s[d-1] */
    c.s[2] = r2;
    c.s[1] = r1;
    c.s[0] = r0;
    c.wc++;
}
/* the remainder in the decode tails' T^4 form (st_crc16_ok continues it) */
DEV CrcZ crcp_z(const CrcP &c) {
    CrcZ z{0u, 0u, 0u};
#pragma unroll
    for (int k = 14; k >= 0; k--) crcz_w(z, c.s[k]);
    z.px = c.px;
    return z;
}
/* fold the lines before line cl (whole wave).  The ring holds the two lines [iend / 4 - 2,
 * iend / 4), and the refill keeps the line of word wi (the reader's next word) and the one
 * after it: so before a refill, cl = wi / 16 -- every line the reader has loaded, which the
 * refill may overwrite -- folds from the ring (a line behind a landing refill reads again
 * from global memory, L2-warm; bounding by the cursor's bit position instead left 22% of C2's
 * lines to that path: the word lookahead crosses a line first).  The frame's first line is
 * folded before the walk (parse_frame), so these are whole lines. */
template <bool ALL = false, class C> /* ALL: every line before cl (the walk's end); else at most one (a refill point) */
DEV void crcp_hook(C &c, const BR &b, uint32_t lane, uint32_t cl) {
    for (uint32_t it = 0; any_lane(c.wc < cl) && (ALL || it == 0u); it++) {
        if (c.wc < cl) {
            const uint32_t L = c.wc;
            u32x4 v[4];
            if (L + 2u >= (b.iend >> 2)) {
#pragma unroll
                for (uint32_t i = 0; i < 4; i++)
                    v[i] = lds_ld128((const lds_u32x4 *)(b.ring + (((L & 1u) * 4u + i) * RING_LANE_DW) + lane * 4u));
                lds_sync();
                crcp_fold(c, v);
            } else { /* overwritten by a refill: read it again (each path folds: no merge of v) */
                const u32x4 *g = (const u32x4 *)((const uint8_t *)b.w + (uint64_t)L * 64u);
#pragma unroll
                for (uint32_t i = 0; i < 4; i++) v[i] = g[i];
                crcp_fold(c, v);
            }
        }
    }
}

#define CRC_LINES 4 /* 64-byte lines in flight per lane: each lane walks its own frame */

/* Zero test of the CRC-16 remainder of [b0, b1), the frame with its footer (read_frame_'s
 * check @0x10011a01: the footer equals the CRC of the frame bytes iff the CRC of frame + footer
 * is zero), by arithmetic, with no tables (round 6).  P = x^16 + x^15 + x^2 + 1 = (x + 1) T with
 * T = x^15 + x + 1, so M = 0 mod P iff M has even parity and M = 0 mod T.  The remainder mod
 * T^4 = x^60 + x^4 + 1 (a multiple of T) costs five VALU per 32-bit word: with the state
 * r = r1:r0 (60 bits; r1's top four bits are stale copies of bits alignbit already took),
 * r x^32 + W = (r0 mod x^28) x^32 + W + H (x^4 + 1), H = r >> 28.  Leading zero bytes leave M
 * unchanged and trailing ones multiply it by a power of x (invertible mod T), so whole 16-byte
 * blocks with the bytes outside [b0, b1) cleared give the same verdict.  The 11-bit LDS tables
 * this replaces cost 0.75 bank-conflicted lookups per byte on the CU's one LDS pipe. */
DEV uint32_t byte_keep(int32_t lo, int32_t hi, int32_t w) { /* bytes 4w..4w+3 kept iff in [lo, hi) */
    const int32_t a = min(max(lo - 4 * w, 0), 4), b = min(max(hi - 4 * w, 0), 4);
    const uint32_t mlo = a >= 4 ? 0u : (0xFFFFFFFFu << (8 * a));
    const uint32_t mhi = b >= 4 ? 0xFFFFFFFFu : ((1u << (8 * b)) - 1u);
    return mlo & mhi;
}
DEV bool crcz_zero(const CrcZ &c) {
    if (__builtin_popcount(c.px) & 1) return false;
    uint64_t v = ((uint64_t)(c.r1 & 0x0FFFFFFFu) << 32) | c.r0;
#pragma unroll
    for (int i = 0; i < 4; i++) { /* x^15 = x + 1: degree 59 -> 45 -> 31 -> 17 -> 14 */
        const uint64_t h = v >> 15;
        v = (v & 0x7FFFu) ^ h ^ (h << 1);
    }
    return v == 0;
}
/* the 64-byte line at q into the remainder, its bytes below h cleared (h = 0: whole line) */
DEV void crcz_line(CrcZ &c, uint4 (&v)[4], uint32_t h) {
    if (h) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            v[u].x &= st_hmask(h, 16u * u);
            v[u].y &= st_hmask(h, 16u * u + 4u);
            v[u].z &= st_hmask(h, 16u * u + 8u);
            v[u].w &= st_hmask(h, 16u * u + 12u);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) crcz_blk(c, v[u]);
}
/* CRC-16 verdict of [b0, b1) with NL 64-byte lines in flight per lane, continuing c, which
 * already holds the lines [b0 & ~63, from) (from: a line boundary) */
template <int NL = CRC_LINES>
DEV bool st_crc16_ok(const uint8_t *__restrict__ bytes, uint64_t b0, uint64_t b1, CrcZ c = CrcZ{0u, 0u, 0u},
                     uint64_t from = 0, CrcZ *fin = nullptr) { /* fin: the final remainder (check builds) */
    const uint64_t p0 = max(b0 & ~(uint64_t)63u, from);
    const uint32_t h = p0 < b0 ? (uint32_t)(b0 & 63u) : 0u;
    const uint32_t nl = b1 > p0 ? (uint32_t)((b1 - p0) >> 6) : 0u;
    uint64_t p = p0;
    if (nl) {
        const uint4 *q = (const uint4 *)(bytes + p0);
        uint4 buf[NL][4];
#pragma unroll
        for (int d = 0; d < NL; d++)
#pragma unroll
            for (int u = 0; u < 4; u++) buf[d][u] = q[4u * min((uint32_t)d, nl - 1u) + u];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            buf[0][u].x &= st_hmask(h, 16u * u);
            buf[0][u].y &= st_hmask(h, 16u * u + 4u);
            buf[0][u].z &= st_hmask(h, 16u * u + 8u);
            buf[0][u].w &= st_hmask(h, 16u * u + 12u);
        }
        for (uint32_t i = 0; i < nl; i += NL) {
#pragma unroll
            for (int d = 0; d < NL; d++) {
                if (i + d < nl) {
#pragma unroll
                    for (int u = 0; u < 4; u++) crcz_blk(c, buf[d][u]);
                    const uint32_t j = min(i + d + NL, nl - 1u);
#pragma unroll
                    for (int u = 0; u < 4; u++) buf[d][u] = q[4u * j + u];
                }
            }
        }
        p = p0 + (uint64_t)nl * 64u;
    }
    /* the rest, [p, b1): up to four 16-byte blocks (each starts below b1, so it lies inside the
     * 16-byte-rounded allocation), bytes below b0 (a frame inside one line) or from b1 on cleared */
    const uint32_t nr = (uint32_t)((b1 - p + 15u) >> 4);
    uint4 t[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) t[i] = i < nr ? *(const uint4 *)(bytes + p + 16u * i) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        if (i < nr) {
            const int64_t lo = (int64_t)b0 - (int64_t)(p + 16u * i), hi = (int64_t)b1 - (int64_t)(p + 16u * i);
            const int32_t l32 = (int32_t)max(min(lo, (int64_t)16), (int64_t)0);
            const int32_t h32 = (int32_t)max(min(hi, (int64_t)16), (int64_t)0);
            uint4 v = t[i];
            v.x &= byte_keep(l32, h32, 0);
            v.y &= byte_keep(l32, h32, 1);
            v.z &= byte_keep(l32, h32, 2);
            v.w &= byte_keep(l32, h32, 3);
            crcz_blk(c, v);
        }
    }
    if (fin) *fin = c;
    return crcz_zero(c);
}
/* The CRC-16 hand-off to the decode tails, 8 words per frame (crcp[8f..8f+7]): r0, r1 |
 * parity << 31 of a prefix, the lines it holds + 1 (0: none), frame_off's low word (a check);
 * the span to the next frame's offset (0: none), the verdict over that span, frame_off's low
 * word.  Written by k_parse (crc_mode 1: the prefix; 2: both). */
#define CRCP_WORDS 8u
/* the decode tails' CRC-16 verdict of the frame [b0, b1): the hand-off's verdict when the
 * frame ends where the next one starts, else its prefix continued, else the whole frame */
DEV bool st_crc16_frame(const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ crcp, uint32_t f, uint64_t b0,
                        uint64_t b1) {
    if (crcp) {
        const u32x4 v = *(const u32x4 *)(crcp + CRCP_WORDS * (uint64_t)f + 4u);
        if (v.x && v.z == (uint32_t)b0 && b0 + v.x == b1) return v.y != 0u;
        const u32x4 q = *(const u32x4 *)(crcp + CRCP_WORDS * (uint64_t)f);
        const uint64_t from = ((b0 >> 6) + q.z - 1u) * 64u;
        if (q.z && q.w == (uint32_t)b0 && from <= b1)
            return st_crc16_ok(bytes, b0, b1, CrcZ{q.x, q.y & 0x0FFFFFFFu, q.y >> 31}, from);
    }
    return st_crc16_ok(bytes, b0, b1);
}
#endif /* BNF_CRC16_H */
