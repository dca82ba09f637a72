/* bnf_crc16_tab.h -- the table CRC-16 of k_decode<W>, k_decode_sys and the frame chain */
#ifndef BNF_CRC16_TAB_H
#define BNF_CRC16_TAB_H
#include "bnf_crc16.h"

/* CRC-16 (poly 0x8005) over bytes [b0, b1), slice-by-8 with the tables in LDS. */
DEV uint32_t crc16_step8(uint32_t crc, uint32_t w0, uint32_t w1, const lds_u16 *T) {
    const uint32_t a = w0 ^ (crc << 16);
    return T[7 * 256 + (a >> 24)] ^ T[6 * 256 + ((a >> 16) & 0xff)] ^ T[5 * 256 + ((a >> 8) & 0xff)] ^
           T[4 * 256 + (a & 0xff)] ^ T[3 * 256 + (w1 >> 24)] ^ T[2 * 256 + ((w1 >> 16) & 0xff)] ^
           T[1 * 256 + ((w1 >> 8) & 0xff)] ^ T[w1 & 0xff];
}
DEV uint32_t crc16_range(const uint8_t *__restrict__ bytes, uint64_t b0, uint64_t b1, const lds_u16 *T) {
    uint32_t crc = 0;
    uint64_t p = b0;
    while (p < b1 && (p & 15u)) { crc = ((crc << 8) ^ T[((crc >> 8) ^ bytes[p]) & 0xff]) & 0xffff; p++; }
    const uint4 *q = (const uint4 *)(bytes + p);
    const uint32_t nq = (uint32_t)((b1 - p) >> 4);
    uint32_t i = 0;
    for (; i + 4 <= nq; i += 4) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = q[i + u];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            crc = crc16_step8(crc, __builtin_bswap32(v[u].x), __builtin_bswap32(v[u].y), T);
            crc = crc16_step8(crc, __builtin_bswap32(v[u].z), __builtin_bswap32(v[u].w), T);
        }
    }
    for (; i < nq; i++) {
        const uint4 v = q[i];
        crc = crc16_step8(crc, __builtin_bswap32(v.x), __builtin_bswap32(v.y), T);
        crc = crc16_step8(crc, __builtin_bswap32(v.z), __builtin_bswap32(v.w), T);
    }
    p += (uint64_t)nq * 16u;
    while (p < b1) { crc = ((crc << 8) ^ T[((crc >> 8) ^ bytes[p]) & 0xff]) & 0xffff; p++; }
    return crc;
}

/* a * b mod P over GF(2) (16-bit polynomials) */
DEV uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r = (r & 0x8000u) ? ((r << 1) ^ 0x8005u) & 0xffffu : (r << 1);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
/* crc * x^(8*nbytes) mod P: shift a CRC over nbytes appended bytes */
DEV uint32_t crc16_shift(uint32_t crc, uint64_t nbytes) {
    for (int j = 0; j < 40 && nbytes; j++, nbytes >>= 1)
        if (nbytes & 1u) crc = gf_mul(crc, g_crc16_xpow[j]);
    return crc;
}


/* Wave-cooperative CRC-16 of one byte range (the whole wave, coalesced 1 KB loads).
 * Layout: 16-byte pieces counted back from e = round_up(b1, 16); lane l takes pieces
 * 63 - l + 64 m, so every wave load is 64 consecutive pieces.  Each lane runs a CRC over
 * its own pieces with the 1008 bytes between them as zeros (x^(8*1008) by table TK), the
 * result is shifted to e by lanec = x^(8*16*(63 - l)), and the lanes are XOR-reduced.
 * Returns (wave-uniform) CRC([b0, b1)) * x^(8(e - b1)) mod P: zero iff the range's CRC is
 * zero (x is invertible mod P).  Bytes outside
 * [b0, b1) are masked to 0 (leading zeros leave a zero-initialised CRC at 0). */
DEV uint32_t crc_mulk(uint32_t a, const lds_u16 *TK) { return TK[a & 0xffu] ^ TK[256u + (a >> 8)]; }
DEV uint4 gld16(const uint8_t *p) { /* a global (not flat) 16-byte load */
    const u32x4 v = *(__attribute__((address_space(1))) const u32x4 *)(uintptr_t)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}
DEV uint32_t wave_crc_range(const uint8_t *__restrict__ bytes, uint64_t b0, uint64_t b1, const lds_u16 *T,
                            const lds_u16 *TK, uint32_t lanec, uint32_t lane) {
    const uint64_t e = (b1 + 15u) & ~15ull, a0 = b0 & ~15ull;
    const uint32_t np = (uint32_t)((e - a0) >> 4), M = (np + 63u) >> 6;
    uint32_t acc = 0;
    for (uint32_t m0 = 0; m0 < M; m0 += 4u) {
        uint4 v[4];
        uint64_t pp[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t m = m0 + (uint32_t)u;
            const uint32_t r = 63u - lane + 64u * (M - 1u - min(m, M - 1u));
            pp[u] = e - 16ull * (r + 1u);
            v[u] = (m < M && r < np) ? gld16(bytes + pp[u]) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (m0 + (uint32_t)u >= M) break; /* wave-uniform */
            const int64_t lo = (int64_t)b0 - (int64_t)pp[u], hi = (int64_t)b1 - (int64_t)pp[u];
            const bool edge = lo > 0 || hi < 16;
            if (any_lane(edge)) {
                if (edge) {
                    const int32_t l32 = (int32_t)max(min(lo, (int64_t)16), (int64_t)0);
                    const int32_t h32 = (int32_t)max(min(hi, (int64_t)16), (int64_t)0);
                    v[u].x &= byte_keep(l32, h32, 0);
                    v[u].y &= byte_keep(l32, h32, 1);
                    v[u].z &= byte_keep(l32, h32, 2);
                    v[u].w &= byte_keep(l32, h32, 3);
                }
            }
            acc = crc_mulk(acc, TK);
            acc = crc16_step8(acc, __builtin_bswap32(v[u].x), __builtin_bswap32(v[u].y), T);
            acc = crc16_step8(acc, __builtin_bswap32(v[u].z), __builtin_bswap32(v[u].w), T);
        }
    }
    acc = gf_mul(acc, lanec);
    for (int o = 32; o > 0; o >>= 1) acc ^= (uint32_t)__shfl_xor((int)acc, o);
    return acc;
}
/* the TK table (x^(8*1008) by bytes) into LDS, by the whole wave */
DEV void crc_tk_fill(lds_u16 *TK, uint32_t lane) {
    const uint32_t K = crc16_shift(1u, 1008u);
    for (uint32_t i = lane; i < 256u; i += 64u) {
        TK[i] = (uint16_t)gf_mul(i, K);
        TK[256u + i] = (uint16_t)gf_mul(i << 8, K);
    }
}
#endif /* BNF_CRC16_TAB_H */
