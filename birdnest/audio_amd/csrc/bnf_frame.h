/* bnf_frame.h -- frame header and subframe header parse; channel decorrelation */
#ifndef BNF_FRAME_H
#define BNF_FRAME_H
#include "bnf_bitreader.h"

/* ------------------------------------------------------------ frame header */
enum { E_LOST_SYNC = 0, E_BAD_HEADER = 1, E_CRC = 2, E_UNPARSEABLE = 3 };

/* read_frame_header_ @0x10011d70: fills fi; returns BNF_ST_* (OK also when the header
 * is flagged unparseable -- the caller reports that after the number conversion). */
template <class R> /* R: BR (lane cursor) or WR (wave-uniform cursor) */
DEV uint32_t parse_header(R &b, uint64_t fbit, uint64_t limit, const bnf_stream_params &sp,
                          bnf_frame_info &fi) {
    /* the header's CRC-8 is folded in as each byte is read (no byte buffer: a per-lane array
     * indexed at run time would live in scratch memory) */
    uint32_t crc = 0, last = 0, b2 = 0, b3 = 0;
    auto take = [&](uint32_t v) { crc = g_crc8_tab[crc ^ v]; last = v; };
    uint32_t unparseable = 0, bs_hint = 0, sr_hint = 0, x;
    br_seek(b, fbit);
    take(br_read(b, 8));
    const uint32_t b1 = br_read(b, 8);
    take(b1);
    fi.cached = -1;
    if (b1 & 0x02) unparseable = 1;
    for (int i = 0; i < 2; i++) {
        x = br_read(b, 8);
        if (x == 0xff) {
            fi.cached = 0xff;
            fi.err = E_BAD_HEADER;
            fi.resume_bit = br_pos(b);
            return BNF_ST_ERROR;
        }
        take(x);
        if (i == 0) b2 = x;
        else b3 = x;
    }
    x = b2 >> 4;
    if (x == 0) unparseable = 1;
    else if (x == 1) fi.blocksize = 192;
    else if (x <= 5) fi.blocksize = 576u << (x - 2);
    else if (x <= 7) bs_hint = x;
    else fi.blocksize = 256u << (x - 8);
    x = b2 & 0x0f;
    switch (x) {
    case 0:
        if (sp.has_stream_info) fi.sample_rate = sp.sample_rate;
        else unparseable = 1;
        break;
    case 1: fi.sample_rate = 88200; break;
    case 2: fi.sample_rate = 176400; break;
    case 3: fi.sample_rate = 192000; break;
    case 4: fi.sample_rate = 8000; break;
    case 5: fi.sample_rate = 16000; break;
    case 6: fi.sample_rate = 22050; break;
    case 7: fi.sample_rate = 24000; break;
    case 8: fi.sample_rate = 32000; break;
    case 9: fi.sample_rate = 44100; break;
    case 10: fi.sample_rate = 48000; break;
    case 11: fi.sample_rate = 96000; break;
    case 15:
        fi.err = E_BAD_HEADER;
        fi.resume_bit = br_pos(b);
        return BNF_ST_ERROR;
    default: sr_hint = x; break;
    }
    x = b3 >> 4;
    if (x & 8) {
        fi.channels = 2;
        if ((x & 7) <= 2) fi.assignment = (x & 7) + 1;
        else unparseable = 1;
    } else {
        fi.channels = x + 1;
        fi.assignment = 0;
    }
    x = (b3 & 0x0e) >> 1;
    switch (x) {
    case 0:
        if (sp.has_stream_info) fi.bps = sp.bps;
        else unparseable = 1;
        break;
    case 1: fi.bps = 8; break;
    case 2: fi.bps = 12; break;
    case 4: fi.bps = 16; break;
    case 5: fi.bps = 20; break;
    case 6: fi.bps = 24; break;
    default: unparseable = 1; break;
    }
    if (b3 & 0x01) unparseable = 1;
    /* UTF-8 frame/sample number (@0x10001e20 / @0x10001f60), with libFLAC's truthiness tests */
    const bool is64 = (b1 & 0x01) || (sp.has_stream_info && sp.min_blocksize != sp.max_blocksize);
    {
        uint64_t v = 0;
        uint32_t n;
        bool bad = false;
        x = br_read(b, 8);
        take(x);
        if (!(x & 0x80)) { v = x; n = 0; }
        else if ((x & 0xC0) && !(x & 0x20)) { v = x & 0x1F; n = 1; }
        else if ((x & 0xE0) && !(x & 0x10)) { v = x & 0x0F; n = 2; }
        else if ((x & 0xF0) && !(x & 0x08)) { v = x & 0x07; n = 3; }
        else if ((x & 0xF8) && !(x & 0x04)) { v = x & 0x03; n = 4; }
        else if ((x & 0xFC) && !(x & 0x02)) { v = x & 0x01; n = 5; }
        else if (is64 && (x & 0xFE) && !(x & 0x01)) { v = 0; n = 6; }
        else { bad = true; n = 0; }
        for (; !bad && n; n--) {
            x = br_read(b, 8);
            take(x);
            if (!(x & 0x80) || (x & 0x40)) bad = true;
            else v = (v << 6) | (x & 0x3F);
        }
        if (!is64 && !bad) v &= 0xffffffffull; /* 32-bit accumulation (6 bytes max => 31 bits) */
        if (bad) {
            fi.cached = (int32_t)last;
            fi.err = E_BAD_HEADER;
            fi.resume_bit = br_pos(b);
            return BNF_ST_ERROR;
        }
        fi.number_type = is64 ? 1u : 0u;
        fi.number = v;
    }
    if (bs_hint) {
        x = br_read(b, 8);
        take(x);
        if (bs_hint == 7) {
            uint32_t y = br_read(b, 8);
            take(y);
            x = (x << 8) | y;
        }
        fi.blocksize = x + 1;
    }
    if (sr_hint) {
        x = br_read(b, 8);
        take(x);
        if (sr_hint != 12) {
            uint32_t y = br_read(b, 8);
            take(y);
            x = (x << 8) | y;
        }
        fi.sample_rate = (sr_hint == 12) ? x * 1000u : (sr_hint == 13 ? x : x * 10u);
    }
    x = br_read(b, 8);
    fi.crc8 = x;
    if (br_pos(b) > limit) return BNF_ST_TRUNC;
    if (crc != (x & 0xffu)) {
        fi.err = E_BAD_HEADER;
        fi.resume_bit = br_pos(b);
        return BNF_ST_ERROR;
    }
    /* the frame->sample number conversion can also flag UNPARSEABLE (@0x10012372):
     * fixed-number header, no fixed block size yet, STREAMINFO min != max.  That
     * combination is impossible (min != max forces 64-bit numbers), so only the
     * header-field flag remains; the host replays the conversion itself. */
    fi.unparseable = unparseable;
    if (unparseable) {
        fi.err = E_UNPARSEABLE;
        fi.resume_bit = br_pos(b);
        return BNF_ST_ERROR;
    }
    return BNF_ST_OK;
}

DEV uint32_t sub_bps(const bnf_frame_info &fi, uint32_t ch) {
    uint32_t bps = fi.bps;
    if ((fi.assignment == 1 && ch == 1) || (fi.assignment == 2 && ch == 0) || (fi.assignment == 3 && ch == 1)) bps++;
    return bps;
}

/* ------------------------------------------------------------ subframe parse */
enum { T_CONST = 0, T_VERB = 1, T_FIXED = 2, T_LPC = 3 };
enum { P_MMX16 = 0, P_IA32 = 1, P_WIDE = 2 };

struct SubHdr {
    uint32_t type, order, wasted, bps; /* bps after removing wasted bits */
    uint32_t prec;
    int32_t shift;
    uint32_t porder, rice2;
    int32_t cval;
    uint32_t path;
};

/* read_subframe_ @0x10012480 up to (and including) the residual coding header.
 * STORE: warm-ups go to warm[u * WS] and coefficients to coef[u] for u < NW, in loops
 * unrolled to NW (compile-time indices: register arrays stay in registers).  Returns
 * BNF_ST_*; on ERROR sets err and the reader position is where libFLAC stops. */
template <bool STORE, int NW = 32, int WS = 1, class R = BR>
DEV uint32_t parse_subframe_head(R &b, uint32_t bps, uint32_t bs, uint64_t limit, SubHdr &h,
                                 int32_t *warm, int32_t *coef, int32_t &err) {
    uint32_t x = br_read(b, 8);
    uint32_t wflag = x & 1u;
    x &= 0xFEu;
    h.wasted = 0;
    if (wflag) {
        uint32_t u;
        if (!br_unary(b, u, limit)) return BNF_ST_TRUNC;
        h.wasted = u + 1u;
        if (h.wasted > bps) { err = E_UNPARSEABLE; return BNF_ST_ERROR; }
        bps -= h.wasted;
    }
    if (x & 0x80) { err = E_LOST_SYNC; return BNF_ST_ERROR; }
    if (bps > 32) { err = E_UNPARSEABLE; return BNF_ST_ERROR; }
    h.bps = bps;
    h.order = 0;
    h.porder = 0;
    h.rice2 = 0;
    h.path = P_IA32;
    if (x == 0) {
        h.type = T_CONST;
        h.cval = br_read_s(b, bps);
        return BNF_ST_OK;
    }
    if (x == 2) { h.type = T_VERB; return BNF_ST_OK; }
    if (x < 16) { err = E_UNPARSEABLE; return BNF_ST_ERROR; }
    if (x <= 24) {
        h.type = T_FIXED;
        h.order = (x >> 1) & 7u;
    } else if (x < 64) {
        err = E_UNPARSEABLE;
        return BNF_ST_ERROR;
    } else {
        h.type = T_LPC;
        h.order = ((x >> 1) & 31u) + 1u;
    }
    if (STORE) {
#pragma unroll
        for (int u = 0; u < NW; u++)
            if ((uint32_t)u < h.order) warm[u * WS] = br_read_s(b, bps);
        for (uint32_t u = NW; u < h.order; u++) br_read_s(b, bps);
    } else {
        for (uint32_t u = 0; u < h.order; u++) br_read_s(b, bps);
    }
    if (h.type == T_LPC) {
        uint32_t p = br_read(b, 4);
        if (p == 15) { err = E_LOST_SYNC; return BNF_ST_ERROR; }
        h.prec = p + 1;
        h.shift = br_read_s(b, 5);
        if (STORE) {
#pragma unroll
            for (int u = 0; u < NW; u++)
                if ((uint32_t)u < h.order) coef[u] = br_read_s(b, h.prec);
            for (uint32_t u = NW; u < h.order; u++) br_read_s(b, h.prec);
        } else {
            for (uint32_t u = 0; u < h.order; u++) br_read_s(b, h.prec);
        }
        uint32_t ilog = 31u - (uint32_t)__builtin_clz(h.order);
        if (bps + h.prec + ilog <= 32) h.path = (bps <= 16 && h.prec <= 16 && h.order >= 4) ? P_MMX16 : P_IA32;
        else h.path = P_WIDE;
    }
    uint32_t m = br_read(b, 2);
    if (m > 1) { err = E_UNPARSEABLE; return BNF_ST_ERROR; }
    h.rice2 = m;
    h.porder = br_read(b, 4);
    /* read_residual_partitioned_rice_ sanity checks (@0x10012e1e, @0x10012e41) */
    if (h.porder == 0) {
        if (bs < h.order) { err = E_LOST_SYNC; return BNF_ST_ERROR; }
    } else {
        if ((bs >> h.porder) < h.order) { err = E_LOST_SYNC; return BNF_ST_ERROR; }
        if (bs & ((1u << h.porder) - 1u)) { err = E_UNPARSEABLE; return BNF_ST_ERROR; } /* see oracle */
    }
    return br_pos(b) > limit ? BNF_ST_TRUNC : BNF_ST_OK;
}

/* Channel decorrelation (read_frame_ @0x10011a37-0x10011adb), 32-bit wrap. */
DEV void decorrelate(uint32_t as, int32_t &v0, int32_t &v1) {
    if (as == 1) v1 = (int32_t)((uint32_t)v0 - (uint32_t)v1);
    else if (as == 2) v0 = (int32_t)((uint32_t)v0 + (uint32_t)v1);
    else if (as == 3) {
        uint32_t mid = (uint32_t)v0, side = (uint32_t)v1;
        mid = (mid << 1) | (side & 1u);
        v0 = (int32_t)(mid + side) >> 1;
        v1 = (int32_t)(mid - side) >> 1;
    }
}
#endif /* BNF_FRAME_H */
