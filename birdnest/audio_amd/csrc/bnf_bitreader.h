/*
 * bnf_bitreader.h -- the lane bit reader.  Every lane owns an 8-slot ring of 16-byte blocks of
 * its own bitstream in LDS, filled by exec-masked LDS-DMA (global_load_lds_dwordx4) once per
 * 32-sample chunk; a chunk decodes from blocks that landed during the previous chunk, so HBM
 * latency is hidden behind a whole chunk of work and the per-codeword cursor advance is
 * branch-free (one ds_read_b32).  Words outside the landed range are read from global memory
 * directly (rare: jumps, very high bit rates).
 */
#ifndef BNF_BITREADER_H
#define BNF_BITREADER_H
#include "bnf_common.h"

/* ----------------------------------------------------------------- bit reader */
#define RING_MAX 16       /* 16-byte slots per lane (k_parse and k_decode_st use 8) */
#define RING_LANE_DW 256  /* dwords per slot row (64 lanes x 4) */

/* MSB-first bit stream.  Window hi:lo (big-endian words); the cursor is 32-s bits into
 * hi (s in [0,31]; s == 0 means the cursor sits at the start of lo), so the next 32 bits
 * are alignbit(hi, lo, s) for every cursor position.  nx = raw (little-endian) word wi,
 * the next to enter the window; it is re-read from the ring on every advance. */
struct BR {
    const uint32_t *__restrict__ w; /* stream words (16-byte aligned base) */
    uint32_t nw;                    /* words readable (allocation covers nblk*4) */
    uint32_t nblk;                  /* 16-byte blocks readable */
    lds_u32 *ring;                  /* slot 0 of lane 0 (wave-uniform) */
    lds_u32 *lring;                 /* this lane's word-0 entry */
    uint32_t rdepth, wmask;         /* ring slots (power of 2 <= RING_MAX); ring word mask */
    uint32_t wi, s, hi, lo, nx;
    uint32_t vendw, iend;           /* words < vendw landed in the ring; blocks < iend issued */
    uint32_t iend_old;              /* k_decode's 2-deep DMA pipeline: issued two refills ago */
    uint32_t ra, vlim;              /* k_decode_st: ring byte address of word wi (with the lane's bits), vendw - 1 */
    bool stats;
};

DEV void br_init(BR &b, const uint32_t *words, uint64_t nbytes, lds_u32 *ring, uint32_t lane, uint32_t rdepth) {
    b.rdepth = rdepth;
    b.wmask = 4u * rdepth - 1u;
    b.w = words;
    b.nblk = (uint32_t)((nbytes + 15u) >> 4);
    b.nw = b.nblk * 4u;
    b.ring = ring;
    b.lring = ring + lane * 4u;
    b.wi = 2;
    b.s = b.hi = b.lo = b.nx = 0;
    b.vendw = b.iend = 0;
    b.iend_old = 0;
    b.stats = false;
}

DEV void wait_vm() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
/* vmcnt retires in issue order (loads, stores and LDS-DMA together): waiting until at most
 * N are outstanding completes everything older than the youngest N */
template <int N> DEV void wait_vm_but() { asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory"); }
/* the same with a wave-uniform run-time count (vmcnt is an immediate: jump table) */
DEV void wait_vm_n(uint32_t n) {
    switch (__builtin_amdgcn_readfirstlane(min(n, 63u))) {
#define WVN(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
#define WVN8(k) WVN(k) WVN(k + 1) WVN(k + 2) WVN(k + 3) WVN(k + 4) WVN(k + 5) WVN(k + 6) WVN(k + 7)
        WVN8(0) WVN8(8) WVN8(16) WVN8(24) WVN8(32) WVN8(40) WVN8(48) WVN8(56)
#undef WVN8
#undef WVN
    default: break;
    }
}
/* single-wave workgroups: LDS exchange between lanes needs only the LDS queue drained
 * (and the compiler kept from reordering); no s_barrier, no vmcnt drain of stores/DMA */
DEV void lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

DEV uint32_t gword(const BR &b, uint32_t w) { return (w < b.nw) ? b.w[w] : 0u; }
/* ring layout [slot][lane][4 words] (16 bytes per lane per slot, the LDS-DMA dwordx4
 * image); block j lives in slot j % rdepth */
DEV uint32_t ring_off(const BR &b, uint32_t w) { /* dword offset of word w from lring */
    return ((w & (b.wmask & ~3u)) << 6) + (w & 3u);
}
DEV uint32_t ring_word(const BR &b, uint32_t w) { return b.lring[ring_off(b, w)]; }
/* LDS-DMA destination invariant.  A global_load_lds_dwordx4 writes lane l's 16 bytes at
 * (destination base + 16 l); round 2 found that a base that is not 1 KiB aligned writes the
 * wrong LDS bytes with no fault (wrong PCM).  Every ring slot row is one
 * whole 1 KiB image, so the invariant is: ring bases 1 KiB aligned (LDS_DMA_ALIGN on every
 * __shared__ ring) and slot offsets multiples of 1 KiB (the static_asserts below).  Debug
 * builds (-DBNFLAC_DEBUG_ASSERTS) also check every base at run time. */
#define LDS_DMA_ALIGN __attribute__((aligned(1024)))
static_assert(RING_LANE_DW * 4 == 1024, "a ring slot row must be exactly one 1 KiB LDS-DMA image");
DEV void dma_check_base(const lds_u32 *base) {
#ifdef BNFLAC_DEBUG_ASSERTS
    if (((uint32_t)(uintptr_t)base & 1023u) != 0u) __builtin_trap();
#else
    (void)base;
#endif
}
/* One LDS-DMA: 16 bytes per lane to dst + 16 lane.  (Issued as inline asm instead, hidden from
 * the waitcnt pass, it measured 1-2% slower on k_decode_st in round 4.) */
DEV void lds_dma16(const void *g, lds_u32 *dst) {
    dma_check_base(dst);
    __builtin_amdgcn_global_load_lds((gvoid *)g, (lds_void *)dst, 16, 0, 0);
}
DEV void dma_block(const BR &b, uint32_t j, uint32_t slot) { /* one 16-byte block per lane */
    lds_dma16(b.w + (uint64_t)min(j, b.nblk - 1u) * 4u, b.ring + slot * RING_LANE_DW);
}
/* The same with the instruction's immediate offset (one address for consecutive blocks).  The
 * offset moves the LDS destination as well as the global address (measured on gfx950,
 * tools/dbg_glds_off.hip), so the LDS base passed is the slot row minus the offset: the
 * row still receives lane l's 16 bytes at +16 l. */
template <int OFF>
DEV void lds_dma16_off(const void *g, lds_u32 *row) {
    dma_check_base(row); /* the row the data lands in (the base passed is row - OFF / 4) */
    __builtin_amdgcn_global_load_lds((gvoid *)g, (lds_void *)(row - OFF / 4), 16, OFF, 0);
}

/* Issue the blocks this lane will need next (exec-masked LDS-DMA per ring slot).  Blocks
 * issued earlier have landed once the wait returns.  The block of word wi is kept: br_adv
 * re-reads it. */
template <int KEEP = 0> /* KEEP: younger vector-memory ops (PCM stores) that may stay in flight */
DEV void br_refill(BR &b) {
    wait_vm_but<KEEP>();
    b.vendw = b.iend * 4u;
    /* whole 64-byte lines: [iend, first line of the cursor + rdepth); a 4-slot ring (one
     * line) refills from the cursor's block instead */
    const uint32_t need = b.rdepth >= 8u ? ((b.wi >> 2) & ~3u) : (b.wi >> 2);
    const uint32_t lo = max(b.iend, need), hi = need + b.rdepth;
#pragma unroll 1 /* rare path (seeks, landings), inlined at every cursor advance: keep it small */
    for (int s = 0; s < RING_MAX; s++) {
        if ((uint32_t)s >= b.rdepth) break; /* wave-uniform */
        const uint32_t j = lo + (((uint32_t)s - lo) & (b.rdepth - 1u));
        if (j < hi) dma_block(b, j, (uint32_t)s);
    }
    b.iend = max(b.iend, hi);
}

/* Rare path: word wi is not in the landed part of the ring (a jump, or a lane that
 * consumed more than the ring held): wait for what is in flight, refill if still short. */
DEV void br_drained(BR &b) { /* every vector-memory op of this wave has completed (per lane) */
    b.vendw = b.iend * 4u;
    b.iend_old = b.iend;
}
DEV void br_land(BR &b, uint32_t margin = 0) { /* afterwards words wi .. wi + margin have landed */
    STAT(b.stats, 2);
    wait_vm();
    br_drained(b);
    if (b.wi + margin >= b.vendw) {
        br_refill(b);
        wait_vm();
        br_drained(b);
    }
}

/* Blocking seek (subframe starts, skips). */
DEV void br_seek(BR &b, uint64_t bit) {
    b.s = (uint32_t)(0u - bit) & 31u;
    const uint32_t hw = (uint32_t)((bit + b.s) >> 5) - 1u; /* word holding the cursor (-1 at bit 0) */
    b.hi = __builtin_bswap32(gword(b, hw));
    b.lo = __builtin_bswap32(gword(b, hw + 1u));
    b.wi = hw + 2u;
    b.iend = (b.wi >> 2) & ~3u;
    br_refill(b);
    wait_vm();
    br_drained(b);
    b.nx = ring_word(b, b.wi);
}

/* k_decode's refill: a 2-deep pipeline.  Waits only for the DMAs issued two refills ago
 * (vmcnt counts loads, stores and LDS-DMA together and retires them in issue order, so
 * letting the younger q.s_last + q.d_last + q.s_prev ops stay outstanding is exact), marks
 * those blocks landed, and issues the next blocks.  Blocks issued now become readable two
 * chunks later; the ring keeps ~6 blocks ahead of the cursor.  Called by the whole wave
 * (the counts must be wave-uniform); `want` masks the lanes that refill.  A full drain in
 * between (br_land, seek) only completes more, so the counts stay safe without reset. */
struct VmQ {
    uint32_t d_last, s_last, s_prev; /* DMAs of the last refill; stores since it; before it */
};
DEV void br_refill2(BR &b, bool want, VmQ &q, bool nowait = false) {
    if (!nowait) wait_vm_n(q.s_last + q.d_last + q.s_prev); /* nowait: timing ablation 0x200 only */
    if (want) b.vendw = b.iend_old * 4u;
    /* the ring holds rdepth/4 whole lines; a lane whose cursor (word wi) is in the newest
     * line fetches the next line into the oldest line's slots: 4 x 16-byte DMAs hitting
     * one cache line */
    const uint32_t curl = (b.wi >> 2) & ~3u;
    const bool go = want && b.iend <= curl + 4u;
    const uint32_t slot0 = b.iend & (b.rdepth - 1u); /* multiple of 4 */
    uint32_t d = 0;
#pragma unroll
    for (int h = 0; h < RING_MAX / 4; h++) {
        if ((uint32_t)(h * 4) >= b.rdepth) break; /* wave-uniform */
        const bool gh = go && slot0 == (uint32_t)(h * 4);
        if (__any(gh)) { /* wave-uniform: the 4 DMAs below are issued exactly when this holds */
            d += 4;
            if (gh) {
#pragma unroll
                for (int k = 0; k < 4; k++) dma_block(b, b.iend + k, (uint32_t)(h * 4 + k));
            }
        }
    }
    if (want) {
        b.iend_old = b.iend;
        if (go) b.iend += 4u;
    }
    q.s_prev = q.s_last;
    q.s_last = 0;
    q.d_last = d;
}

/* k_decode's refill (1-deep): br_issue, after a chunk's entropy phase, fetches the 16-byte
 * blocks up to rdepth past the block of the cursor word (never that block's slot, which
 * br_adv re-reads), so at least (rdepth - 1) * 16 bytes lie ahead of the cursor; br_wait1,
 * before the next entropy phase, waits for them -- only the PCM stores packed since (at
 * least q.s_last of them, all younger) may stay in flight -- and marks them landed.  The
 * restore and the pack run in between.  A lane that needs more within one chunk lands
 * (br_land). */
DEV void br_wait1(BR &b, VmQ &q) {
    wait_vm_n(q.s_last);
    b.vendw = b.iend * 4u;
    q.s_last = 0;
}
DEV void br_issue(BR &b, bool want) {
    const uint32_t cb = b.wi >> 2;
    const uint32_t lo = max(b.iend, cb), hi = cb + b.rdepth;
#pragma unroll
    for (int k = 0; k < RING_MAX; k++) {
        if ((uint32_t)k >= b.rdepth) break; /* wave-uniform */
        const uint32_t j = lo + (((uint32_t)k - lo) & (b.rdepth - 1u)); /* the block for slot k */
        const bool go = want && j < hi;
        if (__any(go)) {
            if (go) dma_block(b, j, (uint32_t)k);
        }
    }
    if (want) b.iend = max(b.iend, hi);
}

DEV uint64_t br_pos(const BR &b) { return ((uint64_t)(b.wi - 1u) << 5) - b.s; }
DEV uint32_t br_peek(const BR &b) { return __builtin_amdgcn_alignbit(b.hi, b.lo, b.s); }
/* Pending LDS store carried into the next cursor advance (fused decode): issuing it after
 * the window update and before the next ring read keeps every LDS op covered by the next
 * lgkmcnt wait a whole codeword old. */
struct PendW {
    int32_t *at;
    int32_t v;
    bool on;
};
DEV bool any_lane(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; } /* wave-uniform */
/* leading zeros, ~0u for 0 (v_ffbh_u32; asm so the compiler assumes no range).  An asm
 * statement makes hipcc's waitcnt pass wait lgkmcnt(0) before it; the builtin form
 * (x ? clz(x) : ~0u, also one v_ffbh_u32) keeps counted waits but measured 1-2% slower on
 * k_decode_st (round 4) and no different on k_decode_sys. */
DEV uint32_t ffbh(uint32_t x) {
    uint32_t r;
    asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}


template <bool CHECK = true>
DEV void br_adv(BR &b, uint32_t n, PendW *pw = nullptr) { /* n <= 32; branch-free except the rare landing check */
    const int32_t t = (int32_t)b.s - (int32_t)n;
    const bool c = t < 0;
    b.s = (uint32_t)t & 31u;
    b.hi = c ? b.lo : b.hi;
    b.lo = c ? __builtin_bswap32(b.nx) : b.lo;
    b.wi += c ? 1u : 0u;
    if (CHECK && __builtin_expect(any_lane(b.wi >= b.vendw), 0)) br_land(b);
    if (pw && pw->on) *pw->at = pw->v;
    /* issue the ring read after the window update (an artificial data dependency of the
     * address on the new lo), so the wait for the previous word (one codeword old) is not
     * merged with a wait for this one; other instructions stay free to move */
    uint32_t off = ring_off(b, b.wi);
    asm volatile("" : "+v"(off) : "v"(b.lo));
    b.nx = b.lring[off];
}
template <bool CHECK = true>
DEV uint32_t br_read(BR &b, uint32_t n) { /* 0..32 bits */
    uint32_t v = n ? (br_peek(b) >> ((32u - n) & 31u)) : 0u;
    br_adv<CHECK>(b, n);
    return v;
}
template <bool CHECK = true>
DEV int32_t br_read_s(BR &b, uint32_t n) {
    uint32_t v = br_read<CHECK>(b, n);
    uint32_t s = (32u - n) & 31u;
    return (int32_t)(v << s) >> s;
}
DEV void br_skip(BR &b, uint64_t n) {
    if (n <= 32) br_adv(b, (uint32_t)n);
    else br_seek(b, br_pos(b) + n);
}
/* count zeros up to and including the terminating 1 (read_unary_unsigned @0x10001960) */
DEV bool br_unary(BR &b, uint32_t &q, uint64_t limit) {
    uint32_t acc = 0;
    for (;;) {
        uint32_t p = br_peek(b);
        if (p) {
            uint32_t z = (uint32_t)__builtin_clz(p);
            acc += z;
            br_adv(b, z + 1u);
            q = acc;
            return true;
        }
        acc += 32u;
        br_adv(b, 32u);
        if (br_pos(b) > limit) {
            q = acc;
            return false;
        }
    }
}

DEV uint8_t crc8_bytes(const uint8_t *p, uint32_t n) {
    uint8_t c = 0;
    for (uint32_t i = 0; i < n; i++) c = g_crc8_tab[c ^ p[i]];
    return c;
}
#endif /* BNF_BITREADER_H */
