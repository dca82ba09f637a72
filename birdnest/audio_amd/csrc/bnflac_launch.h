/*
 * bnflac_launch.h -- everything the translation units of libbnflac.so say to each other,
 * declared once: the kernels' `ablate` word, the per-TU table/stats entries, the decode
 * launchers of the kernel TUs and the entry points of the parse TU (-DBNF_K_PARSE) that bnflac_runtime.cpp
 * and bnflac_reader.cpp call.  Every file that defines or calls one of these includes this
 * header, so the compiler checks each definition against its declaration (all of them are
 * extern "C" and hidden: a drifted prototype would still link).
 */
#ifndef BNFLAC_LAUNCH_H
#define BNFLAC_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bnf_health.h"
#include "bnf_mel.h"
#include "bnf_resample.h"
#include "bnf_resync.h"
#include "bnf_select.h"
#include "bnflac_device.h"

/* The batched chain's control words (bnf_ms_scratch.ctl: bad table, candidates found, candidates
 * used) and the key bit of a valid frame start, as the kernels of two translation units read them. */
enum { BNF_MS_BAD = 0, BNF_MS_NCAND = 1, BNF_MS_N = 2, BNF_MS_CTL_WORDS = 4 };
#define BNF_MS_KEY_OK 0x10000u

/* ------------------------------------------------------------- the `ablate` word
 * Every decode and parse kernel takes one uint32_t `ablate`.  It carries two disjoint fields:
 *
 *  - ablation bits (BNF_ABLATE_*), set by the user: bnflac_debug_set_ablate, or BNFLAC_ABLATE in
 *    the environment (read once, at the first launch).  "exact" bits are A/B switches between
 *    two implementations with identical PCM and records; "timing" bits skip work, and results
 *    are wrong while one is set;
 *  - mode bits (BNF_MODE_*), set by the launchers only: which of an instance's jobs a launch
 *    does.  Never a user setting.
 *
 * A launcher passes (bnf_ablate_flags() & BNF_ABLATE_K_<family>) | (mode & BNF_MODE_K_<family>), so a user
 * bit reaches only the kernels that define it and can never be read as a mode.  (Two of
 * k_decode_sys's ablation bits have the numeric values of two of k_decode<W>'s mode bits; the
 * family masks keep them apart.)
 *
 * This is the only list of the bits: include/bnflac.h, INTEGRATION.md and DESIGN.md point here. */

/* timing: no frame CRC-16 (k_decode<W>, k_decode_st, k_decode_sw, k_decode_sys) */
#define BNF_ABLATE_NO_CRC16 0x1u
/* timing: no PCM stores (k_decode<W>, k_decode_st, k_decode_sw, k_decode_sys) */
#define BNF_ABLATE_NO_STORE 0x2u
/* timing: no restore (k_decode<W>, k_decode_sys: residuals stay in the rows; k_decode_st, k_decode_sw: every
 * chunk through the generic steps) */
#define BNF_ABLATE_NO_RESTORE 0x4u
/* timing: no Rice decode (k_decode<W>, k_decode_st, k_decode_sw, k_decode_sys) */
#define BNF_ABLATE_NO_RICE 0x8u
/* timing: k_parse does not walk the subframes (and hands no CRC-16 prefix over) */
#define BNF_ABLATE_NO_WALK 0x10u
/* timing: k_parse's residual walk never refills its ring */
#define BNF_ABLATE_NO_WALK_REFILL 0x20u
/* exact: k_decode_st keeps no running CRC-16 of channel 1 in its chunk loop; the tail reads
 * channel 1 again from k_parse's prefix on */
#define BNF_ABLATE_NO_STFOLD 0x40u
/* exact: the debug event counters and phase timers count (bnflac_debug_stats; k_decode<W>,
 * k_decode_st, k_decode_sys) */
#define BNF_ABLATE_STATS 0x100u
/* exact: k_decode_st is not launched and k_decode<8> takes every stereo frame (the launcher
 * of k_decode_st and k_decode<W> read it) */
#define BNF_ABLATE_NO_ST 0x400u
/* exact: every k_decode<W> chunk through the generic path, none through the fused one */
#define BNF_ABLATE_NO_FUSED 0x800u
/* exact: k_decode<W>'s 24-bit FLACFileReader wide flush (pack_wide24) off */
#define BNF_ABLATE_NO_WIDE24 0x2000u
/* exact, host only: k_decode_sw is not launched (bnf_launch_decode) */
#define BNF_ABLATE_NO_SW 0x10000u
/* exact: k_decode_sys restores every wave with the mixed-width variant (PM_MIXED) */
#define BNF_ABLATE_SYS_MIXED 0x40000u
/* timing: k_decode_sys's producer never refills ahead, it only lands */
#define BNF_ABLATE_SYS_LAND_ONLY 0x80000u
/* exact, host only: the W = 8 instance as one launch (bnf_launch_decode) */
#define BNF_ABLATE_NO_W8SPLIT 0x100000u
/* exact: k_decode_sys's producer takes no fast run, residual by residual */
#define BNF_ABLATE_SYS_NO_RUN 0x200000u
/* exact: k_decode_sys packs every chunk with the generic sys_pack */
#define BNF_ABLATE_SYS_NO_PACK_FAST 0x400000u
/* exact: k_parse's residual walk refills block by block (br_refill) on every refill */
#define BNF_ABLATE_PARSE_BLKREFILL 0x800000u
/* exact: k_decode_sys's producer refills every half chunk, 4 deep, instead of once per chunk */
#define BNF_ABLATE_SYS_REFILL_HALF 0x1000000u
/* timing: k_decode_st / k_decode_sw aim their PCM stores at a 513 KB window at the start of
 * the output (an L2-resident footprint); ignored when out_bytes < 1 MiB */
#define BNF_ABLATE_HOT_WINDOW 0x10000000u
/* exact: k_decode_sw's FLACFileReader line flush off */
#define BNF_ABLATE_SW_NO_LINE 0x20000000u

/* Mode bit: the lane kernel decodes only the frames k_decode_sys handed back (BNF_FL_WAVE_REDO). */
#define BNF_MODE_WREDO 0x4000u
/* Mode bit: k_decode_sw ran before the other lane kernels (they take its SW frames only when
 * it handed them back). */
#define BNF_MODE_SW 0x8000u
/* Mode bit: k_decode_list -- the frames of a device list (k_decode_sys's hand-backs), every
 * class, decoded by this instance (no class split, stereo fast-path frames included). */
#define BNF_MODE_LIST 0x20000u
/* Mode bits of the W = 8 instance when its two jobs run as two launches (bnf_launch_decode):
 * NOST -- the narrow non-stereo frames only (the decode order's class 1; beside k_decode_st,
 * so it never reads a stereo frame's hand-back bit); STREDO -- only the stereo frames
 * k_decode_st handed back (class 0; after it). */
#define BNF_MODE_NOST 0x40000u
#define BNF_MODE_STREDO 0x80000u
/* Mode bit: k_decode_seg -- the W = 32 instance also takes the W16 class's blocks. */
#define BNF_MODE_SEG 0x80000000u

/* Per kernel family: the mode bits its launchers may set and the ablation bits it reads. */
#define BNF_MODE_K_PARSE 0u
#define BNF_ABLATE_K_PARSE (BNF_ABLATE_NO_WALK | BNF_ABLATE_NO_WALK_REFILL | BNF_ABLATE_PARSE_BLKREFILL)
#define BNF_MODE_K_DECODE (BNF_MODE_WREDO | BNF_MODE_SW | BNF_MODE_LIST | BNF_MODE_NOST | BNF_MODE_STREDO | BNF_MODE_SEG)
#define BNF_ABLATE_K_DECODE                                                                                      \
    (BNF_ABLATE_NO_CRC16 | BNF_ABLATE_NO_STORE | BNF_ABLATE_NO_RESTORE | BNF_ABLATE_NO_RICE | BNF_ABLATE_STATS | \
     BNF_ABLATE_NO_ST | BNF_ABLATE_NO_FUSED | BNF_ABLATE_NO_WIDE24)
#define BNF_MODE_K_DECODE_ST (BNF_MODE_WREDO | BNF_MODE_SW)
#define BNF_ABLATE_K_DECODE_ST                                                                                      \
    (BNF_ABLATE_NO_CRC16 | BNF_ABLATE_NO_STORE | BNF_ABLATE_NO_RESTORE | BNF_ABLATE_NO_RICE | BNF_ABLATE_NO_STFOLD | \
     BNF_ABLATE_STATS | BNF_ABLATE_NO_ST | BNF_ABLATE_HOT_WINDOW)
#define BNF_MODE_K_DECODE_SW BNF_MODE_WREDO
#define BNF_ABLATE_K_DECODE_SW                                                                                       \
    (BNF_ABLATE_NO_CRC16 | BNF_ABLATE_NO_STORE | BNF_ABLATE_NO_RESTORE | BNF_ABLATE_NO_RICE | BNF_ABLATE_HOT_WINDOW | \
     BNF_ABLATE_SW_NO_LINE)
#define BNF_MODE_K_DECODE_SYS 0u
#define BNF_ABLATE_K_DECODE_SYS                                                                                  \
    (BNF_ABLATE_NO_CRC16 | BNF_ABLATE_NO_STORE | BNF_ABLATE_NO_RESTORE | BNF_ABLATE_NO_RICE | BNF_ABLATE_STATS | \
     BNF_ABLATE_SYS_MIXED | BNF_ABLATE_SYS_LAND_ONLY | BNF_ABLATE_SYS_NO_RUN | BNF_ABLATE_SYS_NO_PACK_FAST |     \
     BNF_ABLATE_SYS_REFILL_HALF)
/* every launcher-owned bit */
#define BNF_MODE_MASK (BNF_MODE_K_PARSE | BNF_MODE_K_DECODE | BNF_MODE_K_DECODE_ST | BNF_MODE_K_DECODE_SW | BNF_MODE_K_DECODE_SYS)

static_assert(!(BNF_ABLATE_K_PARSE & BNF_MODE_K_PARSE), "k_parse: an ablation bit is a mode bit");
static_assert(!(BNF_ABLATE_K_DECODE & BNF_MODE_K_DECODE), "k_decode<W>: an ablation bit is a mode bit");
static_assert(!(BNF_ABLATE_K_DECODE_ST & BNF_MODE_K_DECODE_ST), "k_decode_st: an ablation bit is a mode bit");
static_assert(!(BNF_ABLATE_K_DECODE_SW & BNF_MODE_K_DECODE_SW), "k_decode_sw: an ablation bit is a mode bit");
static_assert(!(BNF_ABLATE_K_DECODE_SYS & BNF_MODE_K_DECODE_SYS), "k_decode_sys: an ablation bit is a mode bit");
static_assert(!((BNF_ABLATE_NO_SW | BNF_ABLATE_NO_W8SPLIT) & BNF_MODE_MASK), "a host ablation bit is a mode bit");

/* ------------------------------------------------------------- per-TU tables and counters
 * Each kernel TU is its own code object with its own __constant__ CRC tables and g_stats
 * (bnf_common.h defines the pair once; every TU instantiates it).  The parse TU keeps the table of
 * these entries and loops over it in bnf_upload_tables and bnf_stats. */
typedef struct {
    hipError_t (*upload_tables)(const uint8_t *crc8, const uint16_t *crc16x8, const uint16_t *xpow);
    hipError_t (*stats)(uint64_t *out16, int reset); /* adds the TU's g_stats to out16 */
} bnf_tu_ops;
/* (not const: hipcc would emit a const object with a constant initializer into the device code
 * object as well, where the host functions it points to do not exist) */
extern bnf_tu_ops bnf_ops_decode_w8, bnf_ops_decode_w16, bnf_ops_decode_w32, bnf_ops_decode_st_fd, bnf_ops_decode_st_any,
    bnf_ops_decode_sw, bnf_ops_decode_sys;

extern "C" {
/* the user's ablation bits (the one g_ablate, in the parse TU) */
uint32_t bnf_ablate_flags(void);
void bnf_set_ablate(uint32_t v);

/* ------------------------------------------------------------- decode launchers (kernel TUs)
 * perm: the decode order or nullptr; mode: BNF_MODE_* of the launch.
 * seg: k_order's bucket ends (W = 16 / 32 only, with perm): blocks outside the class leave first */
#define BNF_DECODE_ARGS                                                                                              \
    const uint32_t *words, uint64_t nbytes, uint32_t nframes, bnf_stream_params sp, uint32_t chn_lanes, int fmt,   \
        uint8_t *out, uint64_t out_bytes, bnf_frame_info *info
hipError_t bnf_launch_decode_w8(BNF_DECODE_ARGS, const uint32_t *perm, uint32_t mode, const uint32_t *seg, hipStream_t s);
hipError_t bnf_launch_decode_w16(BNF_DECODE_ARGS, const uint32_t *perm, uint32_t mode, const uint32_t *seg, hipStream_t s);
hipError_t bnf_launch_decode_w32(BNF_DECODE_ARGS, const uint32_t *perm, uint32_t mode, const uint32_t *seg, hipStream_t s);
/* k_decode_sys's hand-back list (W = 32: every order); nframes bounds the list */
hipError_t bnf_launch_decode_list(BNF_DECODE_ARGS, const uint32_t *list, uint32_t mode, hipStream_t s);
/* the W16 + W32 segment of the decode order (k_decode_seg; perm and seg required) */
hipError_t bnf_launch_decode_seg(BNF_DECODE_ARGS, const uint32_t *perm, uint32_t mode, const uint32_t *seg, hipStream_t s);
/* stereo fast path (k_decode_st<FLACDECODER> / the other layouts); launched before k_decode<8>
 * (it hands frames back to it).  crcp: k_parse's CRC-16 hand-off or nullptr */
hipError_t bnf_launch_decode_st_fd(BNF_DECODE_ARGS, const uint32_t *perm, uint32_t mode, const uint32_t *crcp, hipStream_t s);
hipError_t bnf_launch_decode_st_any(BNF_DECODE_ARGS, const uint32_t *perm, uint32_t mode, const uint32_t *crcp, hipStream_t s);
/* stereo frames above 16 bits; launched before k_decode<8>/<16>/<32> (it hands frames back to k_decode<16>) */
hipError_t bnf_launch_decode_sw(BNF_DECODE_ARGS, const uint32_t *perm, uint32_t mode, const uint32_t *crcp, hipStream_t s);
/* redo: [0] hand-back count (zeroed by the caller), [4..] the frames handed back */
hipError_t bnf_launch_decode_sys(BNF_DECODE_ARGS, const uint32_t *perm, uint32_t *redo, uint32_t mode, hipStream_t s);

/* ------------------------------------------------------------- the parse TU (parse, index, dispatch): entry points */
hipError_t bnf_upload_tables(const uint8_t *crc8, const uint16_t *crc16x8, const uint16_t *xpow);
hipError_t bnf_stats(uint64_t *out16, int reset);
hipError_t bnf_launch_sync_scan(const uint8_t *d, uint64_t n, uint32_t *d_block_counts, uint32_t *d_total,
                                uint64_t *d_out, uint32_t cap, hipStream_t s);
uint32_t bnf_scan_blocks(uint64_t n);
hipError_t bnf_launch_scan_u32(uint32_t *v, uint32_t n, uint32_t *total, hipStream_t s);
int bnf_crc_mode(void);
void bnf_set_crc_mode(int mode);    /* -1: env */
void bnf_set_decode_sys(int mode);  /* -1: auto */
void bnf_set_parse_wave(int mode);  /* -1: auto */
uint64_t bnf_decode_seg_launches(void);
/* The route of the process's last bnf_launch_decode and bnf_launch_parse (plain host atomics the
 * launchers write; include/bnflac.h, bnflac_debug_last_route, has the same layout). */
enum {
    BNF_ROUTE_DECODE = 0,     /* BNF_RT_* of the decode */
    BNF_ROUTE_HIST = 1,       /* 4 words: SideQ::cls as the decode read it (with BNF_RT_HIST) */
    BNF_ROUTE_NDECODE = 5,    /* bnf_launch_decode calls that launched something */
    BNF_ROUTE_PARSE = 6,      /* BNF_RT_PARSE_* */
    BNF_ROUTE_CM = 7,         /* the hand-off mode launched: 0, 1 or 2 */
    BNF_ROUTE_NPARSE = 8,     /* bnf_launch_parse calls that launched something */
    BNF_ROUTE_PARSE_HIST = 9, /* 3 words: cls[0..2] as the parse read them (with BNF_RT_PARSE_HIST) */
    BNF_ROUTE_WORDS = 12
};
#define BNF_RT_SYS 1u         /* k_decode_sys, then k_decode_list */
#define BNF_RT_FORK_BEFORE 2u /* side grids forked before k_decode_st */
#define BNF_RT_FORK_AFTER 4u  /* side grids forked after k_decode_st */
#define BNF_RT_SERIAL 8u      /* the W16 / W32 grids on the caller's stream */
#define BNF_RT_SEG_ONLY 16u   /* k_decode_seg instead of the W16 / W32 grids */
#define BNF_RT_W8SPLIT 32u    /* k_decode<8> as two launches */
#define BNF_RT_SW 64u         /* k_decode_sw ran first */
#define BNF_RT_HIST 128u      /* the decode read the history words */
#define BNF_RT_PARSE_WAVE 1u  /* k_parse_wave ran (no hand-off) */
#define BNF_RT_PARSE_HIST 2u  /* the parse consulted the history for its hand-off mode */
void bnf_last_route(uint32_t *out); /* BNF_ROUTE_WORDS words */
hipError_t bnf_parse_wave_stats(uint64_t *out8, int reset);
/* words: 16-byte aligned; the allocation must cover round_up(nbytes, 16) bytes.
 * order: nullptr, or 256 + nframes words of device scratch for the frame order (k_order_*);
 * crcp: nullptr, or k_parse's CRC-16 hand-off for these frames (8 words per frame) */
hipError_t bnf_launch_parse(const uint32_t *words, uint64_t nbytes, const uint64_t *frame_offs, uint32_t nframes,
                            bnf_stream_params sp, const uint64_t *out_sample_in, uint64_t base_sample,
                            bnf_frame_info *info, uint32_t *order, uint32_t *crcp, bool *handed, hipStream_t s);
hipError_t bnf_launch_decode(const uint32_t *words, uint64_t nbytes, uint32_t nframes, bnf_stream_params sp,
                             uint32_t chn_lanes, int fmt, uint8_t *out, uint64_t out_bytes, bnf_frame_info *info,
                             uint32_t *order, const uint32_t *crcp, hipStream_t s);
hipError_t bnf_launch_fill_bad(const bnf_frame_info *info, uint32_t nframes, bnf_stream_params sp, int fmt,
                               uint8_t *out, uint64_t out_bytes, hipStream_t s);
hipError_t bnf_launch_chain(const uint8_t *bytes, uint64_t nbytes, const uint64_t *cand, uint32_t ncand,
                            const bnf_frame_info *info, uint64_t first_off, bnf_stream_params sp, uint32_t *gap_crc,
                            int32_t *jump, uint32_t levels, uint32_t *mark, uint32_t *pos, uint64_t *bs, uint8_t *small,
                            uint64_t *d_offs, uint64_t *d_os, bnf_frame_info *d_info, uint32_t cap, uint32_t *nframes,
                            hipStream_t s);
hipError_t bnf_launch_chain_streams(const uint8_t *bytes, uint64_t nbytes, const bnf_stream_desc *sd, uint32_t nstreams,
                                    bnf_stream_params sp, uint32_t cand_cap, bnf_ms_scratch w, uint64_t *d_offs,
                                    uint64_t *d_os, bnf_frame_info *d_info, uint32_t cap, uint32_t *d_sf, uint64_t *d_ss,
                                    uint32_t *d_status, hipStream_t s);
/* The two leading parts of bnf_launch_chain_streams, which the resync chain shares with it.
 * front: the scratch presets and steps 1-3 (candidates, owners, records, keys, w.jump[0, C) = the
 * CRC-16 successors, w.head, the heads marked in w.mark).  jump: step 4, the pointer doubling
 * over whatever successor array w.jump[0, C) holds, growing w.mark along it. */
hipError_t bnf_launch_chain_front(const uint8_t *bytes, uint64_t nbytes, const bnf_stream_desc *sd, uint32_t nstreams,
                                  bnf_stream_params sp, uint32_t cand_cap, bnf_ms_scratch w, hipStream_t s);
hipError_t bnf_launch_chain_jump(uint32_t cand_cap, bnf_ms_scratch w, hipStream_t s);

/* ------------------------------------------------------------- bnflac_resync.hip (no tables, no g_stats, no ablate word)
 * k_rs_*: the rule of bnf_resync.h after bnf_launch_chain_front, on the same scratch w plus r (carved
 * by bnf_resync_carve from memory of bnf_resync_scratch_bytes(cand_cap, nstreams) bytes, 16-byte
 * aligned).  d_offs, d_os, d_info may be nullptr when cap is 0, d_os, d_info, d_ss and d_resync at
 * any time.  r.ct keeps the candidate table of the call (bnflac_debug_index_candidates). */
typedef struct {
    bnf_index_cand *ct;                                        /* C */
    uint64_t *p, *va, *vb, *vs, *gapv, *lv, *rc, *sc, *rp, *sq; /* C + 1 each */
    uint64_t *bsum;                                            /* max(C, S) / 1024 + 2 */
    int32_t *ext;                                              /* C */
    uint32_t *why;                                             /* C */
    int32_t *cut;                                              /* S */
    uint32_t *segs, *rflags;                                   /* S each */
    uint64_t *gapc, *base;                                     /* S each */
    uint64_t *acc;                                             /* 2: placeholders, status bits */
} bnf_rs_scratch;
uint64_t bnf_resync_scratch_bytes(uint32_t cand_cap, uint32_t nstreams);
bnf_rs_scratch bnf_resync_carve(void *mem, uint32_t cand_cap, uint32_t nstreams);
hipError_t bnf_launch_chain_streams_resync(const uint8_t *bytes, uint64_t nbytes, const bnf_stream_desc *sd,
                                           uint32_t nstreams, bnf_stream_params sp, uint32_t cand_cap, bnf_ms_scratch w,
                                           bnf_rs_scratch r, uint64_t *d_offs, uint64_t *d_os, bnf_frame_info *d_info,
                                           uint32_t cap, uint32_t *d_sf, uint64_t *d_ss, bnf_resync_rec *d_resync,
                                           uint32_t *d_status, hipStream_t s);

/* ------------------------------------------------------------- bnflac_md5.hip (no tables, no g_stats, no ablate word)
 * k_md5_streams: stream s is the sample frames [bounds[s], bounds[s + 1]) of pcm, `unit` bytes
 * each.  src 0: those bytes are the MD5 message; src 1..4: they are int32 samples and the message
 * is the low src bytes of each.  Zeroes status (4 words) on s, then launches. */
hipError_t bnf_launch_md5_streams(const uint8_t *pcm, uint64_t pcm_bytes, uint32_t unit, uint32_t src,
                                  const uint64_t *bounds, uint32_t nstreams, const uint8_t *expected, uint8_t *md5,
                                  uint32_t *verdict, uint32_t *status, hipStream_t s);

/* ------------------------------------------------------------- bnflac_scan.hip (no tables, no g_stats, no ablate word)
 * k_scan_streams: the metadata walk (bnf_metadata.h) of the streams sd[0, nstreams) of bytes.
 * Writes first_offset and total_samples of every sd entry, and one record / 16 md5sum bytes per
 * stream where meta / md5 are not nullptr.  expect: nullptr, or the parameters a kept stream
 * has (host memory; copied).  Zeroes status (4 words) on s, then launches. */
hipError_t bnf_launch_scan_streams(const uint8_t *bytes, uint64_t nbytes, bnf_stream_desc *sd, uint32_t nstreams,
                                   const bnf_stream_params *expect, bnf_stream_meta *meta, uint8_t *md5,
                                   uint32_t *status, hipStream_t s);

/* ------------------------------------------------------------- bnflac_select.hip (no tables, no g_stats, no ablate word)
 * k_sel_*: the rule of bnf_select.h over the tables of bnf_launch_chain_streams (offsets and
 * sel_offsets may be nullptr; info and sel_info 16-byte aligned).  scratch: device memory of
 * bnf_select_scratch_bytes(nstreams) bytes, 16-byte aligned.  Writes every status word. */
uint64_t bnf_select_scratch_bytes(uint32_t nstreams);
hipError_t bnf_launch_select_ranges(const uint64_t *offsets, const bnf_frame_info *info, uint32_t cap, const uint32_t *sf,
                                    const uint64_t *ss, uint32_t nstreams, const bnf_sample_range *ranges,
                                    uint64_t *sel_offsets, bnf_frame_info *sel_info, uint32_t sel_cap, uint32_t *sel_frames,
                                    uint64_t *sel_samples, bnf_window *windows, uint32_t *status, void *scratch,
                                    hipStream_t s);
/* k_win_*: the same selection per window request (bnf_select_request), outputs sized by nwindows.
 * scratch: bnf_select_windows_scratch_bytes(nwindows) bytes, 16-byte aligned.  Writes every status word. */
uint64_t bnf_select_windows_scratch_bytes(uint32_t nwindows);
hipError_t bnf_launch_select_windows(const uint64_t *offsets, const bnf_frame_info *info, uint32_t cap, const uint32_t *sf,
                                     const uint64_t *ss, uint32_t nstreams, const bnf_window_request *requests,
                                     uint32_t nwindows, uint64_t *sel_offsets, bnf_frame_info *sel_info, uint32_t sel_cap,
                                     uint32_t *sel_frames, uint64_t *sel_samples, bnf_window *windows, uint32_t *status,
                                     void *scratch, hipStream_t s);
/* k_shr_*: the requests of k_win_* with every frame selected once (bnf_select_windows_shared_host):
 * records and offsets by rank, windows that point into the shared compact PCM, win_sel_first (may be
 * nullptr) the rank of each window's first frame, totals = {frames, samples}.  scratch:
 * bnf_select_shared_scratch_bytes(cap, nwindows) bytes, 16-byte aligned: 32 bytes, 16 per position of
 * [0, cap] and 16 per 1,024 positions, nothing per window (and 32 bytes when nwindows is 0).  Writes
 * every status word. */
uint64_t bnf_select_shared_scratch_bytes(uint32_t cap, uint32_t nwindows);
hipError_t bnf_launch_select_windows_shared(const uint64_t *offsets, const bnf_frame_info *info, uint32_t cap,
                                            const uint32_t *sf, const uint64_t *ss, uint32_t nstreams,
                                            const bnf_window_request *requests, uint32_t nwindows, uint64_t *sel_offsets,
                                            bnf_frame_info *sel_info, uint32_t sel_cap, bnf_window *windows,
                                            uint32_t *win_sel_first, uint64_t *totals, uint32_t *status, void *scratch,
                                            hipStream_t s);
/* k_gather_ranges: row s = rows + s * row_bytes gets min(windows[s].nsamples, row_samples) sample
 * frames of `stride` bytes from pcm + windows[s].pcm_first * stride, then zeros up to row_samples
 * frames.  pcm 16-byte aligned, its allocation at least round_up(pcm_bytes, 16) bytes.  Zeroes
 * status (4 words) on s, then launches. */
hipError_t bnf_launch_gather_ranges(const uint8_t *pcm, uint64_t pcm_bytes, uint32_t stride, const bnf_window *windows,
                                    uint32_t nstreams, uint32_t row_samples, uint64_t row_bytes, uint8_t *rows,
                                    uint32_t *status, hipStream_t s);

/* ------------------------------------------------------------- bnflac_f32.hip (no tables, no g_stats, no ablate word)
 * k_gather_f32: the rule of bnf_pcm_f32.h.  Plane c of stream s = out + (s * planes + c) *
 * plane_pitch floats (planes = 1 with BNF_F32_MONO in flags, else channels) gets
 * min(windows[s].nsamples, row_samples) normalised samples from pcm + windows[s].pcm_first * stride
 * (channel c at c * unit, unit = stride / channels in 2..4), then +0.0f up to row_samples.  pcm and
 * out 16-byte aligned, pcm's allocation at least round_up(pcm_bytes, 16) bytes.  Zeroes status
 * (4 words) on s, then launches. */
hipError_t bnf_launch_gather_f32(const uint8_t *pcm, uint64_t pcm_bytes, uint32_t stride, uint32_t unit, uint32_t bps,
                                 uint32_t channels, uint32_t flags, const bnf_window *windows, uint32_t nstreams,
                                 uint32_t row_samples, uint64_t plane_pitch, float *out, uint32_t *status, hipStream_t s);

/* ------------------------------------------------------------- bnflac_resample.hip (no tables, no g_stats, no ablate word)
 * k_gather_f32_rs: the rule of bnf_resample.h.  The planes of k_gather_f32, row_out floats each, hold
 * the windows filtered to another rate: spec (read here, on the host; refused with
 * hipErrorInvalidValue when bnf_rsmp_spec_refusal names a cause) and its table taps of spec->up *
 * spec->taps floats on the device, 16-byte aligned like pcm and out.  Zeroes status (4 words) on s,
 * then launches with the dynamic LDS the table needs. */
hipError_t bnf_launch_gather_f32_rs(const uint8_t *pcm, uint64_t pcm_bytes, uint32_t stride, uint32_t unit, uint32_t bps,
                                    uint32_t channels, uint32_t flags, const bnf_window *windows, uint32_t nstreams,
                                    const bnf_rsmp_spec *spec, const float *taps, uint32_t row_out, uint64_t plane_pitch,
                                    float *out, uint32_t *status, hipStream_t s);

/* ------------------------------------------------------------- bnflac_mel.hip (no tables, no g_stats, no ablate word)
 * k_gather_mel: the rule of bnf_mel.h.  Per window and plane, rows of row_frames floats frame_pitch
 * apart: the power spectrum or the band sums of the window's STFT frames.  spec is read here, on the
 * host (hipErrorInvalidValue when bnf_mel_spec_refusal names a cause or bands is missing); tab
 * (window, twiddles, weights; 16-byte aligned like pcm) and bands are device tables.  Zeroes status
 * (4 words) on s, then launches with the dynamic LDS bnf_mel_plan_of names. */
hipError_t bnf_launch_gather_mel(const uint8_t *pcm, uint64_t pcm_bytes, uint32_t stride, uint32_t unit, uint32_t bps,
                                 uint32_t channels, uint32_t flags, const bnf_window *windows, uint32_t nstreams,
                                 const bnf_mel_spec *spec, const float *tab, const uint32_t *bands, uint32_t row_frames,
                                 uint64_t frame_pitch, float *out, uint32_t *status, hipStream_t s);

/* ------------------------------------------------------------- bnflac_health.hip (no tables, no g_stats, no ablate word)
 * k_hl_*: the rule of bnf_health.h over the records of a decoded selection (sel_info 16-byte aligned),
 * its window table and the position of each window's first record.  requests, streams and
 * stream_samples are all nullptr or all given.  scratch: bnf_window_health_scratch_bytes(sel_cap,
 * nwindows) bytes, 16-byte aligned: 24 bytes per position of [0, sel_cap) and 24 per 1,024 positions
 * plus 24 (24 bytes when nwindows is 0).  Zeroes status (4 words) on s, then launches. */
uint64_t bnf_window_health_scratch_bytes(uint32_t sel_cap, uint32_t nwindows);
hipError_t bnf_launch_window_health(const bnf_frame_info *sel_info, uint32_t sel_cap, const bnf_window *windows,
                                    const uint32_t *first, uint32_t nwindows, const bnf_window_request *requests,
                                    const bnf_stream_desc *streams, const uint64_t *stream_samples, uint32_t nstreams,
                                    bnf_window_health *health, uint32_t *status, void *scratch, hipStream_t s);
} /* extern "C" */

#endif
