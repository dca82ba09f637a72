/*
 * bnf_metadata.h -- the metadata walk of bnflac_scan_streams: from a stream's first byte to the
 * byte after its last metadata block, STREAMINFO taken on the way.  One __host__ __device__
 * function over a byte accessor: k_scan_streams (bnflac_scan.hip, one lane per stream) and
 * bnflac_scan_stream_host (bnflac_runtime.cpp) are the same code.
 *
 * The rule is strict where libFLAC's find_metadata_ is not: an optional ID3v2 tag at byte 0
 * (skip_id3v2_tag_), then "fLaC" exactly there, then the blocks.  find_metadata_ also steps
 * over junk byte by byte towards the marker or a frame sync, a walk with no bound per stream
 * and a LOST_SYNC error on the way; those streams get NO_MARKER here and go to the stream API.
 *
 * Reads: a byte is loaded only after its index was checked against n, so nothing outside the
 * stream's [begin, end) is read and no result depends on what follows a cut.  The loads of one
 * step (the tag header, the marker, a block header, STREAMINFO's 34 bytes) are independent of
 * each other and issued together; the steps form the chain: tag? -> marker -> block header
 * (-> STREAMINFO) -> next block header ...
 */
#ifndef BNF_METADATA_H
#define BNF_METADATA_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bnflac_device.h"

/* b(i): byte i of the stream, i < n */
struct bnf_bytes {
    const uint8_t *p;
    __host__ __device__ uint32_t operator()(uint64_t i) const { return p[i]; }
};

/* What the walk found.  Everything but status, flags, nblocks and id3_bytes is meaningful only
 * when status is BNF_SCAN_OK. */
typedef struct {
    uint32_t status, flags, nblocks, id3_bytes;
    uint32_t min_blocksize, max_blocksize, min_framesize, max_framesize;
    uint32_t sample_rate, channels, bps;
    uint64_t total_samples;
    uint32_t md5[4]; /* the 16 md5sum bytes, little-endian words */
    uint64_t p;      /* bytes in front of the first frame */
} bnf_meta_walk;

template <class Bytes>
__host__ __device__ inline uint32_t bnf_metadata_walk(const Bytes &b, uint64_t n, bnf_meta_walk &w) {
    w.status = BNF_SCAN_OK;
    w.flags = w.nblocks = w.id3_bytes = 0;
    w.min_blocksize = w.max_blocksize = w.min_framesize = w.max_framesize = 0;
    w.sample_rate = w.channels = w.bps = 0;
    w.total_samples = 0;
    w.md5[0] = w.md5[1] = w.md5[2] = w.md5[3] = 0;
    w.p = 0;
    uint64_t p = 0;
    if (n >= 3) { /* skip_id3v2_tag_: "ID3", version (2), flags (1), four 7-bit size bytes */
        const uint32_t t0 = b(0), t1 = b(1), t2 = b(2);
        if (t0 == 'I' && t1 == 'D' && t2 == '3') {
            if (n < 10) return w.status = BNF_SCAN_TRUNCATED;
            const uint32_t s0 = b(6), s1 = b(7), s2 = b(8), s3 = b(9);
            p = 10u + (((s0 & 0x7fu) << 21) | ((s1 & 0x7fu) << 14) | ((s2 & 0x7fu) << 7) | (s3 & 0x7fu));
            w.flags |= BNF_META_ID3;
            w.id3_bytes = (uint32_t)p;
            if (p > n) return w.status = BNF_SCAN_TRUNCATED;
        }
    }
    if (p + 4 > n) return w.status = BNF_SCAN_NO_MARKER;
    {
        const uint32_t m0 = b(p), m1 = b(p + 1), m2 = b(p + 2), m3 = b(p + 3);
        if (m0 != 'f' || m1 != 'L' || m2 != 'a' || m3 != 'C') return w.status = BNF_SCAN_NO_MARKER;
    }
    p += 4;
    bool have = false;
    for (;;) {
        if (w.nblocks == BNF_SCAN_MAX_BLOCKS) return w.status = BNF_SCAN_TOO_MANY_BLOCKS;
        if (p + 4 > n) return w.status = BNF_SCAN_TRUNCATED;
        const uint32_t h0 = b(p), h1 = b(p + 1), h2 = b(p + 2), h3 = b(p + 3);
        const uint32_t type = h0 & 0x7fu, len = (h1 << 16) | (h2 << 8) | h3;
        w.nblocks++;
        if (type == 0) { /* STREAMINFO, field by field as read_metadata_ takes it; a later one overwrites */
            if (len < 34) return w.status = BNF_SCAN_NO_STREAMINFO;
            if (p + 38 > n) return w.status = BNF_SCAN_TRUNCATED;
            uint32_t si[34];
#pragma unroll
            for (int i = 0; i < 34; i++) si[i] = b(p + 4 + i);
            w.min_blocksize = (si[0] << 8) | si[1];
            w.max_blocksize = (si[2] << 8) | si[3];
            w.min_framesize = (si[4] << 16) | (si[5] << 8) | si[6];
            w.max_framesize = (si[7] << 16) | (si[8] << 8) | si[9];
            w.sample_rate = (si[10] << 12) | (si[11] << 4) | (si[12] >> 4);
            w.channels = ((si[12] >> 1) & 7u) + 1u;
            w.bps = (((si[12] & 1u) << 4) | (si[13] >> 4)) + 1u;
            w.total_samples = ((uint64_t)(si[13] & 15u) << 32) | (si[14] << 24) | (si[15] << 16) | (si[16] << 8) | si[17];
#pragma unroll
            for (int i = 0; i < 4; i++)
                w.md5[i] = si[18 + 4 * i] | (si[19 + 4 * i] << 8) | (si[20 + 4 * i] << 16) | (si[21 + 4 * i] << 24);
            have = true;
        } else if (type == 3) {
            w.flags |= BNF_META_SEEKTABLE;
        }
        p += 4u + (uint64_t)len; /* the bytes of a long STREAMINFO past 34 and every other block: skipped */
        if (p > n) return w.status = BNF_SCAN_TRUNCATED;
        if (h0 & 0x80u) break;
    }
    if (!have) return w.status = BNF_SCAN_NO_STREAMINFO;
    w.p = p; /* p == n: a stream of zero frames */
    return BNF_SCAN_OK;
}

/* What became of a stream: kept, emptied because the walk failed, emptied because it differs
 * from the expected parameters. */
enum { BNF_SCAN_KEPT = 0, BNF_SCAN_FAILED = 1, BNF_SCAN_DIFFERENT = 2 };

/* One stream of a scan: the walk over b = the bytes [begin, end) (not read when bad_range), then
 * the outputs: the record m, the two words of the descriptor the scan owns, and the 16 md5sum
 * bytes as little-endian words.  A stream that is not kept is emptied: first_offset = end,
 * total_samples 0, md5 zeros.  expect: nullptr, or the parameters every kept stream shares
 * (has_stream_info and total_samples are not compared). */
template <class Bytes>
__host__ __device__ inline uint32_t bnf_metadata_scan(const Bytes &b, uint64_t begin, uint64_t end, bool bad_range,
                                                      const bnf_stream_params *expect, bnf_stream_meta &m,
                                                      uint64_t &first_offset, uint64_t &total_samples,
                                                      uint32_t (&md5)[4]) {
    bnf_meta_walk w;
    if (bad_range) {
        w.status = BNF_SCAN_BAD_RANGE;
        w.flags = w.nblocks = w.id3_bytes = 0;
    } else {
        bnf_metadata_walk(b, end - begin, w);
    }
    m.status = w.status;
    m.flags = w.flags;
    m.nblocks = w.nblocks;
    m.id3_bytes = w.id3_bytes;
    m.sp.has_stream_info = 0;
    m.sp.min_blocksize = m.sp.max_blocksize = m.sp.sample_rate = m.sp.channels = m.sp.bps = 0;
    m.sp.total_samples = 0;
    m.min_framesize = m.max_framesize = 0;
    m.first_offset = first_offset = end;
    total_samples = 0;
    md5[0] = md5[1] = md5[2] = md5[3] = 0;
    if (w.status != BNF_SCAN_OK) return BNF_SCAN_FAILED;
    m.sp.has_stream_info = 1;
    m.sp.min_blocksize = w.min_blocksize;
    m.sp.max_blocksize = w.max_blocksize;
    m.sp.sample_rate = w.sample_rate;
    m.sp.channels = w.channels;
    m.sp.bps = w.bps;
    m.sp.total_samples = w.total_samples;
    m.min_framesize = w.min_framesize;
    m.max_framesize = w.max_framesize;
    m.first_offset = begin + w.p; /* the stream's own, also when it is emptied below */
    if (!(w.md5[0] | w.md5[1] | w.md5[2] | w.md5[3])) m.flags |= BNF_META_MD5_ZERO;
    if (expect && (expect->min_blocksize != w.min_blocksize || expect->max_blocksize != w.max_blocksize ||
                   expect->sample_rate != w.sample_rate || expect->channels != w.channels || expect->bps != w.bps)) {
        m.flags |= BNF_META_DIFFERS;
        return BNF_SCAN_DIFFERENT;
    }
    first_offset = begin + w.p;
    total_samples = w.total_samples;
#pragma unroll
    for (int i = 0; i < 4; i++) md5[i] = w.md5[i];
    return BNF_SCAN_KEPT;
}

#endif
