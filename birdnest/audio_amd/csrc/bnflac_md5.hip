/*
 * bnflac_md5.hip -- k_md5_streams: the STREAMINFO md5sum of every stream of a decoded batch,
 * computed where the PCM lies.
 *
 * libFLAC 1.2.1 hashes a stream's sample frames interleaved by channel, each sample as
 * B = (bps + 7) / 8 little-endian bytes (FLAC__MD5Accumulate, LibFlac.dll@0x10007920;
 * bnflac_md5.h is the host version).  MD5 (RFC 1321) is one serial chain per message, so the
 * only parallelism is across streams: one lane owns one stream, 64-thread workgroups, a grid of
 * ceil(nstreams / 64).
 *
 * A lane reads its message straight from the decode output through one of two sources:
 *   packed (SRC 0)  the layout's bytes are the message (FLACDecoder 16-bit with 1-2 channels,
 *                   FLACFileReader 16- or 24-bit): the byte range [bounds[s], bounds[s + 1]) * stride.
 *                   The start has any byte alignment: dwords are loaded from start & ~3 and
 *                   realigned with the lane's own byte funnel (v_alignbyte_b32); the 17th dword
 *                   of a block is carried into the next one.
 *   int32 (SRC = B) INTERLEAVED32: the low B bytes of every int32 of the range.  64 / 32 / 16
 *                   samples make one block for B = 1 / 2 / 4; for B = 3, 64 samples make a group
 *                   of three blocks, and the fast loop advances in whole groups.
 *
 * Fast loop (both sources): a lane runs it while it has a whole block (group) left; the wave
 * stays in it while any lane does, the others masked off.  The loads of the next block are
 * issued before the 64 steps of the current one and turned into its 16 message words after
 * them, so only those 16 words cross into the next iteration.  The 64 steps are fully unrolled:
 * message-word index, rotate count and round constant are compile-time constants and the 16
 * words are plain VGPRs.  No LDS, no tables in memory, no atomics in the loop.
 *
 * Tail (one byte feeder for every source): the bytes left of the last partial block or group,
 * then 0x80, the zeros and the 64-bit bit length, in as many blocks as that takes.  It reads
 * single bytes at their own addresses, so it reads nothing outside the range.
 *
 * Read bounds: no lane reads outside [pcm, pcm + round_up(pcm_bytes, 4)).  Every dword of a whole
 * block starts below the range's end; the 17th dword of the packed source is the only one that
 * can start at it (when the start is dword aligned, where its value is not used), and its
 * address is clamped to the buffer's last dword.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bnflac_launch.h"

#define MD5_LANES 64

/* The 64 steps of one block.  w: the block's 16 little-endian message words. */
__device__ __forceinline__ void md5_steps(uint32_t (&h)[4], const uint32_t (&w)[16]) {
    constexpr uint32_t K[64] = {
        0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501,
        0x698098d8, 0x8b44f7af, 0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821,
        0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453, 0xd8a1e681, 0xe7d3fbc8,
        0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a,
        0xfffa3942, 0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70,
        0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665,
        0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1,
        0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};
    constexpr int S[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        uint32_t f;
        int g;
        if (i < 16) {
            f = d ^ (b & (c ^ d)); /* v_bfi_b32 */
            g = i;
        } else if (i < 32) {
            f = c ^ (d & (b ^ c));
            g = (5 * i + 1) & 15;
        } else if (i < 48) {
            f = b ^ c ^ d;
            g = (3 * i + 5) & 15;
        } else {
            f = c ^ (b | ~d);
            g = (7 * i) & 15;
        }
        const uint32_t t = a + f + K[i] + w[g];
        a = d;
        d = c;
        c = b;
        b += __builtin_rotateleft32(t, S[(i >> 4) * 4 + (i & 3)]);
    }
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
}

/* A source's view of one lane's message.  SRC 0: packed bytes; SRC 1..4: int32 samples, B = SRC.
 *   GROUP_BLOCKS  blocks the fast loop advances by;  RAW  dwords one block's loads fill;
 *   STEP          source bytes of a group: one block, or 64 / 32 / 64 / 16 int32 samples. */
template <int SRC>
struct Md5Src {
    static constexpr int B = SRC;
    static constexpr int GROUP_BLOCKS = SRC == 3 ? 3 : 1;
    static constexpr int RAW = SRC == 0 ? 16 : SRC == 3 ? 22 : 64 / SRC;
    static constexpr int STEP = SRC == 0 ? 64 : SRC == 3 ? 256 : 256 / (SRC ? SRC : 1);
    static constexpr int first_sample(int j) { return 64 * j / B; } /* of block j of a group */

    const uint8_t *p;    /* SRC 0: the next block's first byte, rounded down to a dword; else its group's first sample */
    const uint8_t *last; /* SRC 0: the buffer's last dword */
    uint32_t sh;         /* SRC 0: start & 3 */
    uint32_t carry;      /* SRC 0: the dword the next block's first word starts in */

    /* issue the loads of block J of the group at g (SRC 0: the 16 dwords after the carried one) */
    template <int J>
    __device__ __forceinline__ void issue(uint32_t (&raw)[RAW], const uint8_t *g) const {
        if constexpr (SRC == 0) {
            const uint32_t *q = (const uint32_t *)g;
#pragma unroll
            for (int i = 0; i < 15; i++) raw[i] = q[i + 1];
            const uint8_t *e = g + 64;
            raw[15] = *(const uint32_t *)(e < last ? e : last);
        } else {
            const uint32_t *q = (const uint32_t *)g + first_sample(J);
#pragma unroll
            for (int i = 0; i < RAW; i++) raw[i] = q[i];
        }
    }
    /* ... and turn them into the block's 16 message words */
    template <int J>
    __device__ __forceinline__ void words(const uint32_t (&raw)[RAW], uint32_t (&w)[16]) {
        if constexpr (SRC == 0) {
            w[0] = __builtin_amdgcn_alignbyte(raw[0], carry, sh);
#pragma unroll
            for (int i = 1; i < 16; i++) w[i] = __builtin_amdgcn_alignbyte(raw[i], raw[i - 1], sh);
            carry = raw[15];
        } else if constexpr (SRC == 1) { /* byte 0 of four samples: three v_perm_b32 */
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t lo = __builtin_amdgcn_perm(raw[4 * i + 1], raw[4 * i], 0x0c0c0400u);
                const uint32_t hi = __builtin_amdgcn_perm(raw[4 * i + 3], raw[4 * i + 2], 0x0c0c0400u);
                w[i] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int m = 64 * J + 4 * i + k; /* message byte of the group */
                    v |= ((raw[m / B - first_sample(J)] >> (8 * (m % B))) & 0xffu) << (8 * k);
                }
                w[i] = v;
            }
        }
    }
};

/* Blocks J .. GROUP_BLOCKS - 1 of the group at src.p, block J's words in nx: hash a block while
 * the next one's loads fly.  After the group's last block that is the next group's block 0; a
 * lane with no next group (`more` false) loads this group's block 0 again instead, so the body
 * has no branch and reads nothing new, and leaves with nx unspecified.  The loads stay in
 * front of the steps (sched_barrier), and their registers pass through an empty asm that
 * also takes the steps' result, so the conversion cannot move in front of the steps. */
template <int SRC, int J>
__device__ __forceinline__ void md5_group(Md5Src<SRC> &src, uint32_t (&h)[4], uint32_t (&nx)[16], bool more) {
    constexpr int G = Md5Src<SRC>::GROUP_BLOCKS, NJ = J + 1 < G ? J + 1 : 0;
    uint32_t w[16], raw[Md5Src<SRC>::RAW];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = nx[i];
    const uint8_t *const next = src.p + Md5Src<SRC>::STEP;
    src.template issue<NJ>(raw, NJ ? src.p : more ? next : src.p);
    __builtin_amdgcn_sched_barrier(0);
    md5_steps(h, w);
#pragma unroll
    for (int i = 0; i < Md5Src<SRC>::RAW; i++) asm volatile("" : "+v"(raw[i]) : "v"(h[1]));
    src.template words<NJ>(raw, nx);
    if constexpr (NJ)
        md5_group<SRC, NJ>(src, h, nx, more);
    else
        src.p = next;
}

template <int SRC>
__global__ __launch_bounds__(MD5_LANES) void k_md5_streams(const uint8_t *__restrict__ pcm, uint64_t pcm_bytes, uint32_t unit,
                                                           const uint64_t *__restrict__ bounds, uint32_t nstreams,
                                                           const uint8_t *__restrict__ expected, uint8_t *__restrict__ md5,
                                                           uint32_t *__restrict__ verdict, uint32_t *__restrict__ status) {
    using Src = Md5Src<SRC>;
    constexpr uint32_t GROUP_BYTES = 64u * Src::GROUP_BLOCKS; /* message bytes of a group */
    const uint32_t s = blockIdx.x * MD5_LANES + threadIdx.x;
    if (s >= nstreams) return;
    const uint64_t b0 = bounds[s], b1 = bounds[s + 1];
    uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    uint32_t v; /* the verdict */
    if (b0 > b1 || b1 > pcm_bytes / unit) {
        h[0] = h[1] = h[2] = h[3] = 0;
        v = 3;
    } else {
        const uint8_t *const base = pcm + b0 * unit; /* the range's first byte */
        /* message length: the range's bytes, or B of every 4 of them */
        const uint64_t len = SRC == 0 ? (b1 - b0) * unit : (b1 - b0) * unit / 4 * (uint32_t)SRC;
        uint64_t groups = len / GROUP_BYTES;
        const uint32_t rem = (uint32_t)(len - groups * GROUP_BYTES);
        Src src;
        src.sh = (uint32_t)(uintptr_t)base & 3u;
        src.p = SRC == 0 ? base - src.sh : base;
        src.last = pcm + ((pcm_bytes + 3) & ~(uint64_t)3) - 4;
        src.carry = 0;
        if (groups) {
            uint32_t nx[16], raw[Src::RAW];
            if constexpr (SRC == 0) src.carry = *(const uint32_t *)src.p;
            src.template issue<0>(raw, src.p);
            src.template words<0>(raw, nx);
            do {
                md5_group<SRC, 0>(src, h, nx, groups > 1);
            } while (--groups);
        }
        /* the tail: rem bytes from here on, 0x80, zeros, the bit length */
        const uint8_t *const t = SRC == 0 ? src.p + src.sh : src.p;
        const uint32_t nblk = (rem + 9 + 63) / 64;
        for (uint32_t k = 0; k < nblk; k++) {
            uint32_t w[16];
#pragma unroll
            for (int i = 0; i < 16; i++) {
                uint32_t x = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t m = 64 * k + 4 * i + j;
                    uint32_t byte = m == rem ? 0x80u : 0u;
                    if (m < rem) byte = SRC == 0 ? t[m] : t[m / (SRC ? SRC : 1) * 4 + m % (SRC ? SRC : 1)];
                    x |= byte << (8 * j);
                }
                w[i] = x;
            }
            if (k + 1 == nblk) {
                w[14] = (uint32_t)(len << 3);
                w[15] = (uint32_t)(len >> 29);
            }
            md5_steps(h, w);
        }
        v = 2;
        if (expected) {
            uint32_t diff = 0, any = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t e = expected[16ull * s + i];
                any |= e;
                diff |= e ^ ((h[i >> 2] >> (8 * (i & 3))) & 0xffu);
            }
            if (any) v = diff ? 1 : 0;
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) md5[16ull * s + i] = (uint8_t)(h[i >> 2] >> (8 * (i & 3)));
    if (verdict) verdict[s] = v;
    /* one atomic per stream: [0] bit 0 a bad range, [1] equal, [2] differing, [3] not checked */
    if (v == 3)
        atomicOr(&status[0], 1u);
    else
        atomicAdd(&status[1 + v], 1u);
}

extern "C" hipError_t bnf_launch_md5_streams(const uint8_t *pcm, uint64_t pcm_bytes, uint32_t unit, uint32_t src,
                                             const uint64_t *bounds, uint32_t nstreams, const uint8_t *expected,
                                             uint8_t *md5, uint32_t *verdict, uint32_t *status, hipStream_t s) {
    hipError_t e = hipMemsetAsync(status, 0, 4 * sizeof(uint32_t), s);
    if (e != hipSuccess || !nstreams) return e;
    if (src > 4 || !unit) return hipErrorInvalidValue;
    const dim3 grid((nstreams + MD5_LANES - 1) / MD5_LANES), block(MD5_LANES);
#define MD5_LAUNCH(SRC)                                                                                                \
    hipLaunchKernelGGL(k_md5_streams<SRC>, grid, block, 0, s, pcm, pcm_bytes, unit, bounds, nstreams, expected, md5, \
                       verdict, status)
    switch (src) {
    case 0: MD5_LAUNCH(0); break;
    case 1: MD5_LAUNCH(1); break;
    case 2: MD5_LAUNCH(2); break;
    case 3: MD5_LAUNCH(3); break;
    default: MD5_LAUNCH(4); break;
    }
#undef MD5_LAUNCH
    return hipGetLastError();
}
