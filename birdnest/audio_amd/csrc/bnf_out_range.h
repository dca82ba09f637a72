/*
 * bnf_out_range.h -- the rule of bnflac_decode_frames' "a frame is written only when its whole
 * range lies in [0, out_bytes)".  One function, callable from host and device: decode_block
 * (k_decode<W>), k_decode_st, k_decode_sw (bnflac_kernels.hip), k_decode_sys (bnflac_sys.hip) and
 * k_fill_bad ask it, so a frame is in range for all of them or for none.  The header needs no
 * HIP: a plain C++ compiler takes it too (tools/out_range_table.cpp prints its verdicts).
 *
 * A frame of `blocksize` samples at position p (samples, 64 bits: the caller's table entry, or
 * the header's sample number minus base_sample, which wraps to a value near 2^64 when the number
 * lies below base_sample) occupies bytes [p * stride, (p + blocksize) * stride) of the output.
 * With limit = out_bytes / stride, the samples the output holds, it fits iff
 *
 *     p <= limit  &&  blocksize <= limit - p
 *
 * No product and no sum of the untrusted p is formed, so nothing wraps: limit - p is computed only
 * when p <= limit.  (The form this replaces, (p + blocksize) * stride <= out_bytes, passes for
 * p = 2^64 - d, d <= blocksize, and for p = ceil(2^64 / stride): the frame was then written before
 * d_out, or over another frame's range.)  For a position the rule accepts, p * stride and
 * (p + blocksize) * stride are at most out_bytes and the callers' address arithmetic is exact.
 */
#ifndef BNF_OUT_RANGE_H
#define BNF_OUT_RANGE_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BNF_OUT_HD __host__ __device__
#else
#define BNF_OUT_HD
#endif

/* The samples an output of out_bytes bytes holds at stride bytes per sample (every layout's stride
 * is at least 2; a stride of 0 holds nothing).  The same for every frame of a call, except that
 * BNF_OUT_FLACDECODER's stride follows the frame's channels. */
BNF_OUT_HD inline uint64_t bnf_out_limit(uint64_t out_bytes, uint64_t stride) {
    return stride ? out_bytes / stride : 0u;
}

/* The frame at position p lies inside the output. */
BNF_OUT_HD inline bool bnf_out_in_range(uint64_t p, uint32_t blocksize, uint64_t limit) {
    return p <= limit && blocksize <= limit - p;
}

#endif
