/* bnf_common.h -- what every kernel TU of libbnflac.so holds: the CRC tables, g_stats, the LDS and
 * global access helpers (bnflac_kernels.hip's head comment describes the kernels) */
#ifndef BNF_COMMON_H
#define BNF_COMMON_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bnflac_device.h"
#include "bnflac_launch.h" /* the `ablate` word (BNF_ABLATE_*, BNF_MODE_*) and every cross-TU declaration */

#define DEV __device__ __forceinline__

/* ------------------------------------------- CRC tables (CRC-8; slice-by-8 CRC-16 for k_decode<W>, k_decode_sys) */
/* Tables are filled by the host at module load (bnflac_runtime.cpp) into these: */
__constant__ uint8_t g_crc8_tab[256];
__constant__ uint16_t g_crc16_tab[8][256]; /* slice-by-8 */
__constant__ uint16_t g_crc16_xpow[40];    /* x^(8*2^j) mod P for j < 40 */
/* Debug event counters (wave-level events, enabled by ablate bit 0x100; timing runs
 * leave them off).  0 fused chunks, 1 generic chunks, 2 DMA landing waits, 3 slow Rice
 * codewords, 4 refills, 5 waves, 6 k_decode_st tails that continued the running CRC-16 (lanes),
 * 7 of those, the ones whose remainder differs from the re-read's (-DBNFLAC_CRC_FOLD_CHECK
 * builds only, with or without 0x100). */
__device__ unsigned long long g_stats[16]; /* 8.. : s_memtime cycles per phase, summed over waves */
/* Phase timers (s_memtime) for the debug counters; compiled in only with
 * -DBNFLAC_PHASE_TIMERS, because a scalar-memory op anywhere in the loop makes hipcc's
 * LDS waits conservative (lgkmcnt(0)). */
DEV uint64_t tnow(bool on) { /* call at wave-uniform points only */
#ifndef BNFLAC_PHASE_TIMERS
    (void)on;
    return 0ull;
#endif
    if (!on) return 0ull;
    const uint64_t t = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    return t;
}
#define STAT(on, i) do { if (on) { if (__builtin_amdgcn_read_exec() && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec())) atomicAdd(&g_stats[i], 1ull); } } while (0)

typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) uint16_t lds_u16;
typedef __attribute__((address_space(3))) void lds_void;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
/* LDS accesses to buffers that are never LDS-DMA targets, as inline asm: hipcc cannot tell
 * them from the DMA'd ring and would drain every vector-memory op (vmcnt(0)) first.
 * Completion is waited for explicitly (lds_sync / lgkmcnt). */
DEV void lds_st128(const void *a, u32x4 v) {
    asm volatile("ds_write_b128 %0, %1" ::"v"((uint32_t)(uintptr_t)a), "v"(v) : "memory");
}
DEV u32x4 lds_ld128(const void *a) { /* result valid after s_waitcnt lgkmcnt(0) */
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"((uint32_t)(uintptr_t)a) : "memory");
    return v;
}
DEV void lds_st128(const lds_u32x4 *a, u32x4 v) {
    asm volatile("ds_write_b128 %0, %1" ::"v"((uint32_t)(uintptr_t)a), "v"(v) : "memory");
}
DEV u32x4 lds_ld128(const lds_u32x4 *a) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"((uint32_t)(uintptr_t)a) : "memory");
    return v;
}
DEV void lds_st64(const void *a, uint64_t v) {
    asm volatile("ds_write_b64 %0, %1" ::"v"((uint32_t)(uintptr_t)a), "v"(v) : "memory");
}
DEV uint64_t lds_ld64(const void *a) {
    uint64_t v;
    asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"((uint32_t)(uintptr_t)a) : "memory");
    return v;
}
typedef __attribute__((address_space(1))) const void gvoid;
/* 16-byte global store through an integer address: the address-space cast keeps it a
 * global_store (a generic pointer would make it a flat store, which also counts in
 * lgkmcnt -- every later LDS wait would then wait for the HBM write) */
DEV void gst128(uint64_t addr, u32x4 v) { *(__attribute__((address_space(1))) u32x4 *)addr = v; }

/* ------------------------------------------------------------- per-TU tables and counters */
/* Each kernel TU (build.py HIP_TUS) is its own code object with its own __constant__ tables and
 * g_stats: the two functions below act on the including TU's copy, and each TU publishes them as
 * its bnf_tu_ops entry (bnflac_launch.h), which the parse TU loops over. */
static hipError_t tu_upload_tables(const uint8_t *crc8, const uint16_t *crc16x8, const uint16_t *xpow) {
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_crc8_tab), crc8, 256);
    if (e != hipSuccess) return e;
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_crc16_tab), crc16x8, 8 * 256 * sizeof(uint16_t));
    if (e != hipSuccess) return e;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_crc16_xpow), xpow, 40 * sizeof(uint16_t));
}
static hipError_t tu_stats(uint64_t *out16, int reset) { /* adds this TU's g_stats to out16 */
    uint64_t v[16];
    hipError_t e = hipMemcpyFromSymbol(v, HIP_SYMBOL(g_stats), sizeof v);
    if (e != hipSuccess) return e;
    for (int i = 0; i < 16; i++) out16[i] += v[i];
    if (reset) {
        static const uint64_t z[16] = {0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_stats), z, sizeof z);
    }
    return e;
}
#endif /* BNF_COMMON_H */
