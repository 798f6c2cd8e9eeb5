// Low-level device primitives shared by the GEMM, decode and norm kernels (mx_gemm_tile.inc, mx_gemm_stream.hip, mx_gemm_skinny.hip,
// qlinear_decode.hip, rmsnorm_quantize.hip and the quantizer headers): buffer descriptors, the LDS-DMA, counted waits and the loads
// of MFMA fragments from global memory.  Each of them encodes a hardware rule (the descriptor's flags word, the wait states between a
// scalar write and a vector-memory read, who owns M0, the MFMA register layouts).  One copy of each, so the kernels cannot drift apart.
#pragma once
#include "mx_common.h"

namespace mm {

// hipcc parses __device__ bodies in its host pass as well; gfx950 inline asm and target builtins only exist in
// the device pass, so those few bodies are compiled for the device only.
#if defined(__HIP_DEVICE_COMPILE__)
#define MM_DEVICE_ONLY(...) __VA_ARGS__
#else
#define MM_DEVICE_ONLY(...)
#endif

typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v6i __attribute__((ext_vector_type(6)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------
// Buffer descriptors
// ---------------------------------------------------------------------------------------------------------
// 128-bit raw buffer descriptor {base_lo, base_hi(16 bits) | stride 0, num_records (bytes), flags}, every word made
// provably wave-uniform so that it can be bound to an "s" operand of an inline-asm buffer instruction.
typedef int rsrc_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ rsrc_t make_rsrc(const void *base, unsigned bytes) {
    const unsigned long long v = (unsigned long long)base;
    rsrc_t r;
    r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)v);
    r[1] = __builtin_amdgcn_readfirstlane((int)((unsigned)(v >> 32) & 0xFFFFu));
    r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    r[3] = 0x00020000;
    return r;
}

// The same descriptor as a compiler-visible buffer resource, for loads into registers through the raw_buffer_load builtins
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_brsrc(const uint8_t *base, unsigned bytes) {
    const unsigned long long v = (unsigned long long)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)hi << 32) | lo), 0,
                                             (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

// ---------------------------------------------------------------------------------------------------------
// LDS-DMA and counted waits
// ---------------------------------------------------------------------------------------------------------
// LDS byte address of a generic pointer into the workgroup's LDS: the low half of the flat address (the aperture base sits in
// the high half).  Written as a truncation, not as an address-space cast: the cast carries a null test that hipcc (ROCm 7.2)
// lowers to an illegal V_CMP against src_shared_base when it cannot prove the pointer wave-uniform.
__device__ __forceinline__ unsigned lds_address(const uint8_t *p) {
    return (unsigned)(unsigned long long)p;
}

// one buffer_load_dwordx4 ... lds: 64 lanes x 16 B -> LDS bytes [lds_addr, lds_addr + 1024) in lane order (M0 = wave-uniform base,
// the hardware adds lane * 16); per-lane source = descriptor base + voff + soff.
//   s_nop 4 : SALU/readfirstlane results (descriptor, soffset) may not be read by a VMEM instruction for 5 states
//   s_nop 0 : one state between the M0 write and the LDS-DMA that reads it
// M0 belongs to the compiler, so it is saved and restored inside the statement.
// The compiler does not see the LDS writes; ordering is the caller's: a counted wait_vmcnt<N>() (LDS-DMA completion is what vmcnt
// counts), then a barrier where other waves read the bytes.
__device__ __forceinline__ void dma16(const rsrc_t &rsrc, int voff, int soff, unsigned lds_addr) {
    MM_DEVICE_ONLY(unsigned keep;
                   asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                                "buffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
                                : "=&s"(keep)
                                : "v"(voff), "s"(rsrc), "s"(lds_addr), "s"(soff)
                                : "memory");)
}

// at most N vector-memory instructions (loads, stores and LDS-DMA together, in issue order) of this wave still outstanding
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    MM_DEVICE_ONLY(asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");)
}

// ---------------------------------------------------------------------------------------------------------
// MFMA fragments of a packed operand row from global memory
// ---------------------------------------------------------------------------------------------------------
// bytes of one row's 128-deep slab
template <int EL> constexpr int slab_bytes = EL == EL_FP8 ? 128 : (EL == EL_FP6 ? 96 : 64);

// v_mfma_scale_f32_32x32x64_f8f6f4: one lane's fragment for MFMA step h (64 deep) of slab `slab`; row byte offset `rowoff` inside the
// descriptor, lane l = (row/col l & 31, kb = l >> 5).
// Register layouts (measured, tests/test_hw_gpu.py): fp4/fp6 lanes hold the 32 consecutive elements of K block 2h + kb;
// fp8 lanes hold K = 64h + 16kb + [0,16) in registers 0-3 and K = 64h + 32 + 16kb + [0,16) in registers 4-7.
template <int EL>
__device__ __forceinline__ v8i load_frag(__amdgpu_buffer_rsrc_t rsrc, int rowoff, int slab, int h, int kb) {
    const int so = slab * slab_bytes<EL>;
    v8i r = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (EL == EL_FP8) {
        const v4i lo = __builtin_amdgcn_raw_buffer_load_b128(rsrc, rowoff + (4 * h + kb) * 16, so, 0);
        const v4i hi = __builtin_amdgcn_raw_buffer_load_b128(rsrc, rowoff + (4 * h + 2 + kb) * 16, so, 0);
        r = v8i{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    } else if constexpr (EL == EL_FP4) {
        const v4i v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, rowoff + (2 * h + kb) * 16, so, 0);
        r = v8i{v[0], v[1], v[2], v[3], 0, 0, 0, 0};
    } else {
        const int o = rowoff + (2 * h + kb) * 24;
        const v2i a = __builtin_amdgcn_raw_buffer_load_b64(rsrc, o, so, 0);
        const v2i b = __builtin_amdgcn_raw_buffer_load_b64(rsrc, o + 8, so, 0);
        const v2i c = __builtin_amdgcn_raw_buffer_load_b64(rsrc, o + 16, so, 0);
        r = v8i{a[0], a[1], b[0], b[1], c[0], c[1], 0, 0};
    }
    return r;
}

// v_mfma_scale_f32_16x16x128_f8f6f4: the fragment of a whole 128-deep slab.
// Register layouts (tests/test_hw_gpu.py): lane l = (row/col l & 15, K block h = l >> 4); fp4/fp6 lanes hold the 32 elements of
// block h, fp8 lanes hold K = 16h + [0,16) and 64 + 16h + [0,16); the scale byte of a lane belongs to block h.
template <int EL>
__device__ __forceinline__ v8i load_frag16(__amdgpu_buffer_rsrc_t rsrc, int rowoff, int slab, int h) {
    const int so = slab * slab_bytes<EL>;
    v8i r = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (EL == EL_FP8) {
        const v4i lo = __builtin_amdgcn_raw_buffer_load_b128(rsrc, rowoff + h * 16, so, 0);
        const v4i hi = __builtin_amdgcn_raw_buffer_load_b128(rsrc, rowoff + 64 + h * 16, so, 0);
        r = v8i{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    } else if constexpr (EL == EL_FP4) {
        const v4i v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, rowoff + h * 16, so, 0);
        r = v8i{v[0], v[1], v[2], v[3], 0, 0, 0, 0};
    } else {
        const int o = rowoff + h * 24;
        const v2i a = __builtin_amdgcn_raw_buffer_load_b64(rsrc, o, so, 0);
        const v2i b = __builtin_amdgcn_raw_buffer_load_b64(rsrc, o + 8, so, 0);
        const v2i c = __builtin_amdgcn_raw_buffer_load_b64(rsrc, o + 16, so, 0);
        r = v8i{a[0], a[1], b[0], b[1], c[0], c[1], 0, 0};
    }
    return r;
}

}  // namespace mm
