// Device side of the paged KV cache (PagedKV, mx_kernels.h), shared by kv_cache.hip, kv_prefill.hip and rope_append.hip: the page-table
// walk (seq_len, kv_row, k_row), where an appended token's row lies and what is written there (append_row, store_row: the int4 rule or
// the fp8 rule of include/micromix_hip.h, or a bf16 copy), the decoding (int4: codes_to_bf16; fp8: fp8x4_to_bf16, fp8x4_to_f32; both:
// scale_of, zero_of) and the split-KV merge (merge_chunks).
// One copy of each, so the kernels cannot drift apart.  In the append, a wave owns a (token, head) row, lane l its elements 2 l, 2 l + 1.
// The fp8 kind (KV_FP8): OCP e4m3fn codes, element j in byte j, with the int4 kind's (scale, zero) pair per row, scale = 2^e and
// zero = +0.0, so value = decode(code) * scale - zero holds for both.  e is the smallest integer in [-14, 15] with amax <= 448 * 2^e.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

#include "mx_kernels.h"

namespace mm {
namespace kv {

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef __bf16 v2bf __attribute__((ext_vector_type(2)));
typedef short v2s __attribute__((ext_vector_type(2)));
typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int HD = 128;            // head_dim
using mm::KV_INT4;
using mm::KV_BF16;
using mm::KV_FP8;

__device__ inline float bf16f(uint32_t bits16) { return __uint_as_float(bits16 << 16); }

__device__ inline uint16_t f2bf_rne(float f) {    // finite inputs
    const uint32_t u = __float_as_uint(f);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ inline uint32_t pack_bf(float lo, float hi) { return (uint32_t)f2bf_rne(lo) | ((uint32_t)f2bf_rne(hi) << 16); }

__device__ inline __half sat_half(float x) { return __float2half_rn(fminf(fmaxf(x, -65504.0f), 65504.0f)); }

// the two halves of a row's (scale, zero) fp16 pair, read as one dword
__device__ inline float scale_of(uint32_t w) { return __half2float(__ushort_as_half((unsigned short)(w & 0xffffu))); }
__device__ inline float zero_of(uint32_t w) { return __half2float(__ushort_as_half((unsigned short)(w >> 16))); }

// 8 int4 codes (one dword, element 2j in the low nibble of byte j) -> 8 bf16 values 16 + code (exact), MFMA operand order
__device__ inline v8bf codes_to_bf16(uint32_t w) {
    const uint32_t lo = w & 0x0f0f0f0fu, hi = (w >> 4) & 0x0f0f0f0fu;
    v4u r;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const uint32_t sel = 0x0c000c00u | ((4u + m) << 16) | (uint32_t)m;  // byte0 = lo.byte m, byte2 = hi.byte m, bytes 1, 3 = 0
        r[m] = (__builtin_amdgcn_perm(hi, lo, sel) << 3) | 0x41804180u;    // bf16 0x4180 | c << 3 = 16 + c
    }
    return __builtin_bit_cast(v8bf, r);
}

// 4 e4m3 codes (one dword, element j in byte j) -> 4 bf16 values (exact: e4m3 has 3 mantissa bits), element j in half j.  The scale
// operand is 1.0, so nothing depends on which way the converter applies it
__device__ inline v2u fp8x4_to_bf16(uint32_t w) {
    v2u r;
    r.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
    r.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true));
    return r;
}

// 4 e4m3 codes -> 4 fp32 values
__device__ inline void fp8x4_to_f32(uint32_t w, float *f) {
    const v2f lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    f[0] = lo.x; f[1] = lo.y; f[2] = hi.x; f[3] = hi.y;
}

// the sequence a flat index belongs to: the largest b with indptr[b] <= i (empty sequences are skipped over)
__device__ inline int find_seq(const int *indptr, int B, int i) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (indptr[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ inline int seq_len(const PagedKV &kv, int b) {
    const int np = kv.indptr[b + 1] - kv.indptr[b];
    return np > 0 ? (np - 1) * kv.P + min(max(kv.last_page_len[b], 0), kv.P) : 0;    // clamped: a bad entry never reads past the page list
}

// row index (in rows of one token-head) of K (which = 0) or V (which = 1) of `page`, `slot`; a V row lies v_offset behind its K row
__device__ inline int64_t kv_row(const PagedKV &kv, int page, int which, int h, int slot) {
    return ((((int64_t)page * kv.L + kv.layer) * 2 + which) * kv.Hkv + h) * kv.P + slot;
}
__device__ inline int64_t v_offset(const PagedKV &kv) { return (int64_t)kv.Hkv * kv.P; }

// the K row of token t, head h of the sequence whose page list is `pages`; false (and row 0, which is safe to address) for a token
// at or past `end` or on a page outside the cache
__device__ inline bool k_row(const PagedKV &kv, const int *pages, int t, int end, int h, int64_t &row) {
    const int page = t < end ? pages[t / kv.P] : -1;
    const bool ok = page >= 0 && page < kv.max_pages;
    row = ok ? kv_row(kv, page, 0, h, t % kv.P) : 0;
    return ok;
}

// the first position of a window of W >= 1 tokens that ends at position p (HF's sliding_window: max(0, p - W + 1)); p >= -1
__device__ inline int window_begin(int p, int W) { return p >= W ? p - W + 1 : 0; }

// the K (which = 0) or V (which = 1) row of appended token i, head h; -1: nothing is written for this token
__device__ inline int64_t append_row(const PagedKV &kv, const int *append_indptr, int i, int which, int h) {
    const int b = find_seq(append_indptr, kv.B, i);
    const int len = seq_len(kv, b);
    const int pos = len - (append_indptr[b + 1] - append_indptr[b]) + (i - append_indptr[b]);
    if (pos < 0 || pos >= len) return -1;                     // a table that does not count the appended tokens: nothing written
    const int page = kv.indices[kv.indptr[b] + pos / kv.P];
    if (page < 0 || page >= kv.max_pages) return -1;
    return kv_row(kv, page, which, h, pos % kv.P);
}

// the whole wave stores one row: `two` = this lane's elements 2 lane, 2 lane + 1 (bf16 bits)
template <int KIND>
__device__ inline void store_row(const PagedKV &kv, int64_t row, int lane, uint32_t two) {
    if (KIND == KV_BF16) {
        ((uint32_t *)kv.data)[row * (HD / 2) + lane] = two;
        return;
    }
    if (KIND == KV_FP8) {
        // bf16 magnitudes order as their bit patterns do, so amax, the exponent and the clamp are integer work: no divide, no log
        uint32_t m0 = two & 0x7fffu, m1 = (two >> 16) & 0x7fffu;
        uint32_t amax = max(m0, m1);
#pragma unroll
        for (int o = 32; o; o >>= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, o));
        // amax = 1.M * 2^(E - 127) <= 448 * 2^e = 1.75 * 2^(e + 8): e = E - 135, one more when M > 0.75 * 128
        const int e = min(max((int)(amax >> 7) - 135 + ((amax & 127u) > 96u ? 1 : 0), -14), 15);
        const uint32_t top = ((uint32_t)(135 + e) << 7) | 96u;               // 448 * 2^e as bf16 bits; only e = 15 (clamped) can exceed it
        m0 = min(m0, top);
        m1 = min(m1, top);
        const uint32_t cl = (two & 0x80008000u) | m0 | (m1 << 16);           // the signs stay, -0.0 too
        const v2s r = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(v2s{0, 0}, __builtin_bit_cast(v2bf, cl), __uint_as_float((uint32_t)(127 + e) << 23), false);
        ((uint16_t *)kv.data)[row * (HD / 2) + lane] = (uint16_t)r.x;
        if (lane == 0) ((uint32_t *)kv.param)[row] = (uint32_t)(15 + e) << 10;   // fp16 (2^e, +0.0)
        return;
    }
    const float x0 = bf16f(two & 0xffffu), x1 = bf16f(two >> 16);
    float mn = fminf(x0, x1), mx = fmaxf(x0, x1);
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    const float s = __half2float(sat_half(__fdiv_rn(fmaxf(mx - mn, 1e-5f), 15.0f)));
    const float base = fminf(fmaxf(rintf(__fdiv_rn(-mn, s)), 0.0f), 15.0f);
    const float c0 = fminf(fmaxf(rintf(__fdiv_rn(x0, s)) + base, 0.0f), 15.0f);
    const float c1 = fminf(fmaxf(rintf(__fdiv_rn(x1, s)) + base, 0.0f), 15.0f);
    kv.data[row * (HD / 2) + lane] = (uint8_t)((unsigned)c0 | ((unsigned)c1 << 4));
    if (lane == 0) {
        kv.param[row * 2] = __half_as_ushort(__float2half_rn(s));
        kv.param[row * 2 + 1] = __half_as_ushort(sat_half(fabsf(base * s)));   // base = clamp(-0.0) has no defined sign: a zero `zero` is stored as +0.0
    }
}

// Split-KV merge of N adjacent output values: chunk c left (m, l) at ml[2 (first + c stride)] and its partial sums at
// part[(first + c stride) HD]; a chunk without attended tokens has m = -inf and l = 0.  Leaves the normalised values in out[].
template <int N>
__device__ inline void merge_chunks(const float *ml, const float *part, int64_t first, int64_t stride, int nc, float (&out)[N]) {
    typedef float vf __attribute__((ext_vector_type(N)));
    float M = -INFINITY;
    for (int c = 0; c < nc; ++c) M = fmaxf(M, ml[(first + c * stride) * 2]);
    float ls = 0.0f;
    vf acc = 0.0f;
    if (M != -INFINITY) {
        for (int c = 0; c < nc; ++c) {
            const int64_t p = first + c * stride;
            const float f = exp2f(ml[p * 2] - M);
            ls += f * ml[p * 2 + 1];
            acc += f * *(const vf *)(part + p * HD);
        }
    }
    const float inv = ls > 0.0f ? 1.0f / ls : 0.0f;
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = acc[k] * inv;
}

}  // namespace kv
}  // namespace mm
