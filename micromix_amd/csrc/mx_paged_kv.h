// Device side of the paged KV cache (PagedKV, mx_kernels.h), shared by kv_cache.hip, kv_prefill.hip, rope_append.hip, rope_prefill.hip and kv_gather.hip: the page-table
// walk (seq_len, kv_row, k_row), where an appended token's row lies and what is written there (append_row, store_row: the int4 rule or
// the fp8 rule of include/micromix_hip.h, or a bf16 copy), the decoding (int4: codes_to_bf16; fp8: fp8x4_to_bf16, fp8x4_to_f32; both:
// scale_of, zero_of) and the split-KV merge (merge_chunks).
// One copy of each, so the kernels cannot drift apart.  In the append, a wave owns a (token, head) row, lane l its elements 2 l, 2 l + 1
// (store_row), or eight lanes own it, 16 elements each (store_row8, the prefill shape); both are made of the same element rules.
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

// the K or V row of head h that a token appended at position pos of sequence b (length len) is written to; -1: nothing is written
__device__ inline int64_t append_row_at(const PagedKV &kv, int b, int pos, int len, int which, int h) {
    if (pos < 0 || pos >= len) return -1;                     // a table that does not count the appended tokens: nothing written
    const int page = kv.indices[kv.indptr[b] + pos / kv.P];
    if (page < 0 || page >= kv.max_pages) return -1;
    return kv_row(kv, page, which, h, pos % kv.P);
}

// the K (which = 0) or V (which = 1) row of appended token i, head h; -1: nothing is written for this token
__device__ inline int64_t append_row(const PagedKV &kv, const int *append_indptr, int i, int which, int h) {
    const int b = find_seq(append_indptr, kv.B, i);
    const int len = seq_len(kv, b);
    const int pos = len - (append_indptr[b + 1] - append_indptr[b]) + (i - append_indptr[b]);
    return append_row_at(kv, b, pos, len, which, h);
}

// ---- the two quantizing rules, element by element: what store_row (a wave per row) and store_row8 (eight lanes per row) are made of
// fp8: bf16 magnitudes order as their bit patterns do, so amax, the exponent and the clamp are integer work: no divide, no log.
// amax = 1.M * 2^(E - 127) <= 448 * 2^e = 1.75 * 2^(e + 8): e = E - 135, one more when M > 0.75 * 128
__device__ inline int fp8_exponent(uint32_t amax) { return min(max((int)(amax >> 7) - 135 + ((amax & 127u) > 96u ? 1 : 0), -14), 15); }
__device__ inline uint32_t fp8_top(int e) { return ((uint32_t)(135 + e) << 7) | 96u; }   // 448 * 2^e as bf16 bits; only e = 15 (clamped) can exceed it
// two bf16 elements clamped to +-top; the signs stay, -0.0 too
__device__ inline uint32_t fp8_clamp(uint32_t two, uint32_t top) {
    uint32_t m0 = two & 0x7fffu, m1 = (two >> 16) & 0x7fffu;
    m0 = min(m0, top);
    m1 = min(m1, top);
    return (two & 0x80008000u) | m0 | (m1 << 16);
}
// the e4m3 codes of two clamped elements, into the low (HI = false) or high half of `into`
template <bool HI>
__device__ inline v2s fp8_codes(v2s into, uint32_t clamped, int e) {
    return __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(into, __builtin_bit_cast(v2bf, clamped), __uint_as_float((uint32_t)(127 + e) << 23), HI);
}
__device__ inline uint32_t fp8_param(int e) { return (uint32_t)(15 + e) << 10; }          // fp16 (2^e, +0.0)
// int4: quantize_int_group(x, 4, 128) in fp32 with correctly rounded divides; the codes as floats 0 .. 15
__device__ inline float int4_scale(float mn, float mx) { return __half2float(sat_half(__fdiv_rn(fmaxf(mx - mn, 1e-5f), 15.0f))); }
__device__ inline float int4_base(float mn, float s) { return fminf(fmaxf(rintf(__fdiv_rn(-mn, s)), 0.0f), 15.0f); }
__device__ inline float int4_code(float x, float s, float base) { return fminf(fmaxf(rintf(__fdiv_rn(x, s)) + base, 0.0f), 15.0f); }
__device__ inline unsigned short int4_scale_bits(float s) { return __half_as_ushort(__float2half_rn(s)); }
// base = clamp(-0.0) has no defined sign: a zero `zero` is stored as +0.0
__device__ inline unsigned short int4_zero_bits(float base, float s) { return __half_as_ushort(sat_half(fabsf(base * s))); }

// the whole wave stores one row: `two` = this lane's elements 2 lane, 2 lane + 1 (bf16 bits)
template <int KIND>
__device__ inline void store_row(const PagedKV &kv, int64_t row, int lane, uint32_t two) {
    if (KIND == KV_BF16) {
        ((uint32_t *)kv.data)[row * (HD / 2) + lane] = two;
        return;
    }
    if (KIND == KV_FP8) {
        uint32_t m0 = two & 0x7fffu, m1 = (two >> 16) & 0x7fffu;
        uint32_t amax = max(m0, m1);
#pragma unroll
        for (int o = 32; o; o >>= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, o));
        const int e = fp8_exponent(amax);
        const uint32_t top = fp8_top(e);
        m0 = min(m0, top);                                                   // fp8_clamp, on the magnitudes taken above
        m1 = min(m1, top);
        const uint32_t cl = (two & 0x80008000u) | m0 | (m1 << 16);
        const v2s r = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(v2s{0, 0}, __builtin_bit_cast(v2bf, cl), __uint_as_float((uint32_t)(127 + e) << 23), false);
        ((uint16_t *)kv.data)[row * (HD / 2) + lane] = (uint16_t)r.x;
        if (lane == 0) ((uint32_t *)kv.param)[row] = fp8_param(e);
        return;
    }
    const float x0 = bf16f(two & 0xffffu), x1 = bf16f(two >> 16);
    float mn = fminf(x0, x1), mx = fmaxf(x0, x1);
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    const float s = int4_scale(mn, mx), base = int4_base(mn, s);
    const float c0 = int4_code(x0, s, base), c1 = int4_code(x1, s, base);
    kv.data[row * (HD / 2) + lane] = (uint8_t)((unsigned)c0 | ((unsigned)c1 << 4));
    if (lane == 0) {
        kv.param[row * 2] = int4_scale_bits(s);
        kv.param[row * 2 + 1] = int4_zero_bits(base, s);
    }
}

// ---- eight lanes store one row (rope_prefill.hip): lane j of the eight holds elements 8 j .. 8 j + 7 (lo) and 64 + 8 j .. 64 + 8 j + 7
// (hi) as bf16 bits, so a row is two 16-byte accesses per lane and the row's min / max / amax a three-step exchange among the eight.
// The eight lanes are eight adjacent lanes of a wave, all active.
template <int CTRL>
__device__ inline uint32_t dpp(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, CTRL, 0xf, 0xf, false); }
// f over the eight lanes' values: lane ^ 1, lane ^ 2 within the quad (quad_perm), then the mirrored lane of the other quad, which holds
// that quad's result whichever it is (row_half_mirror)
#define MM_KV_REDUCE8(f, x) \
    do { x = f(x, __builtin_bit_cast(decltype(x), dpp<0xb1>(__builtin_bit_cast(uint32_t, x)))); \
         x = f(x, __builtin_bit_cast(decltype(x), dpp<0x4e>(__builtin_bit_cast(uint32_t, x)))); \
         x = f(x, __builtin_bit_cast(decltype(x), dpp<0x141>(__builtin_bit_cast(uint32_t, x)))); } while (0)

// ---- what a reader of a slot gets back, as bf16 bits: the one copy of the rule, for the rows store_row8 has just written and for the
// rows kv_gather.hip finds stored.  fp8: 4 codes (one dword) times scale = 2^e, exact, so the high halves of the fp32 products are the
// values.  int4: two codes as floats 0 .. 15 with the row's fp16 (scale, zero) as stored: the product is exact, so one fp32 and one
// bf16 rounding
__device__ inline v2u fp8_seen(uint32_t codes, float scale) {
    const v2u back = fp8x4_to_bf16(codes);
    v2u r;
    r.x = (__float_as_uint(bf16f(back.x & 0xffffu) * scale) >> 16) | (__float_as_uint(bf16f(back.x >> 16) * scale) & 0xffff0000u);
    r.y = (__float_as_uint(bf16f(back.y & 0xffffu) * scale) >> 16) | (__float_as_uint(bf16f(back.y >> 16) * scale) & 0xffff0000u);
    return r;
}
__device__ inline uint32_t int4_seen(float c0, float c1, float sf, float zf) { return pack_bf(c0 * sf - zf, c1 * sf - zf); }

// the K (which = 0) or V (which = 1) row of head h, given the K row of head 0 of the same page and slot (kv_row)
__device__ inline int64_t row_of(const PagedKV &kv, int64_t k_row0, int which, int h) { return k_row0 + ((int64_t)which * kv.Hkv + h) * kv.P; }

// Writes row `row` of the cache by the kind's rule -- the bytes store_row writes -- unless row < 0, and leaves in lo / hi the bf16 values a
// reader of the slot gets back: int4 bf16(code * scale - zero) in fp32 (the product is exact, so one fp32 and one bf16 rounding), fp8
// code * 2^e (exact), bf16 the values themselves.  No byte-wide stores: int4 two dwords of codes, fp8 two 8-byte stores, bf16 two
// 16-byte stores per lane; lane 0 of the eight stores the (scale, zero) dword.
template <int KIND>
__device__ inline void store_row8(const PagedKV &kv, int64_t row, int j, v4u &lo, v4u &hi) {
    if (KIND == KV_BF16) {
        if (row >= 0) {
            v4u *dst = (v4u *)kv.data + row * (HD / 8);
            dst[j] = lo;
            dst[HD / 16 + j] = hi;
        }
        return;
    }
    if (KIND == KV_FP8) {
        uint32_t amax = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) amax = max(max(amax, max(lo[m] & 0x7fffu, (lo[m] >> 16) & 0x7fffu)), max(hi[m] & 0x7fffu, (hi[m] >> 16) & 0x7fffu));
        MM_KV_REDUCE8(max, amax);
        const int e = fp8_exponent(amax);
        const uint32_t top = fp8_top(e);
        const float scale = __uint_as_float((uint32_t)(127 + e) << 23);
        v2u code[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            v4u &x = half ? hi : lo;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                v2s r = fp8_codes<false>(v2s{0, 0}, fp8_clamp(x[2 * m], top), e);
                r = fp8_codes<true>(r, fp8_clamp(x[2 * m + 1], top), e);
                code[half][m] = __builtin_bit_cast(uint32_t, r);
                const v2u seen = fp8_seen(code[half][m], scale);
                x[2 * m] = seen.x;
                x[2 * m + 1] = seen.y;
            }
        }
        if (row >= 0) {
            v2u *dst = (v2u *)kv.data + row * (HD / 8);
            dst[j] = code[0];
            dst[HD / 16 + j] = code[1];
            if (j == 0) ((uint32_t *)kv.param)[row] = fp8_param(e);
        }
        return;
    }
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        mn = fminf(fminf(mn, fminf(bf16f(lo[m] & 0xffffu), bf16f(lo[m] >> 16))), fminf(bf16f(hi[m] & 0xffffu), bf16f(hi[m] >> 16)));
        mx = fmaxf(fmaxf(mx, fmaxf(bf16f(lo[m] & 0xffffu), bf16f(lo[m] >> 16))), fmaxf(bf16f(hi[m] & 0xffffu), bf16f(hi[m] >> 16)));
    }
    MM_KV_REDUCE8(fminf, mn);
    MM_KV_REDUCE8(fmaxf, mx);
    const float s = int4_scale(mn, mx), base = int4_base(mn, s);
    const unsigned short sb = int4_scale_bits(s), zb = int4_zero_bits(base, s);
    const float sf = __half2float(__ushort_as_half(sb)), zf = __half2float(__ushort_as_half(zb));    // as a reader finds them
    uint32_t code[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        v4u &x = half ? hi : lo;
        code[half] = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float c0 = int4_code(bf16f(x[m] & 0xffffu), s, base), c1 = int4_code(bf16f(x[m] >> 16), s, base);
            code[half] |= ((unsigned)c0 | ((unsigned)c1 << 4)) << (8 * m);
            x[m] = int4_seen(c0, c1, sf, zf);
        }
    }
    if (row >= 0) {
        uint32_t *dst = (uint32_t *)kv.data + row * (HD / 8);
        dst[j] = code[0];
        dst[HD / 16 + j] = code[1];
        if (j == 0) ((uint32_t *)kv.param)[row] = (uint32_t)sb | ((uint32_t)zb << 16);
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
