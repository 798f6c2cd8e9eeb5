// The append side of the paged KV cache, shared by kv_append_kernel (kv_cache.hip) and rope_kv_append_kernel (rope_append.hip): where a
// new token's row lies (append_row) and what is written there (store_row: the int4 rule of include/micromix_hip.h, or a bf16 copy).
// One copy of both, so the two kernels cannot drift apart.  A wave owns a (token, head) row, lane l its elements 2 l and 2 l + 1.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

namespace mm {
namespace kva {

constexpr int HD = 128;            // head_dim

__device__ inline float bf16f(uint32_t bits16) { return __uint_as_float(bits16 << 16); }

__device__ inline uint16_t f2bf_rne(float f) {    // finite inputs
    const uint32_t u = __float_as_uint(f);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ inline __half sat_half(float x) { return __float2half_rn(fminf(fmaxf(x, -65504.0f), 65504.0f)); }

// the sequence a flat index belongs to: the largest b with indptr[b] <= i (empty sequences are skipped over)
__device__ inline int find_seq(const int *indptr, int B, int i) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (indptr[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ inline int seq_len(const int *kv_indptr, const int *last_page_len, int b, int P) {
    const int np = kv_indptr[b + 1] - kv_indptr[b];
    return np > 0 ? (np - 1) * P + min(max(last_page_len[b], 0), P) : 0;    // clamped: a bad entry never reads past the page list
}

// row index (in rows of one token-head) of K (kv = 0) or V (kv = 1) of `page`, `slot`
__device__ inline int64_t kv_row(int page, int L, int layer, int kv, int Hkv, int h, int P, int slot) {
    return ((((int64_t)page * L + layer) * 2 + kv) * Hkv + h) * P + slot;
}

// the K (kv = 0) or V (kv = 1) row of appended token i, head h; -1: nothing is written for this token
__device__ inline int64_t append_row(const int *kv_indptr, const int *kv_indices, const int *last_page_len, const int *append_indptr, int B,
                                     int i, int max_pages, int L, int layer, int kv, int Hkv, int h, int P) {
    const int b = find_seq(append_indptr, B, i);
    const int len = seq_len(kv_indptr, last_page_len, b, P);
    const int pos = len - (append_indptr[b + 1] - append_indptr[b]) + (i - append_indptr[b]);
    if (pos < 0 || pos >= len) return -1;                     // a table that does not count the appended tokens: nothing written
    const int page = kv_indices[kv_indptr[b] + pos / P];
    if (page < 0 || page >= max_pages) return -1;
    return kv_row(page, L, layer, kv, Hkv, h, P, pos % P);
}

// the whole wave stores one row: `two` = this lane's elements 2 lane, 2 lane + 1 (bf16 bits)
template <bool INT4>
__device__ inline void store_row(uint8_t *kv_data, __half *kv_param, int64_t row, int lane, uint32_t two) {
    if (!INT4) {
        ((uint32_t *)kv_data)[row * (HD / 2) + lane] = two;
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
    kv_data[row * (HD / 2) + lane] = (uint8_t)((unsigned)c0 | ((unsigned)c1 << 4));
    if (lane == 0) {
        kv_param[row * 2] = __float2half_rn(s);
        kv_param[row * 2 + 1] = sat_half(fabsf(base * s));   // base = clamp(-0.0) has no defined sign: a zero `zero` is stored as +0.0
    }
}

}  // namespace kva
}  // namespace mm
