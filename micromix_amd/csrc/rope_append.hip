// RoPE + paged KV append in one launch (include/micromix_hip.h, mm_rope_kv_append): reads q | k | v as the fused q/k/v projection leaves
// them (three pointers, one token stride), rotates q and K by the caller's bf16 cos / sin rows, writes the rotated q contiguous and the
// rotated K and V into the cache by the slot rule and the int4 / fp8 rule of mm_kv_append (mx_paged_kv.h: the same code).
//
// RoPE is HF's apply_rotary_pos_emb in bf16 tensor arithmetic, x * cos + rotate_half(x) * sin with every op rounded to bf16:
//   a = bf16(x[d] * cos[d]);  b = bf16((d < 64 ? -x[d + 64] : x[d - 64]) * sin[d]);  y[d] = bf16(a + b)
// in fp32 (a product of two bf16 values is exact there), round to nearest even.  The roundings between the ops leave nothing to contract.
//
// One workgroup per (token, kv head): wave 0 rotates and stores K, wave 1 stores V, the other waves rotate the kv head's g query heads.
// A lane owns elements 2 lane, 2 lane + 1 of a 128-wide row as one dword, so its rotate_half partner is the same dword of lane ^ 32: one
// v_permlane32_swap, no LDS.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <type_traits>

#include "mx_kernels.h"
#include "mx_paged_kv.h"
#include "mx_qknorm.h"            // qknorm_pair: QK-norm of a wave's row ahead of its rotation (NORM, mm_rope_kv_append_qknorm)
#include "mx_rope.h"              // rope_one: the element rule, shared with rope_prefill.hip; rope_pair: a wave's row, with decode_step.hip

namespace {

using namespace mm::kv;

constexpr int MAX_Q_WAVES = 6;     // query heads beyond these are taken in further rounds (no limit on g)

struct RopeArgs {
    mm::PagedKV kv;
    const int *append_indptr;
    const uint16_t *q, *k, *v, *cos, *sin;
    uint16_t *q_out;
    int64_t qkv_stride, cs_stride;     // elements per token
    int Hq, g;
};

struct RopeNormArgs : RopeArgs {
    const uint16_t *q_weight, *k_weight;       // bf16 [128] each
    float eps;
};

// NORM: q and k rows pass mx_qknorm.h's rule before the rotation; a wave loads its dword of the weight once, next to cos / sin
template <int KIND, bool NORM>
__global__ __launch_bounds__(64 * (2 + MAX_Q_WAVES)) void rope_kv_append_kernel(const std::conditional_t<NORM, RopeNormArgs, RopeArgs> a) {
    const int i = blockIdx.x, h = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t in = (int64_t)i * a.qkv_stride;
    if (wave == 1) {                                          // V: as mm_kv_append
        const uint32_t two = ((const uint32_t *)(a.v + in + (int64_t)h * HD))[lane];
        const int64_t row = append_row(a.kv, a.append_indptr, i, 1, h);
        if (row >= 0) store_row<KIND>(a.kv, row, lane, two);
        return;
    }
    const uint32_t cs = ((const uint32_t *)(a.cos + (int64_t)i * a.cs_stride))[lane];
    const uint32_t sn = ((const uint32_t *)(a.sin + (int64_t)i * a.cs_stride))[lane];
    [[maybe_unused]] uint32_t w = 0;
    if constexpr (NORM) w = ((const uint32_t *)(wave == 0 ? a.k_weight : a.q_weight))[lane];
    if (wave == 0) {                                          // K
        uint32_t two = ((const uint32_t *)(a.k + in + (int64_t)h * HD))[lane];
        if constexpr (NORM) two = qknorm_pair(two, w, a.eps);
        two = rope_pair(two, cs, sn, lane);
        const int64_t row = append_row(a.kv, a.append_indptr, i, 0, h);
        if (row >= 0) store_row<KIND>(a.kv, row, lane, two);
        return;
    }
    // q: every token, whatever its cache slot
    const int nq = (int)(blockDim.x >> 6) - 2;
    for (int j = wave - 2; j < a.g; j += nq) {
        const int hq = h * a.g + j;
        uint32_t two = ((const uint32_t *)(a.q + in + (int64_t)hq * HD))[lane];
        if constexpr (NORM) two = qknorm_pair(two, w, a.eps);
        // stored as a float: a store of an integer type here may alias the page table for all the compiler knows, and then wave 0 and
        // wave 1 read the table (append_row) with vector loads instead of scalar ones (7 % of the launch at T = 4096)
        ((float *)(a.q_out + ((int64_t)i * a.Hq + hq) * HD))[lane] = __uint_as_float(rope_pair(two, cs, sn, lane));
    }
}

}  // namespace

namespace mm {

// q_weight != nullptr: the QK-norm form, both weights given
hipError_t launch_rope_kv_append(const PagedKV &kv, const void *q, const void *k, const void *v, int64_t qkv_stride, int Hq, const void *cos,
                                 const void *sin, int64_t cs_stride, const int *append_indptr, int T, void *q_out, hipStream_t stream,
                                 const void *q_weight, const void *k_weight, float eps) {
    RopeNormArgs a;
    a.kv = kv;
    a.append_indptr = append_indptr;
    a.q = (const uint16_t *)q;
    a.k = (const uint16_t *)k;
    a.v = (const uint16_t *)v;
    a.cos = (const uint16_t *)cos;
    a.sin = (const uint16_t *)sin;
    a.q_out = (uint16_t *)q_out;
    a.qkv_stride = qkv_stride;
    a.cs_stride = cs_stride;
    a.Hq = Hq;
    a.g = Hq / kv.Hkv;
    a.q_weight = (const uint16_t *)q_weight;
    a.k_weight = (const uint16_t *)k_weight;
    a.eps = eps;
    const dim3 grid(T, kv.Hkv);
    const int threads = 64 * (2 + (a.g < MAX_Q_WAVES ? a.g : MAX_Q_WAVES));
    const RopeArgs &plain = a;
    if (q_weight) {
        if (kv.kind == KV_INT4) rope_kv_append_kernel<KV_INT4, true><<<grid, threads, 0, stream>>>(a);
        else if (kv.kind == KV_FP8) rope_kv_append_kernel<KV_FP8, true><<<grid, threads, 0, stream>>>(a);
        else rope_kv_append_kernel<KV_BF16, true><<<grid, threads, 0, stream>>>(a);
    } else if (kv.kind == KV_INT4) rope_kv_append_kernel<KV_INT4, false><<<grid, threads, 0, stream>>>(plain);
    else if (kv.kind == KV_FP8) rope_kv_append_kernel<KV_FP8, false><<<grid, threads, 0, stream>>>(plain);
    else rope_kv_append_kernel<KV_BF16, false><<<grid, threads, 0, stream>>>(plain);
    return hipGetLastError();
}

}  // namespace mm
