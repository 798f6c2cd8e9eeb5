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

#include "mx_kernels.h"
#include "mx_paged_kv.h"

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

// bf16(bf16(x * c) + bf16(r * s)) for one element
__device__ inline uint32_t rope_one(uint32_t x, uint32_t r, uint32_t c, uint32_t s) {
    const uint32_t a = f2bf_rne(bf16f(x) * bf16f(c)), b = f2bf_rne(bf16f(r) * bf16f(s));
    return f2bf_rne(bf16f(a) + bf16f(b));
}

// the rotated elements 2 lane, 2 lane + 1 of a row; the whole wave calls it
__device__ inline uint32_t rope_pair(uint32_t x, uint32_t cs, uint32_t sn, int lane) {
    // lanes 32..63 of the first operand change places with lanes 0..31 of the second, so in every lane one of the two results is the
    // dword of lane ^ 32 and the other the lane's own: the xor of the three is the partner's
    const auto sw = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    const uint32_t r = sw[0] ^ sw[1] ^ x ^ (lane < 32 ? 0x80008000u : 0u);     // rotate_half: -x[d + 64] below 64, x[d - 64] above
    return rope_one(x & 0xffffu, r & 0xffffu, cs & 0xffffu, sn & 0xffffu) | (rope_one(x >> 16, r >> 16, cs >> 16, sn >> 16) << 16);
}

template <int KIND>
__global__ __launch_bounds__(64 * (2 + MAX_Q_WAVES)) void rope_kv_append_kernel(const RopeArgs a) {
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
    if (wave == 0) {                                          // K
        const uint32_t two = rope_pair(((const uint32_t *)(a.k + in + (int64_t)h * HD))[lane], cs, sn, lane);
        const int64_t row = append_row(a.kv, a.append_indptr, i, 0, h);
        if (row >= 0) store_row<KIND>(a.kv, row, lane, two);
        return;
    }
    // q: every token, whatever its cache slot
    const int nq = (int)(blockDim.x >> 6) - 2;
    for (int j = wave - 2; j < a.g; j += nq) {
        const int hq = h * a.g + j;
        const uint32_t two = ((const uint32_t *)(a.q + in + (int64_t)hq * HD))[lane];
        // stored as a float: a store of an integer type here may alias the page table for all the compiler knows, and then wave 0 and
        // wave 1 read the table (append_row) with vector loads instead of scalar ones (7 % of the launch at T = 4096)
        ((float *)(a.q_out + ((int64_t)i * a.Hq + hq) * HD))[lane] = __uint_as_float(rope_pair(two, cs, sn, lane));
    }
}

}  // namespace

namespace mm {

hipError_t launch_rope_kv_append(const PagedKV &kv, const void *q, const void *k, const void *v, int64_t qkv_stride, int Hq, const void *cos,
                                 const void *sin, int64_t cs_stride, const int *append_indptr, int T, void *q_out, hipStream_t stream) {
    RopeArgs a;
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
    const dim3 grid(T, kv.Hkv);
    const int threads = 64 * (2 + (a.g < MAX_Q_WAVES ? a.g : MAX_Q_WAVES));
    if (kv.kind == KV_INT4) rope_kv_append_kernel<KV_INT4><<<grid, threads, 0, stream>>>(a);
    else if (kv.kind == KV_FP8) rope_kv_append_kernel<KV_FP8><<<grid, threads, 0, stream>>>(a);
    else rope_kv_append_kernel<KV_BF16><<<grid, threads, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace mm
