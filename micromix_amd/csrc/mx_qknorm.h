// QK-norm (Qwen3's q_norm / k_norm): HF's Qwen3RMSNorm over one 128-element bf16 row of q or k, ahead of mx_rope.h's element rule.
// The one copy of the rule (include/micromix_qknorm.h states it for callers) and its three register layouts: rope_append.hip and the
// K row of decode_step.hip (a dword per lane), rope_prefill.hip (eight lanes per row), the q operand of decode_step.hip (two 32-element
// blocks per lane).  For a row x, weight w (bf16 [128]) and eps:
//   1  p[l] = x[2l]^2 + x[2l+1]^2 in fp32, l = 0 .. 63.  The squares of bf16 values are exact in fp32, so this is one rounding, and the
//      fma the compiler may contract it into gives the same bits.
//   2  S = the sum of the 64 p[l] in ONE binary tree: partners whose index l differs in bit 0 are added first, then bit 1, 2, 3, 5, 4,
//      in that order.  fp32 addition is commutative, so both sides of a butterfly step get the same bits and every lane ends with S.
//      Why 5 before 4: in two of the three layouts bit 5 of l is in the lane (the row's low and high half, the block and its rotate_half
//      partner) and bit 4 is the neighbour, so the tree costs them one cross-lane step; a wave with a dword per lane pays six either way.
//   3  r = 1 / sqrt(S * 2^-7 + eps): the scaling is exact, the sum one rounding (contracted or not), then the correctly rounded square
//      root and divide of the RMSNorm quantizer (rmsnorm_quantize.hip says why not __fsqrt_rn or v_rsq_f32).
//   4  n[d] = bf16_rne(fp32(x[d]) * r);  y[d] = bf16_rne(fp32(w[d]) * fp32(n[d])): HF's hidden.to(bf16), then weight * hidden in bf16.
//   5  y goes through rope_one / rope_pair unchanged.
// Finite inputs.  No LDS, no scratch: DPP within a row of 16 lanes, v_permlane16_swap / v_permlane32_swap across rows.
#pragma once
#include <stdint.h>

#include "mx_paged_kv.h"

namespace mm {
namespace kv {

// step 1 for the pair of elements a dword holds
__device__ inline float qkn_square(uint32_t two) {
    const float x0 = bf16f(two & 0xffffu), x1 = bf16f(two >> 16);
    return x0 * x0 + x1 * x1;
}

// step 3
__device__ inline float qkn_rscale(float S, float eps) { return __fdiv_rn(1.0f, __builtin_sqrtf(S * 0.0078125f + eps)); }

// step 4 for a dword of x and the same dword of w
__device__ inline uint32_t qkn_scale(uint32_t two, float r, uint32_t w) {
    const uint32_t n0 = f2bf_rne(bf16f(two & 0xffffu) * r), n1 = f2bf_rne(bf16f(two >> 16) * r);
    return (uint32_t)f2bf_rne(bf16f(w & 0xffffu) * bf16f(n0)) | ((uint32_t)f2bf_rne(bf16f(w >> 16) * bf16f(n1)) << 16);
}

template <int CTRL>
__device__ inline float qkn_dpp(float x) { return __uint_as_float(dpp<CTRL>(__float_as_uint(x))); }

// x + the x of lane ^ 16 / lane ^ 32: the swap leaves, in its two results, the lane's own value and its partner's in either order
__device__ inline float qkn_add_xor16(float x) {
    const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}
__device__ inline float qkn_add_xor32(float x) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}

// ---- a wave holds the row, dword l in lane l (rope_pair's layout); the whole wave calls it.  Six cross-lane steps: lane ^ 1, lane ^ 2
// (quad_perm), then the mirrored lane of the other quad and of the other eight (row_half_mirror, row_mirror: after the steps before,
// every lane there holds that group's sum), then lane ^ 32 and lane ^ 16.
__device__ inline uint32_t qknorm_pair(uint32_t two, uint32_t w, float eps) {
    float s = qkn_square(two);
    s += qkn_dpp<0xb1>(s);         // bit 0
    s += qkn_dpp<0x4e>(s);         // bit 1
    s += qkn_dpp<0x141>(s);        // bit 2
    s += qkn_dpp<0x140>(s);        // bit 3
    s = qkn_add_xor32(s);          // bit 5
    s = qkn_add_xor16(s);          // bit 4
    return qkn_scale(two, qkn_rscale(s, eps), w);
}

// ---- eight adjacent lanes hold the row (store_row8's layout): lane j has dwords 4 j .. 4 j + 3 (lo) and 32 + 4 j .. 32 + 4 j + 3 (hi),
// w the same chunks of the weight.  Bits 0 and 1 of l are in the lane, bits 2 and 3 lane j ^ 1 and j ^ 2 on the two halves' sums, bit 5
// the two halves, bit 4 the other quad.
__device__ inline void qknorm_row8(v4u &lo, v4u &hi, const v4u (&w)[2], float eps) {
    float sl = (qkn_square(lo[0]) + qkn_square(lo[1])) + (qkn_square(lo[2]) + qkn_square(lo[3]));
    float sh = (qkn_square(hi[0]) + qkn_square(hi[1])) + (qkn_square(hi[2]) + qkn_square(hi[3]));
    sl += qkn_dpp<0xb1>(sl);       // bit 2
    sh += qkn_dpp<0xb1>(sh);
    sl += qkn_dpp<0x4e>(sl);       // bit 3
    sh += qkn_dpp<0x4e>(sh);
    float s = sl + sh;             // bit 5
    s += qkn_dpp<0x141>(s);        // bit 4
    const float r = qkn_rscale(s, eps);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        lo[m] = qkn_scale(lo[m], r, w[0][m]);
        hi[m] = qkn_scale(hi[m], r, w[1][m]);
    }
}

// ---- a lane holds two 32-element blocks of the row, dwords 16 kq .. 16 kq + 15 (x) and those of block kq ^ 2 (p), as the MFMA A operand
// of the decode walk and its rotate_half partners; lane ^ 16 holds blocks kq ^ 1 and kq ^ 3 of the same row.  Four levels in the lane
// per block, the two blocks (bit 5), then lane ^ 16 (bit 4).  Lanes l and l ^ 16 call it together.  It returns r of step 3: the caller
// applies qkn_scale dword by dword with the weight's blocks kq and kq ^ 2, which it loads as it goes (a lane that held both blocks of
// the weight over the sum would cost the walk behind it a wave of occupancy).
__device__ inline float qkn_block16(const v4u (&x)[4]) {
    float a[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) a[s] = (qkn_square(x[s][0]) + qkn_square(x[s][1])) + (qkn_square(x[s][2]) + qkn_square(x[s][3]));
    return (a[0] + a[1]) + (a[2] + a[3]);
}
__device__ inline float qknorm_blocks_rscale(const v4u (&x)[4], const v4u (&p)[4], float eps) {
    return qkn_rscale(qkn_add_xor16(qkn_block16(x) + qkn_block16(p)), eps);
}

}  // namespace kv
}  // namespace mm
