// The RoPE element rule of include/micromix_hip.h (mm_rope_kv_append), shared by rope_append.hip and rope_prefill.hip: HF's
// apply_rotary_pos_emb in bf16 tensor arithmetic, x * cos + rotate_half(x) * sin with every op rounded to bf16:
//   a = bf16(x[d] * cos[d]);  b = bf16((d < 64 ? -x[d + 64] : x[d - 64]) * sin[d]);  y[d] = bf16(a + b)
// in fp32 (a product of two bf16 values is exact there), round to nearest even.  The roundings between the ops leave nothing to contract.
#pragma once
#include <stdint.h>

#include "mx_paged_kv.h"

namespace mm {
namespace kv {

// bf16(bf16(x * c) + bf16(r * s)) for one element; r is the element's rotate_half partner with its sign applied (a flipped sign bit)
__device__ inline uint32_t rope_one(uint32_t x, uint32_t r, uint32_t c, uint32_t s) {
    const uint32_t a = f2bf_rne(bf16f(x) * bf16f(c)), b = f2bf_rne(bf16f(r) * bf16f(s));
    return f2bf_rne(bf16f(a) + bf16f(b));
}

// the rotated elements 2 lane, 2 lane + 1 of a row that a wave holds one dword per lane; the whole wave calls it
__device__ inline uint32_t rope_pair(uint32_t x, uint32_t cs, uint32_t sn, int lane) {
    // lanes 32..63 of the first operand change places with lanes 0..31 of the second, so in every lane one of the two results is the
    // dword of lane ^ 32 and the other the lane's own: the xor of the three is the partner's
    const auto sw = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    const uint32_t r = sw[0] ^ sw[1] ^ x ^ (lane < 32 ? 0x80008000u : 0u);     // rotate_half: -x[d + 64] below 64, x[d - 64] above
    return rope_one(x & 0xffffu, r & 0xffffu, cs & 0xffffu, sn & 0xffffu) | (rope_one(x >> 16, r >> 16, cs >> 16, sn >> 16) << 16);
}

}  // namespace kv
}  // namespace mm
