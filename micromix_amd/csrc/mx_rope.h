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

}  // namespace kv
}  // namespace mm
