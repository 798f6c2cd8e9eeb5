// The 16-bit key of a bf16 value and the wave reductions over it, shared by verify.hip (mm_argmax_rows) and sample.hip (mm_sample_rows).
//
// Every value gets a key that grows with it, on the bf16 bits alone: -inf 0x0000, the negative numbers up to -0 == +0 at 0x7F80, the
// positive ones up to +inf 0xFF00, and every NaN, of either sign, 0xFF01.  Equal keys are equal values (both zeros included), so a key
// names a class of tokens with one logit, its high byte a level-1 bin of a radix select and its low byte the level-2 bin inside it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

typedef unsigned short us8 __attribute__((ext_vector_type(8)));
typedef short ss8 __attribute__((ext_vector_type(8)));

constexpr unsigned KEY_NAN = 0xFF01u, KEY_POS_INF = 0xFF00u, BF16_NEG_INF = 0xFF80u;

// the keys of 8 bf16 values: |x| with every NaN clamped to one value, negated for a set sign bit, shifted to unsigned; -NaN wraps
// around to 0xFFFF and the last min brings it back to +NaN's key
__device__ inline us8 argmax_keys(us8 u) {
    const us8 mag = __builtin_elementwise_min(u & (us8)0x7FFF, (us8)0x7F81);
    const us8 neg = (us8)((ss8)u >> 15);
    const us8 s = (mag ^ neg) - neg;
    return __builtin_elementwise_min(s + (us8)0x7F80, (us8)KEY_NAN);
}

__device__ inline unsigned argmax_key(unsigned u) {                                  // the same for one value
    const unsigned mag = min(u & 0x7FFFu, 0x7F81u), neg = (u & 0x8000u) ? 0xFFFFu : 0u;
    return min((((mag ^ neg) - neg) + 0x7F80u) & 0xFFFFu, KEY_NAN);
}

// a token id that names a column of the row (mm_spec_sample_rows' candidates: anything else means "no candidate")
__device__ inline bool in_vocab(int x, int vocab) { return x >= 0 && x < vocab; }

__device__ inline unsigned wave_max(unsigned x) {
#pragma unroll
    for (int off = 32; off; off >>= 1) x = max(x, (unsigned)__shfl_xor((int)x, off));
    return x;
}
__device__ inline unsigned wave_min(unsigned x) {
#pragma unroll
    for (int off = 32; off; off >>= 1) x = min(x, (unsigned)__shfl_xor((int)x, off));
    return x;
}

}  // namespace mm
