// The integer arithmetic of mm_spec_sample_rows (include/micromix_spec.h): the 24-bit uniform number, mulshift, the accept predicate and
// a token's residual mass, in 128-bit integers.  Plain C++ with no HIP call, so the host includes it too: tools/spec_rule_host_check.cpp
// runs these very functions against Python integers (tests/test_spec_sample_cpu.py).  No 128-bit division anywhere.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MM_SPEC_HD __host__ __device__
#else
#define MM_SPEC_HD
#endif

namespace mm {

typedef unsigned __int128 u128;

// U = trunc(u * 2^24) of a uniform number as mm_sample_rows reads it: NaN -> 0, else clamped to [0, 1 - 2^-24].  The product is exact
MM_SPEC_HD inline unsigned spec_u24(float u) {
    const float c = u > 0.0f ? (u < 1.0f - 0x1p-24f ? u : 1.0f - 0x1p-24f) : 0.0f;
    return (unsigned)(c * 0x1p24f);
}

// floor(U * z / 2^24) for U < 2^24, exactly, without a product beyond 128 bits: z = 2^24 a + b gives U a + floor(U b / 2^24).  < z for z > 0
MM_SPEC_HD inline u128 spec_mulshift(u128 z, unsigned U) {
    return (z >> 24) * U + (((z & (u128)0xFFFFFFu) * U) >> 24);
}

// the candidate x survives: floor(U_a * Q_x Z_p / 2^24) < P_x Z_q, masses <= 2^43 and sums < 2^63, so both products are below 2^106
MM_SPEC_HD inline bool spec_accept(unsigned long long Px, unsigned long long Zp, unsigned long long Qx, unsigned long long Zq, unsigned Ua) {
    return spec_mulshift((u128)Qx * Zp, Ua) < (u128)Px * Zq;
}

// R_i = max(0, P_i Z_q - Q_i Z_p): the mass the target gives token i beyond the draft's, both scaled to the common denominator Z_p Z_q
MM_SPEC_HD inline u128 spec_residual(unsigned long long Pi, unsigned long long Zp, unsigned long long Qi, unsigned long long Zq) {
    const u128 a = (u128)Pi * Zq, b = (u128)Qi * Zp;
    return a > b ? a - b : (u128)0;
}

}  // namespace mm
