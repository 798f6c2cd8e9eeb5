// LDS sizes of the decode quantization phase (mx_decode_quant.h): plain C++ without a HIP include, shared by the kernels, by the
// launchers of qlinear_decode.hip and by the host-only plan of the streaming kernels (mx_stream_plan.h).
#pragma once
#include <stddef.h>

namespace mm {
namespace dq {
constexpr size_t operand_bytes(int M, const int K[3]) {   // quantized rows + their scale bytes
    const size_t Kt = (size_t)K[0] + K[1] + K[2];
    return (size_t)M * (K[0] / 2 + K[1] / 4 * 3 + K[2] + Kt / 32);
}
// LDS behind the (16-byte rounded) operands when the norm runs inside the launch: [K bf16 norm weights | M x P partial sums | M rvar]
constexpr int rms_pow2(int T) { int P = 64; while (P < T) P <<= 1; return P; }
constexpr size_t rms_bytes(int M, const int K[3]) {
    const size_t Kt = (size_t)K[0] + K[1] + K[2];
    return Kt * 2 + (size_t)M * rms_pow2((int)(Kt >> 5)) * 4 + 64;
}
constexpr int RMS_MAX_K = 8192;      // the wave-local halving tree covers P <= 256 partial sums
// quantize_rows_early applies: at most `npass` (row, group, half) slots per thread of a workgroup of NT
constexpr bool early_fits(int M, int Kt, int NT, int npass) { return 2 * (size_t)M * (size_t)(Kt >> 5) <= (size_t)NT * npass; }
}  // namespace dq
}  // namespace mm
