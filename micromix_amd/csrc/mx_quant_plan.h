// Host side of the activation quantizers (reorder_quantize.hip, rmsnorm_quantize.hip, qlinear_decode.hip): which kernel a launch runs
// on, with how many threads, how much dynamic LDS and what limit to raise.  Plain C++ without a HIP include, in the manner of
// mx_stream_plan.h: everything takes the CU count and the developer overrides as arguments (tools/quant_plan_host_check.cpp checks the
// invariants the kernels depend on over CU counts from 1 to 1024 and every K up to 32768, tests/test_quant_dispatch_cpu.py replays a
// sweep recorded before this header existed).  A launcher has three steps: plan, pick the instantiation from the plan, launch.
#pragma once
#include <stddef.h>

#include "mx_decode_quant_sizes.h"   // dq::operand_bytes, rms_bytes: the LDS of the decode launches' quantization phase
#include "mx_launch_shape.h"

namespace mm {
namespace quant {

// A kernel's dynamic-LDS limit is raised once a launch needs more than this (the default limit is 64 KiB; 48 KiB is what every
// toolchain grants), to the largest size its family reaches.
constexpr int LDS_RAISE_ABOVE = 48 * 1024;
constexpr int REORDER_LDS_MAX = 96 * 1024;     // K = 32768: the row, 64 KiB, + the image of its fp6 / fp8 codes, at most 32 KiB
constexpr int RMS_LDS_MAX = 104 * 1024;        // ... + the partial sums (K = 32768: 100 KiB); the ring of four 16 KiB slots: 74 KiB
constexpr int DECODE_LDS_MAX = 126 * 1024;     // the decode launch takes what its static 32 KB reduction buffer leaves of a CU's LDS
constexpr int raise_for(int lds, int family_max) { return lds > LDS_RAISE_ABOVE ? family_max : 0; }
constexpr int roundup64(int n) { return (n + 63) / 64 * 64; }

// One resident wave of workgroups (no tail), each striding over the rows, and at most `rows` of them; a grouped launch's `ngroups`
// groups share the wave (at least one workgroup each, at most the largest group's rows).  per_cu: the occupancy query's answer -- only
// the device knows it.
constexpr int resident_grid(int rows, int cus, int per_cu, int ngroups = 1) {
    const int wave = cus * per_cu / ngroups < 1 ? 1 : cus * per_cu / ngroups;
    return rows < wave ? rows : wave;
}

// ---- reorder_quantize.hip: the plain, the grouped and the two device-sized launches (moe_activate_quantize: w4 = false) ----
// One thread per 32-group of the output and per four 16-byte chunks of the K-wide input row, whichever are more; the kernels exist
// with __launch_bounds__ of 256 and of 1024.  LDS: the staged row + (matching-precision weights) the image of its fp6 / fp8 codes.
struct ReorderPlan {
    int threads;
    int max_threads;      // 256 or 1024: the instantiation
    int lds_bytes, raise_to;
    constexpr LaunchShape shape(int grid_x, int grid_y = 1) const { return LaunchShape{grid_x, grid_y, threads, lds_bytes, raise_to}; }
};
constexpr ReorderPlan plan_reorder_quantize(int K, int KN, int KS, int KO, bool w4) {
    const int G = (KN + KS + KO) / 32, stagers = K / 32;
    const int threads = roundup64(G > stagers ? G : stagers);
    const int lds = K * 2 + (w4 ? 0 : KS / 4 * 3 + KO);
    return ReorderPlan{threads, threads <= 256 ? 256 : 1024, lds, raise_for(lds, REORDER_LDS_MAX)};
}

// ---- rmsnorm_quantize.hip ----
// K <= 8192 (256 threads): the LDS-DMA ring or the kernel that stages fp32 products; beyond, the kernel that stages the 16-bit row with
// one (K <= 16384) or two of the reference's group threads per thread, at most 512 threads.  The ring moves global memory straight to
// LDS and cannot add on the way: no ring with the residual.
// Measured (tools/time_rmsnorm.py, K = 4096, us, products / ring of 3): 256 rows 7.5 / 5.8 -- the ring kernel's prologue requests its
// first rows before anything else -- but 4096 rows 11.6 / 14.7: with several rows per workgroup the launch is bound by the per-row
// instruction stream (the integer rounding alone is 1.5 us of it), not by bytes in flight, and the ring kernel reads its row back from
// LDS for the sum of squares.  So: the ring while a workgroup sees at most ~2 rows (rows <= 2 x CUs), the products kernel beyond.
// ring_pin (MICROMIX_RMS_RING): negative unset, 0 never the ring, 3 / 4 always with that depth.
enum RmsKernel { RMS_RING3, RMS_RING4, RMS_PRODUCTS, RMS_STAGED1, RMS_STAGED2 };
constexpr int RMS_RING_MAX_K = 8192;
constexpr int rms_max_threads(RmsKernel k) { return k == RMS_STAGED1 || k == RMS_STAGED2 ? 512 : 256; }     // the kernels' __launch_bounds__
constexpr int rms_ring_depth(RmsKernel k) { return k == RMS_RING3 ? 3 : k == RMS_RING4 ? 4 : 0; }
struct RmsPlan {
    RmsKernel kernel;
    int threads;
    int P;                // the halving tree's width: the next power of two over the K / 32 partial sums, at least 64
    int pslots;           // floats of LDS kept for the partial sums
    int slot_bytes;       // ring kernels: one slot of the ring, the row rounded up to whole 1 KB pieces
    int lds_bytes, raise_to;
    constexpr LaunchShape shape(int grid_x) const { return LaunchShape{grid_x, 1, threads, lds_bytes, raise_to}; }
};
constexpr RmsPlan plan_rmsnorm_quantize(int rows, int K, int KS, int KO, bool add, int cus, int ring_pin) {
    const int T = K / 32;
    const int gpt = T > 512 ? 2 : 1;
    // (the ring kernel's counted vmcnt needs exactly roundup64(K / 32) threads -- every wave's lane 0 owns a group; it traps otherwise)
    const int threads = roundup64((T + gpt - 1) / gpt);
    const int P = dq::rms_pow2(T);
    const int image = KS / 4 * 3 + KO;
    const bool products = threads <= 256;
    const int ring = add ? 0 : (ring_pin >= 0 ? ring_pin : (rows <= 2 * cus ? 3 : 0));
    if (products && ring >= 3) {
        const int R = ring >= 4 ? 4 : 3, slot = (K * 2 + 1023) / 1024 * 1024, pslots = P > threads ? P : threads;
        const int lds = R * slot + 1024 + pslots * 4 + image;      // [R slots][1 KB dump][partial sums][image of the S | O codes]
        return RmsPlan{R == 4 ? RMS_RING4 : RMS_RING3, threads, P, pslots, slot, lds, raise_for(lds, RMS_LDS_MAX)};
    }
    const int pslots = P > gpt * threads ? P : gpt * threads;
    const int lds = K * (products ? 4 : 2) + pslots * 4 + image;   // [row: fp32 products or bf16][partial sums][image]
    return RmsPlan{products ? RMS_PRODUCTS : (gpt == 1 ? RMS_STAGED1 : RMS_STAGED2), threads, P, pslots, 0, lds, raise_for(lds, RMS_LDS_MAX)};
}

// ---- qlinear_decode.hip: M <= 8 rows, every workgroup quantizes them itself ----
constexpr int DECODE_THREADS = 512;      // = decode::NT (static_asserted in qlinear_decode.hip)
// dynamic LDS: the quantized rows and scales of all M rows (+ the norm's range) + as many staged bf16 rows as fit
constexpr size_t decode_operand_bytes(int M, const int K[3], bool rms) {
    return rms ? ((dq::operand_bytes(M, K) + 15) & ~(size_t)15) + dq::rms_bytes(M, K) : dq::operand_bytes(M, K);
}
// features per workgroup: 16 while 32 would leave half of the CUs without a workgroup
constexpr int decode_features(int N, int cus) { return 2 * ((N + 31) / 32) <= cus ? 16 : 32; }
// at least one staged row fits beside the operands (qlinear_decode_supported asks; the plan below relies on it)
constexpr bool decode_fits(int M, const int K[3], bool rms) {
    return M >= 1 && M <= 8 && ((size_t)K[0] + K[1] + K[2]) * 2 + decode_operand_bytes(M, K, rms) <= (size_t)DECODE_LDS_MAX;
}
struct DecodePlan {
    int features;         // 16 or 32 per workgroup
    int stage_rows;       // activation rows staged in LDS at a time
    bool pairs;           // lane pairs in the quantization phase: one pass of the workgroup covers every (row, group, half) slot
    int lds_bytes, raise_to, blocks;
    constexpr LaunchShape shape() const { return LaunchShape{blocks, 1, DECODE_THREADS, lds_bytes, raise_to}; }
};
// persist (MICROMIX_DECODE_PERSIST, default on): the 32-feature kernel walks its feature blocks, one workgroup per CU.  Measured
// (tools/time_decode.py, K = 4096, (2048,128,1920), one box, us at M = 1 / 4 / 8): gate/up N = 14336 one workgroup per block 13.0 /
// 16.0 / 20.2, one per CU 11.4 / 13.4 / 15.8, two per CU 13.1 / 16.1 / 20.2; fused gate + up N = 28672: 26.1 / 32.3 / 40.2 against
// 20.9 / 23.1 / 25.4 (two per CU 22.7 / 26.6 / 31.3).  Off restores one workgroup per block (A/B runs).
// (rms, add and w4 pick the instantiation; only rms changes a number)
constexpr DecodePlan plan_qlinear_decode(int M, int N, const int K[3], bool rms, bool /*add*/, bool /*w4*/, int cus, bool persist) {
    const size_t Kt = (size_t)K[0] + K[1] + K[2], ops = decode_operand_bytes(M, K, rms);
    const size_t fit = ((size_t)DECODE_LDS_MAX - ops) / (Kt * 2);
    const int stage_rows = fit > (size_t)M ? M : (int)fit;
    const int features = decode_features(N, cus);
    int blocks = (N + features - 1) / features;
    if (features == 32 && persist && blocks > cus) blocks = cus;
    return DecodePlan{features, stage_rows, 2 * (size_t)stage_rows * (Kt / 32) <= (size_t)DECODE_THREADS, (int)((size_t)stage_rows * Kt * 2 + ops),
                      DECODE_LDS_MAX, blocks};
}

}  // namespace quant
}  // namespace mm
