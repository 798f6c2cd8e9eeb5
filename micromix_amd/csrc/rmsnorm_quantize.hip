// RMSNorm fused with column-reorder + per-32-group MXFP4/MXFP6/MXFP8 quantize for gfx950.
//
// Reference: rmsnorm_bf16_mixed_kernel, mgemm/src/rmsnorm.cu:95-312 (binding bindings.cpp:257-303).  Per row:
//   rvar  = 1 / sqrt(sum(x^2) / K + eps)                     fp32, the reference's summation order (see below)
//   v[i]  = bf16((float(x[idx[i]]) * float(w[idx[i]])) * rvar)                                    rmsnorm.cu:190-195
//   per 32-group of reordered positions: amax, e = ceil(log2(amax / FMAX)) (amax == 0 -> scale 0.5)       :216-245
//   q[i]  = RNE_fmt(bf16(clamp(round(v[i] * 2^-e), +-FMAX)))     -- the reference rounds to an INTEGER first     :262-267
// (MM_RMS_NO_INTEGER_ROUND drops the round(); the result is then reorder_quantize of the normalised row.)
//
// Summation order (bit-exact against oracle/mx_oracle.py: rmsnorm_rvar): group thread t of T = K/32 adds the squares of
// elements i*K/4 + 8t + j, i = 0..3, j = 0..7, one after the other -- these are exactly the four 16-byte chunks the thread
// stages into LDS -- and the T partial sums meet in the halving tree s[t] += s[t + stride] over the next power of two,
// zero padded (the reference hard-codes that tree for T = 128 and is wrong for its other K; see the oracle's note).
// fp32 divide and square root are the correctly rounded ones (the reference's rsqrt() approximation is not reproducible):
// __fdiv_rn and __builtin_sqrtf.  NOT __fsqrt_rn, which on this toolchain is the native v_sqrt_f32 -- one ulp off for 15 % of
// arguments (tools/probe_rvar.hip); rounds 1-2 used it, and about one row in 7000 then had an element one code off against the
// oracle (found by tests/quant_stress.py in round 3; the fixed test cases had happened to miss it).
//
// Layout as reorder_quantize.hip: one workgroup strides over rows, thread t owns reordered group t, its 32 indices stay in
// registers for the whole launch, the row is staged in LDS by coalesced 16-byte loads.
//   K <= 8192 (rmsnorm_quantize_products_kernel): a thread keeps the norm weights of the four chunks it STAGES (natural order:
//   four coalesced 16-byte loads) and stages the fp32 products x * w -- exact, two 8-bit significands -- so the gather reads the
//   product with one ds_read_b32 and there is no gather of the weights at all.  The 32-bit row is laid out in two planes
//   (elements 0-3 of every chunk, then elements 4-7) so that the staging writes stay whole 16-byte lanes side by side.  Every
//   wave sums the partial sums by itself after ONE barrier (same tree, same order): two barriers per row instead of four.
//   K > 8192 (rmsnorm_quantize_kernel): the 16-bit row and 32 gathered norm weights per thread in registers (the 32-bit row
//   of K = 32768 would not fit the LDS).
#include <stdlib.h>

#include "mx_buffer_ops.h"   // MM_DEVICE_ONLY; make_rsrc, dma16, wait_vmcnt: the ring kernel's LDS-DMA
#include "mx_group_convert.h"
#include "mx_rms_convert.h"
#include "mx_kernels.h"
#include "mx_quant_plan.h"

#define MM_RMS_SCHED_BARRIER() do { MM_DEVICE_ONLY(__builtin_amdgcn_sched_barrier(0);) } while (0)

namespace mm {

//   then convert_group<EL> into global memory (fp4: 16 bytes per lane, whole lines as they are) or into the LDS image of the row's
//   fp6 / fp8 codes (store_code_image, mx_group_convert.h).
template <bool INT_ROUND, bool PRODUCTS>
__device__ __forceinline__ uint32_t rms_group(const uint8_t *__restrict__ row, const uint32_t (&ix)[16], const uint32_t (&wg)[16],
                                              float rvar, int seg, int j, int r, int KN, uint8_t *oN, uint8_t *image, int bytesS) {
    uint32_t v[16];
    const uint32_t amax = rms_gather<PRODUCTS>(row, ix, wg, rvar, v);
    const int fexp = seg == 0 ? ElemTraits<EL_FP4>::FMAX_EXP : seg == 1 ? ElemTraits<EL_FP6>::FMAX_EXP : ElemTraits<EL_FP8>::FMAX_EXP;
    const uint32_t fmant = seg == 0 ? ElemTraits<EL_FP4>::FMAX_MANT : seg == 1 ? ElemTraits<EL_FP6>::FMAX_MANT : ElemTraits<EL_FP8>::FMAX_MANT;
    int e;
    const float scale = rms_scale<INT_ROUND>(v, amax, fexp, fmant, e);
    if (seg == 0) convert_group<EL_FP4, true>(v, scale, oN + (size_t)r * (KN >> 1) + j * 16);
    else if (seg == 1) convert_group<EL_FP6>(v, scale, image + j * 24);
    else convert_group<EL_FP8>(v, scale, image + bytesS + j * 32);
    return (uint32_t)(e + 127);
}

// How a row's 16-byte chunks reach the staging registers (in the spirit of StageLoad / StageSiluMul, reorder_quantize.hip).  load() issues
// the global loads of chunk c = cu + g of row r (grow: that row of src; cu: the workgroup-uniform part of c, g: the thread), chunk() turns
// the registers into the eight bf16 that are staged and summed, keep() runs once per staged chunk for a hook that also stores what it
// staged.  RowLoad, the plain load, is what mm_rmsnorm_quantize stages with.
// (The hook is the kernel's last argument and its type a template parameter: the instantiations with RowLoad are mm_rmsnorm_quantize's
// kernels as they were, register for register; what the residual costs lives in the RowAddResidual instantiations alone.)
struct RowLoad {
    typedef uint4 Regs;
    static constexpr int WAVES_PER_SIMD = 0;      // the products kernel's __launch_bounds__: no bound
    __device__ __forceinline__ Regs load(const uint4 *__restrict__ grow, int, int, int c, int, int) const { return grow[c]; }
    __device__ __forceinline__ uint4 chunk(Regs &t) const { return t; }
    __device__ __forceinline__ void keep(const Regs &, int, int, int, int) const {}
};
// mm_add_rmsnorm_quantize: the staged row is s = bf16(x + res) (add_bf16x8, mx_rms_convert.h); the chunk of `res` travels beside the
// chunk of x, the packed sums go to LDS and into the sum of squares, and leave once for s_out -- the new residual stream.  A row
// belongs to one workgroup and a chunk to one thread, so every byte of s_out is written exactly once.
// (Addresses as uniform base + the thread's 16 g bytes: with one 64-bit address per chunk and tensor in registers the two-group kernel,
// 248 registers with the plain load, spilled 50 of them.)
struct RowAddResidual {
    struct Regs { uint4 x, r; };
    // the products kernel at three waves per SIMD, as with the plain load (158 VGPRs there; the second chunk in flight per lane made it
    // 170 with the integer rounding, two over the 168 that three waves leave each other)
    static constexpr int WAVES_PER_SIMD = 3;
    const uint16_t *__restrict__ res;   // [rows, K]
    uint16_t *__restrict__ s_out;       // [rows, K]
    __device__ __forceinline__ Regs load(const uint4 *__restrict__ grow, int r, int K, int, int cu, int g) const {
        Regs t;
        t.x = (grow + cu)[g];
        t.r = (reinterpret_cast<const uint4 *>(res + (size_t)r * K) + cu)[g];
        return t;
    }
    __device__ __forceinline__ uint4 chunk(Regs &t) const { return t.x = add_bf16x8(t.x, t.r); }
    __device__ __forceinline__ void keep(const Regs &t, int r, int K, int cu, int g) const {
        (reinterpret_cast<uint4 *>(s_out + (size_t)r * K) + cu)[g] = t.x;
    }
};

// GPT = groups per thread.  8192 < K <= 16384: one (K / 32 <= 512 threads).  16384 < K <= 32768: TWO -- thread g plays the reference's group
// threads t = g and g + 512 one after the other, with their indices and norm weights in 2 x 32 registers.  (Rounds 1-5 ran that range with
// 1024 threads, i.e. 128 registers per lane, which this kernel does not fit in: it spilled 12-13 registers, reloaded inside the row
// loop.  Round 6: no kernel of the library may use scratch -- 512 threads have 256 registers each.)
template <bool INT_ROUND, int GPT, class Stage = RowLoad>
__global__ void __launch_bounds__(512)
rmsnorm_quantize_kernel(const uint16_t *__restrict__ src, const uint16_t *__restrict__ weight, float eps, int rows, int K,
                        const int16_t *__restrict__ idx, int KN, int KS, int KO, uint8_t *__restrict__ oN,
                        uint8_t *__restrict__ oS, uint8_t *__restrict__ oO, uint8_t *__restrict__ sfN,
                        uint8_t *__restrict__ sfS, uint8_t *__restrict__ sfO, const Stage hook) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // [K bf16 row][P floats of partial sums]
    const int T = K >> 5;  // the reference's group threads = stager threads: group thread t stages chunks t, T + t, 2T + t, 3T + t
    const int g = threadIdx.x, NTH = (int)blockDim.x;
    // this thread's group threads: t_u = g + u * NTH (GPT = 1: NTH >= T, so t_0 = g alone)
    bool active[GPT];
#pragma unroll
    for (int u = 0; u < GPT; ++u) active[u] = g + u * NTH < T;
    float *part = reinterpret_cast<float *>(smem + (size_t)K * 2);
    int P = 64;
    while (P < T) P <<= 1;
    const int bytesS = KS / 4 * 3;
    const int pslots = P > GPT * NTH ? P : GPT * NTH;
    uint8_t *image = smem + (size_t)K * 2 + (size_t)pslots * 4;   // [row][partial sums][image of the S | O codes]

    // the norm weights of this thread's 32 columns: the weight vector is staged in LDS (coalesced) and gathered from there
    // with the same byte offsets as the row (32 scattered 2-byte global loads per thread cost more than the two rows a
    // workgroup typically processes)
    uint32_t ix[GPT][16], wg[GPT][16];
#pragma unroll
    for (int u = 0; u < GPT; ++u)
        if (active[u]) {
            const int t = g + u * NTH;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                reinterpret_cast<uint4 *>(smem)[swizzle_chunk(i * T + t)] = reinterpret_cast<const uint4 *>(weight)[i * T + t];
        }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < GPT; ++u)
        if (active[u]) {
            const uint4 *p = reinterpret_cast<const uint4 *>(idx + (size_t)(g + u * NTH) * 32);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4 q = p[i];
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t both = swizzle_offsets((w[k] << 1) & 0xFFFEFFFEu);       // byte offsets into a staged (chunk-swizzled) [K] bf16 vector
                    const uint32_t b0 = both & 0xFFFFu, b1 = both >> 16;
                    ix[u][4 * i + k] = b0 | (b1 << 16);
                    wg[u][4 * i + k] = (uint32_t)*reinterpret_cast<const uint16_t *>(smem + b0) |
                                       ((uint32_t)*reinterpret_cast<const uint16_t *>(smem + b1) << 16);
                }
            }
        }
    __syncthreads();   // the row staging below reuses the same LDS bytes
    const int gN = KN >> 5, gS = KS >> 5;
    int seg[GPT], j[GPT], kseg[GPT];
#pragma unroll
    for (int u = 0; u < GPT; ++u) {
        const int t = g + u * NTH;
        if (t < gN) { seg[u] = 0; j[u] = t; kseg[u] = KN; }
        else if (t < gN + gS) { seg[u] = 1; j[u] = t - gN; kseg[u] = KS; }
        else { seg[u] = 2; j[u] = t - gN - gS; kseg[u] = KO; }
    }

    // GPT = 1: the next row's four chunks are loaded into registers before the current row is processed (HBM latency hides under
    // the gather), and stored to LDS -- squares summed on the way -- after the barrier that ends the current row.
    // GPT = 2 fetches each row when it needs it (2 x 4 chunks: the registers go to the second group's indices and weights)
    constexpr bool PREFETCH = GPT == 1;
    // (... all 2 x 4 chunks at once with the plain load.  A hook with two loads per chunk takes them in pairs of chunks, each pair staged and
    // summed before the next is requested: beside 2 x 32 registers of indices and weights the kernel has no room for more in flight --
    // 248 registers with the plain load -- and the order of the sum is the same, chunk after chunk)
    constexpr bool IN_PAIRS = !PREFETCH && sizeof(typename Stage::Regs) > sizeof(uint4);
    typename Stage::Regs stage[IN_PAIRS ? 1 : GPT][IN_PAIRS ? 2 : 4];
    auto fetch = [&](int r) {
        if (r < rows) {
            const uint4 *grow = reinterpret_cast<const uint4 *>(src + (size_t)r * K);
#pragma unroll
            for (int u = 0; u < GPT; ++u)
                if (active[u]) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) stage[u][i] = hook.load(grow, r, K, i * T + g + u * NTH, i * T + u * NTH, g);
                }
        }
    };
    // chunk i of group thread t_u: staged, its squares added to `sum`
    auto stage_chunk = [&](typename Stage::Regs &t, int u, int i, int r, float &sum) {
        const uint4 q = hook.chunk(t);
        reinterpret_cast<uint4 *>(smem)[swizzle_chunk(i * T + g + u * NTH)] = q;
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = bf16_bits_to_f32(w[k] & 0xFFFFu), b = bf16_bits_to_f32(w[k] >> 16);
            sum = __builtin_fmaf(a, a, sum);  // a*a is exact: the fused and the unfused forms round identically
            sum = __builtin_fmaf(b, b, sum);
        }
        hook.keep(t, r, K, i * T + u * NTH, g);
    };
    // (the partial sum of group thread t_u, in the reference's order: its four chunks one after the other)
    auto stage_and_sum = [&](int u, int r) -> float {
        float sum = 0.0f;
        if (active[u]) {
            if constexpr (IN_PAIRS) {
                const uint4 *grow = reinterpret_cast<const uint4 *>(src + (size_t)r * K);
#pragma unroll
                for (int i0 = 0; i0 < 4; i0 += 2) {
                    MM_RMS_SCHED_BARRIER();      // (or the scheduler requests the next pair in front of this one's sums)
#pragma unroll
                    for (int i = 0; i < 2; ++i) stage[0][i] = hook.load(grow, r, K, (i0 + i) * T + g + u * NTH, (i0 + i) * T + u * NTH, g);
#pragma unroll
                    for (int i = 0; i < 2; ++i) stage_chunk(stage[0][i], u, i0 + i, r, sum);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) stage_chunk(stage[u][i], u, i, r, sum);
            }
        }
        return sum;
    };
    if constexpr (PREFETCH) fetch(blockIdx.x);
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        if constexpr (!PREFETCH && !IN_PAIRS) fetch(r);
        float sum[GPT];
#pragma unroll
        for (int u = 0; u < GPT; ++u) sum[u] = stage_and_sum(u, r);
        if constexpr (PREFETCH) fetch(r + gridDim.x);
        // part[t] for t < T; group threads past T write the zero padding (their sum is 0), the line after them zeroes one more slot per
        // thread.  GPT = 1: P <= 2 NTH, so that is every slot up to P, and stride <= NTH: every step of the tree is taken in full.
        // GPT = 2 with NTH < 512 (320, 384, 448 threads; P = 1024): slots 3 NTH .. 1023 are never written, and the first step of the tree
        // (stride 512) is taken by g < NTH only, so slots NTH .. 511 never receive slots 512 + NTH .. 1023.  Both are sound because
        // T <= 512 + NTH (NTH >= T / 2 and T <= 1024): every slot that is not zeroed (>= 3 NTH) or not folded (>= 512 + NTH) lies at or
        // past T -- its value in the reference's tree is the zero padding, adding it changes nothing -- and is never read: the fold reads
        // g + 512 < 512 + NTH <= 3 NTH only (NTH >= 256), and every later stride is <= 256 <= NTH.
        // (tests/test_rms_order_gpu.py: K = 16512, 20480, 24576, 28672.  The conditions argued from -- NTH >= 256, 2 NTH >= T, T <= 1024,
        // 512 + NTH >= T, 3 NTH >= 512 + NTH -- are checked for every plan of this kernel by tools/quant_plan_host_check.cpp.)
#pragma unroll
        for (int u = 0; u < GPT; ++u) part[g + u * NTH] = sum[u];
        if (g + GPT * NTH < P) part[g + GPT * NTH] = 0.0f;
        __syncthreads();
        for (int stride = P >> 1; stride >= 64; stride >>= 1) {
            if (g < stride) part[g] += part[g + stride];
            __syncthreads();
        }
        if (g < 64) {
            float s = part[g];
#pragma unroll
            for (int stride = 32; stride >= 1; stride >>= 1) s += __shfl_down(s, stride, 64);
            if (g == 0) part[0] = __fdiv_rn(1.0f, __builtin_sqrtf(__fdiv_rn(s, (float)K) + eps));
        }
        __syncthreads();
        const float rvar = part[0];
#pragma unroll
        for (int u = 0; u < GPT; ++u)
            if (active[u]) {
                const uint8_t *row = smem;
                const uint32_t byte = rms_group<INT_ROUND, false>(row, ix[u], wg[u], rvar, seg[u], j[u], r, KN, oN, image, bytesS);
                uint8_t *sf = seg[u] == 0 ? sfN : seg[u] == 1 ? sfS : sfO;
                const uint32_t b1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0x55, 0xF, 0xF, false);
                const uint32_t b2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0xAA, 0xF, 0xF, false);
                const uint32_t b3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0xFF, 0xF, 0xF, false);
                if ((g & 3) == 0)
                    store_scale_dword(sf + sf_offset(r, j[u], kseg[u]), byte | (b1 << 8) | (b2 << 16) | (b3 << 24));
            }
        __syncthreads();  // the row and part[] are rewritten by the next iteration
        // (the image is read here and rewritten only after the next iteration's first barrier; at most K bytes = 2 GPT chunks per thread)
        store_code_image<2 * GPT>(image, bytesS, KO, oS, oO, r);
    }
}

// K <= 8192: the row is staged as fp32 products x * w (see the header).  LDS: [plane A: K floats' first halves][plane B][P partial sums];
// element c = 8q + e lives at byte (e < 4 ? 0 : 2K) + 16 q' + 4(e & 3), q' = swizzle_chunk(q) (mx_group_convert.h), so chunk q's two
// halves are two conflict-free 16-byte writes.
template <bool INT_ROUND, class Stage = RowLoad>
// (167 VGPRs when this was measured, 158 with the current toolchain: six workgroups per CU either way.  Bounding it to 128 for eight -- __launch_bounds__(256, 4) -- spills 38 registers: 14.4 -> 25.9 us.)
__global__ void __launch_bounds__(256, Stage::WAVES_PER_SIMD)
rmsnorm_quantize_products_kernel(const uint16_t *__restrict__ src, const uint16_t *__restrict__ weight, float eps, int rows, int K,
                                 const int16_t *__restrict__ idx, int KN, int KS, int KO, uint8_t *__restrict__ oN,
                                 uint8_t *__restrict__ oS, uint8_t *__restrict__ oO, uint8_t *__restrict__ sfN,
                                 uint8_t *__restrict__ sfS, uint8_t *__restrict__ sfO, const Stage hook) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int T = K >> 5;
    const int g = threadIdx.x;
    const bool active = g < T;
    const uint32_t planeB = (uint32_t)K * 2;
    float *part = reinterpret_cast<float *>(smem + (size_t)K * 4);
    int P = 64;
    while (P < T) P <<= 1;
    const int bytesS = KS / 4 * 3;
    uint8_t *image = smem + (size_t)K * 4 + (size_t)(P > (int)blockDim.x ? P : (int)blockDim.x) * 4;   // [planes][partial sums][image of the S | O codes]

    uint32_t ix[16];
    const uint32_t none[16] = {};
    uint4 wch[4];
    if (active) {
        const uint4 *p = reinterpret_cast<const uint4 *>(idx + (size_t)g * 32);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 q = p[i];
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // both 16-bit column indices of the register at once (no carries between the halves: every intermediate stays below
                // 2^16): chunk q = c >> 3, swizzled (q ^ ((q >> 4) & 3)), byte = plane(c & 4) + 16 q' + 4 (c & 3)
                uint32_t q2 = (w[k] >> 3) & 0x0FFF0FFFu;                 // K <= 8192: q < 1024
                q2 ^= (q2 >> 4) & 0x00030003u;
                ix[4 * i + k] = (q2 << 4) + ((w[k] & 0x00030003u) << 2) + ((w[k] >> 2) & 0x00010001u) * planeB;   // < 4K <= 32768 each
            }
            wch[i] = reinterpret_cast<const uint4 *>(weight)[i * T + g];
        }
    }
    const int gN = KN >> 5, gS = KS >> 5;
    int seg, j, kseg;
    if (g < gN) { seg = 0; j = g; kseg = KN; }
    else if (g < gN + gS) { seg = 1; j = g - gN; kseg = KS; }
    else { seg = 2; j = g - gN - gS; kseg = KO; }

    typename Stage::Regs stage[4];
    auto fetch = [&](int r) {
        if (active && r < rows) {
            const uint4 *grow = reinterpret_cast<const uint4 *>(src + (size_t)r * K);
#pragma unroll
            for (int i = 0; i < 4; ++i) stage[i] = hook.load(grow, r, K, i * T + g, i * T, g);
        }
    };
    auto stage_and_sum = [&](int r) -> float {
        float sum = 0.0f;
        if (active) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4 sq = hook.chunk(stage[i]);
                const uint32_t x[4] = {sq.x, sq.y, sq.z, sq.w};
                const uint32_t w[4] = {wch[i].x, wch[i].y, wch[i].z, wch[i].w};
                float pr[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float a = bf16_bits_to_f32(x[k] & 0xFFFFu), b = bf16_bits_to_f32(x[k] >> 16);
                    sum = __builtin_fmaf(a, a, sum);  // a*a is exact: the fused and the unfused forms round identically
                    sum = __builtin_fmaf(b, b, sum);
                    pr[2 * k] = a * bf16_bits_to_f32(w[k] & 0xFFFFu);
                    pr[2 * k + 1] = b * bf16_bits_to_f32(w[k] >> 16);
                }
                const int q = swizzle_chunk(i * T + g);
                reinterpret_cast<float4 *>(smem)[q] = make_float4(pr[0], pr[1], pr[2], pr[3]);
                reinterpret_cast<float4 *>(smem + planeB)[q] = make_float4(pr[4], pr[5], pr[6], pr[7]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) hook.keep(stage[i], r, K, i * T, g);
        }
        return sum;
    };
    fetch(blockIdx.x);
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        const float sum = stage_and_sum(r);
        fetch(r + gridDim.x);
        part[g] = sum;              // threads T.. contribute the zero padding (P < 2 * blockDim.x)
        if (g + (int)blockDim.x < P) part[g + blockDim.x] = 0.0f;
        __syncthreads();
        // every wave walks the halving tree s[t] += s[t + stride], stride = P/2 ... 1, by itself: lane l holds s[l + 64 j]
        float rvar;
        {
            const int l = g & 63;
            float v[4] = {part[l], 0.0f, 0.0f, 0.0f};
            const int n0 = P >> 6;      // 1, 2 or 4
            if (n0 > 1) v[1] = part[l + 64];
            if (n0 > 2) { v[2] = part[l + 128]; v[3] = part[l + 192]; }
            if (n0 > 2) { v[0] += v[2]; v[1] += v[3]; }
            if (n0 > 1) v[0] += v[1];
            float s = v[0];
#pragma unroll
            for (int stride = 32; stride >= 1; stride >>= 1) s += __shfl_down(s, stride, 64);
            s = __shfl(s, 0, 64);
            rvar = __fdiv_rn(1.0f, __builtin_sqrtf(__fdiv_rn(s, (float)K) + eps));
        }
        if (active) {
            const uint8_t *row = smem;
            uint32_t byte;
            uint8_t *sf;
            byte = rms_group<INT_ROUND, true>(row, ix, none, rvar, seg, j, r, KN, oN, image, bytesS);
            sf = seg == 0 ? sfN : seg == 1 ? sfS : sfO;
            const uint32_t b1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0x55, 0xF, 0xF, false);
            const uint32_t b2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0xAA, 0xF, 0xF, false);
            const uint32_t b3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0xFF, 0xF, 0xF, false);
            if ((g & 3) == 0)
                store_scale_dword(sf + sf_offset(r, j, kseg), byte | (b1 << 8) | (b2 << 16) | (b3 << 24));
        }
        __syncthreads();  // the row and part[] are rewritten by the next iteration
        store_code_image(image, bytesS, KO, oS, oO, r);   // (read here, rewritten only after the next iteration's first barrier)
    }
}

// ---------------------------------------------------------------------------------------------------------
// K <= 8192, round 5: the rows arrive by LDS-DMA in a ring of R slots (rmsnorm_quantize_ring_kernel).
// Why: the products kernel above keeps 167 VGPRs (six workgroups of two waves per CU) and one 8 KB row in flight per workgroup:
// ~48 KB of loads in flight per CU, where reorder_quantize_kernel -- the same bytes, 0.72 of 8 TB/s -- has 13-16 workgroups' rows in
// flight.  Here a row costs no registers while it travels: `buffer_load_dwordx4 ... lds` (four 1 KB pieces per wave and row, the
// chunk swizzle of mx_group_convert.h applied on the SOURCE address) straight into slot r % R, R - 1 rows ahead, behind ONE counted
// s_waitcnt vmcnt.  The row stays bf16 (8 KB per slot at K = 4096); the norm weights of the thread's 32 columns are gathered once
// into 16 registers (as in rmsnorm_quantize_kernel); the sum of squares reads the thread's four chunks back from LDS in the
// reference's order; every wave walks the halving tree by itself.  Two barriers per row:
//   B1(r): row r has landed for every wave AND every wave is done with row r-1 (its slot is refilled right behind B1: row r+R-1);
//          the [S | O] code image of row r-1 is complete: it leaves here (store_code_image);
//   B2(r): the T partial sums are in LDS.
// vmcnt counts loads, stores and LDS-DMA together in issue order.  Per iteration a wave issues: [wait] B1, the image stores of row
// r-1 (0-2), the four DMAs of row r+R-1, B2, then the stores of row r: the scale dword (always: lane 0 of every wave owns one) and the
// fp4 codes (when the wave has a lane in the fp4 segment).  So younger than row r's own DMAs are, per ring step, at least 4 DMAs + 1
// store: vmcnt(5 (R - 2)) never lets one of row r's pieces stay in flight, and lets the rows behind it (all of them but at most one
// piece per step, when a wave issues both stores) travel on.  When the next row does not exist nothing was issued for it: vmcnt(0).
// Every wave issues exactly four DMAs per row (rows of K <= 8192 are at most 16 pieces on at most 4 waves); a piece past the row's
// end lies past the descriptor's range, fetches nothing and lands in a dump area of its own.
// The descriptor, the DMA instruction and the counted wait are make_rsrc, dma16 and wait_vmcnt<N> of mx_buffer_ops.h.
// ---------------------------------------------------------------------------------------------------------
template <bool INT_ROUND, int R>
__global__ void __launch_bounds__(256)
rmsnorm_quantize_ring_kernel(const uint16_t *__restrict__ src, const uint16_t *__restrict__ weight, float eps, int rows, int K,
                             const int16_t *__restrict__ idx, int KN, int KS, int KO, uint8_t *__restrict__ oN,
                             uint8_t *__restrict__ oS, uint8_t *__restrict__ oO, uint8_t *__restrict__ sfN,
                             uint8_t *__restrict__ sfS, uint8_t *__restrict__ sfO, int slot_bytes) {
    static_assert(R >= 3 && 5 * (R - 2) < 64, "ring depth");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];   // [R slots][1 KB dump][P floats of partial sums][image of the S | O codes]
    const int T = K >> 5;
    // The counted wait below, vmcnt(5 (R - 2)), relies on EVERY wave issuing at least one store per row (the scale dword of its lane 0),
    // i.e. on lane 0 of every wave owning a group: blockDim.x == roundup64(K / 32), as launch_rmsnorm_quantize launches it.  A launch
    // with surplus waves (DMA pieces but no stores) would let a row be read before it has landed: refuse it loudly.
    if ((int)blockDim.x != ((T + 63) & ~63)) __builtin_trap();
    const int g = threadIdx.x;
    const bool active = g < T;
    const int wave = __builtin_amdgcn_readfirstlane(g >> 6), lane = g & 63, nw = (int)blockDim.x >> 6;
    uint8_t *const dump = smem + (size_t)R * slot_bytes;
    float *part = reinterpret_cast<float *>(dump + 1024);
    int P = 64;
    while (P < T) P <<= 1;
    const int bytesS = KS / 4 * 3;
    uint8_t *image = reinterpret_cast<uint8_t *>(part) + (size_t)(P > (int)blockDim.x ? P : (int)blockDim.x) * 4;
    const unsigned lds0 = (unsigned)(unsigned long long)smem;
    const int pieces = (K + 511) >> 9;                       // 1 KB pieces of a row
    // this lane's source offset inside a piece: LDS chunk c = 64 i + p holds source chunk swizzle_chunk(c) = 64 i + swizzle_chunk(p)
    const int voff = swizzle_chunk(lane) * 16;

    // rows r0, r0 + stride, ...: DMA of the n-th of them into slot n % R
    const int stride = (int)gridDim.x;
    auto issue_row = [&](int r, int slot) {
        const rsrc_t rs = make_rsrc(src + (size_t)r * K, (unsigned)K * 2u);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int pc = wave + i * nw;                    // piece index (wave-uniform); past the row: nothing fetched, lands in the dump
            const bool real = pc < pieces;
            dma16(rs, real ? voff : 0x7FFFFF00, __builtin_amdgcn_readfirstlane(real ? pc * 1024 : 0),
                      __builtin_amdgcn_readfirstlane(real ? lds0 + (unsigned)slot * (unsigned)slot_bytes + (unsigned)pc * 1024u
                                                          : lds0 + (unsigned)R * (unsigned)slot_bytes));
        }
    };

    // ---- prologue: the thread's 32 column offsets and norm weights.  The weight vector is staged in the LAST slot (free until the
    // first refill, behind B1 of the first row) by plain loads; the first R - 1 rows are requested behind those loads ----
    uint32_t ix[16], wg[16];
    uint8_t *const wslot = smem + (size_t)(R - 1) * slot_bytes;
    // The index and weight loads are issued from inline asm (the compiler would wait for them where it first touches them -- before the
    // DMAs are even requested), the first R - 1 rows follow at once, and ONE counted wait certifies the plain loads: they are older
    // than the `dmas` LDS-DMA instructions behind them.
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    v4u wq[4] = {}, iq[4] = {};
    {
        [[maybe_unused]] const uint4 *ip = reinterpret_cast<const uint4 *>(idx + (size_t)(active ? g : 0) * 32), *wp = reinterpret_cast<const uint4 *>(weight);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            MM_DEVICE_ONLY(asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(iq[i]) : "v"(ip + i) : "memory");)
            MM_DEVICE_ONLY(asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(wq[i]) : "v"(wp + (active ? i * T + g : 0)) : "memory");)
        }
    }
    int r = (int)blockIdx.x;
    int dmas = 0;
#pragma unroll
    for (int n = 0; n < R - 1; ++n)
        if (r + n * stride < rows) { issue_row(r + n * stride, n); dmas += 4; }
    if (dmas >= 12) wait_vmcnt<12>();
    else if (dmas == 8) wait_vmcnt<8>();
    else if (dmas == 4) wait_vmcnt<4>();
    else wait_vmcnt<0>();
#pragma unroll
    for (int i = 0; i < 4; ++i) { MM_DEVICE_ONLY(asm volatile("" : "+v"(iq[i]), "+v"(wq[i]));) }     // valid from here on
    if (active) {
#pragma unroll
        for (int i = 0; i < 4; ++i) reinterpret_cast<v4u *>(wslot)[swizzle_chunk(i * T + g)] = wq[i];
    }
    __syncthreads();        // the staged weights are visible
    if (active) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t w[4] = {iq[i][0], iq[i][1], iq[i][2], iq[i][3]};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t both = swizzle_offsets((w[k] << 1) & 0xFFFEFFFEu);       // byte offsets into a staged (chunk-swizzled) [K] bf16 vector
                const uint32_t b0 = both & 0xFFFFu, b1 = both >> 16;
                ix[4 * i + k] = both;
                wg[4 * i + k] = (uint32_t)*reinterpret_cast<const uint16_t *>(wslot + b0) |
                                ((uint32_t)*reinterpret_cast<const uint16_t *>(wslot + b1) << 16);
            }
        }
    }
    const int gN = KN >> 5, gS = KS >> 5;
    int seg, j, kseg;
    if (g < gN) { seg = 0; j = g; kseg = KN; }
    else if (g < gN + gS) { seg = 1; j = g - gN; kseg = KS; }
    else { seg = 2; j = g - gN - gS; kseg = KO; }

    int slot = 0, prev = -1;
    for (int it = 0; r < rows; r += stride, ++it) {
        // row r has landed (this wave's pieces; the barrier extends it to every wave's)
        // (the first R - 1 iterations: the rows requested by the prologue have no stores between them -- only the DMAs are counted)
        if (r + (R - 2) * stride >= rows) wait_vmcnt<0>();
        else if (it < R - 1) wait_vmcnt<4 * (R - 2)>();
        else wait_vmcnt<5 * (R - 2)>();
        __syncthreads();                                                                  // B1
        if (prev >= 0) store_code_image(image, bytesS, KO, oS, oO, prev);                 // the previous row's fp6 / fp8 codes leave
        {
            const int rn = r + (R - 1) * stride;
            int sn = slot + (R - 1);
            sn = sn >= R ? sn - R : sn;
            if (rn < rows) issue_row(rn, sn);                                             // into the slot the previous row has left
        }
        const uint8_t *row = smem + (size_t)slot * slot_bytes;
        float sum = 0.0f;
        if (active) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4 q = reinterpret_cast<const uint4 *>(row)[swizzle_chunk(i * T + g)];
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float a = bf16_bits_to_f32(w[k] & 0xFFFFu), b = bf16_bits_to_f32(w[k] >> 16);
                    sum = __builtin_fmaf(a, a, sum);  // a*a is exact: the fused and the unfused forms round identically
                    sum = __builtin_fmaf(b, b, sum);
                }
            }
        }
        part[g] = sum;              // threads T.. contribute the zero padding (P < 2 * blockDim.x)
        if (g + (int)blockDim.x < P) part[g + blockDim.x] = 0.0f;
        __syncthreads();                                                                  // B2
        const float rvar = rms_tree_rvar(part, P, lane, K, eps);
        if (active) {
            const uint32_t byte = rms_group<INT_ROUND, false>(row, ix, wg, rvar, seg, j, r, KN, oN, image, bytesS);
            uint8_t *sf = seg == 0 ? sfN : seg == 1 ? sfS : sfO;
            const uint32_t b1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0x55, 0xF, 0xF, false);
            const uint32_t b2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0xAA, 0xF, 0xF, false);
            const uint32_t b3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0xFF, 0xF, 0xF, false);
            if ((g & 3) == 0)
                store_scale_dword(sf + sf_offset(r, j, kseg), byte | (b1 << 8) | (b2 << 16) | (b3 << 24));
        }
        prev = r;
        slot = slot + 1 == R ? 0 : slot + 1;
    }
    __syncthreads();
    if (prev >= 0) store_code_image(image, bytesS, KO, oS, oO, prev);
}

// ---- the host side: the plan is mx_quant_plan.h's; what follows reads the environment, picks the instantiation and launches ----
// MICROMIX_RMS_RING, read once per process: 0 never the ring kernel, 3 / 4 always with that depth (K <= 8192); unset: the plan's rule
static int rms_ring_pin() {
    static const int pin = getenv("MICROMIX_RMS_RING") ? atoi(getenv("MICROMIX_RMS_RING")) : -1;
    return pin;
}

// what every kernel of the file takes in front of its last argument (the staging hook; the ring kernels: the slot size)
struct RowArgs {
    const uint16_t *src, *weight;
    float eps;
    int rows, K;
    const int16_t *idx;
    int KN, KS, KO;
    uint8_t *oN, *oS, *oO, *sfN, *sfS, *sfO;
};
// The one launch of a planned kernel: CUs x occupancy workgroups striding over the rows, with the diagnostics events
template <auto Kern, class Last>
static hipError_t launch_rows(const quant::RmsPlan &p, const RowArgs &a, hipStream_t stream, const Last &last) {
    const int blocks = quant::resident_grid(a.rows, device_cus(), resident_per_cu<Kern>(p.threads, p.lds_bytes));
    return launch_kernel<Kern>(p.shape(blocks), stream, diag_events(), a.src, a.weight, a.eps, a.rows, a.K, a.idx, a.KN, a.KS, a.KO, a.oN, a.oS, a.oO, a.sfN,
                               a.sfS, a.sfO, last);
}
// The plans that stage the row through registers, with either hook: 256 / 512 / 512 threads, K <= 8192 / 16384 / 32768 (beyond 16384 a
// thread plays two of the reference's group threads)
template <class Stage>
static hipError_t launch_staged(const quant::RmsPlan &p, bool integer_round, const RowArgs &a, hipStream_t stream, const Stage &hook) {
    auto launch = p.kernel == quant::RMS_PRODUCTS ? (integer_round ? launch_rows<rmsnorm_quantize_products_kernel<true, Stage>, Stage>
                                                                   : launch_rows<rmsnorm_quantize_products_kernel<false, Stage>, Stage>)
                : p.kernel == quant::RMS_STAGED1 ? (integer_round ? launch_rows<rmsnorm_quantize_kernel<true, 1, Stage>, Stage>
                                                                  : launch_rows<rmsnorm_quantize_kernel<false, 1, Stage>, Stage>)
                                                 : (integer_round ? launch_rows<rmsnorm_quantize_kernel<true, 2, Stage>, Stage>
                                                                  : launch_rows<rmsnorm_quantize_kernel<false, 2, Stage>, Stage>);
    return launch(p, a, stream, hook);
}

hipError_t launch_rmsnorm_quantize(const void *src, const void *weight, float eps, int rows, int K, const int16_t *idx, int KN,
                                   int KS, int KO, bool integer_round, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN,
                                   uint8_t *sfS, uint8_t *sfO, hipStream_t stream) {
    if (rows == 0) return hipSuccess;
    const quant::RmsPlan p = quant::plan_rmsnorm_quantize(rows, K, KS, KO, false, device_cus(), rms_ring_pin());
    const RowArgs a = {(const uint16_t *)src, (const uint16_t *)weight, eps, rows, K, idx, KN, KS, KO, oN, oS, oO, sfN, sfS, sfO};
    if (const int R = quant::rms_ring_depth(p.kernel)) {
        auto launch = R == 4 ? (integer_round ? launch_rows<rmsnorm_quantize_ring_kernel<true, 4>, int> : launch_rows<rmsnorm_quantize_ring_kernel<false, 4>, int>)
                             : (integer_round ? launch_rows<rmsnorm_quantize_ring_kernel<true, 3>, int> : launch_rows<rmsnorm_quantize_ring_kernel<false, 3>, int>);
        return launch(p, a, stream, p.slot_bytes);
    }
    return launch_staged(p, integer_round, a, stream, RowLoad());
}

// mm_add_rmsnorm_quantize: the kernels that stage the row through registers, at every row count -- the LDS-DMA ring moves global memory
// straight to LDS and cannot add on the way, so the plan of a launch with the residual never names it
hipError_t launch_add_rmsnorm_quantize(const void *src, const void *res, void *s_out, const void *weight, float eps, int rows, int K,
                                       const int16_t *idx, int KN, int KS, int KO, bool integer_round, uint8_t *oN, uint8_t *oS, uint8_t *oO,
                                       uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, hipStream_t stream) {
    if (rows == 0) return hipSuccess;
    const quant::RmsPlan p = quant::plan_rmsnorm_quantize(rows, K, KS, KO, true, device_cus(), rms_ring_pin());
    const RowArgs a = {(const uint16_t *)src, (const uint16_t *)weight, eps, rows, K, idx, KN, KS, KO, oN, oS, oO, sfN, sfS, sfO};
    return launch_staged(p, integer_round, a, stream, RowAddResidual{(const uint16_t *)res, (uint16_t *)s_out});
}

}  // namespace mm
