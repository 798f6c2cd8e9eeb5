// Tiled fused three-segment MX GEMM for gfx950 -- the M > 64 path of mm_matmul: 256x256 tiles when they fill the chip, 128x256 /
// 128x128 tiles (same 8-wave body) or 64x128 / 64x64 tiles (4 compute + 4 loader waves) for launches with fewer tiles, split-K
// through a caller-provided workspace for the fewest; plan_tiles() (mx_gemm_plan.h, host-only) chooses, mm_matmul_describe() reports the choice.
// The notes below are about the 256x256 tile; mx_gemm_tile.inc documents the body and the 64-row pipeline.
//
// Arithmetic and reference citations: see mx_gemm.hip (gemm.cu:26-78, w4a4.cu, w4a6.cu, w4a8.cu, w6a6.cu,
// w8a8.cu).  Machine mapping, chosen from measurements on MI355X
// (tools/mfma_rate.py, profiles/):
//  * v_mfma_scale_f32_32x32x64_f8f6f4 sustains ~3.9 PF with the fp8 operand as srcA but only ~3.0-3.5 PF
//    with it as srcB, and fp6(A) x fp4(B) beats fp4(A) x fp6(B) the same way.  Activations are the wider
//    (or equal) format in every segment, so the ACTIVATION tile is srcA (MFMA rows = tokens) and the
//    WEIGHT tile srcB (MFMA columns = output features).
//  * a 128x128 tile needs ~47 B/clk/CU from L2 at that MFMA rate (L2 peak ~56): 256x256 halves it.
//  * 8 waves as 4 (tokens) x 2 (features), two per SIMD: each wave owns 64 x 128 outputs = 2 x 4 MFMA tiles and per
//    64-deep K step reads 2 activation + 4 weight fragments for 8 MFMAs.  (A 4-wave / one-per-SIMD variant with 128 x
//    128 per wave was measured: an LDS-DMA instruction costs the issuing wave ~180 cycles, more than the 64-cycle MFMA
//    it is meant to hide behind, so a single wave per SIMD leaves the matrix pipe idle ~45 % of the time.)
//  * the 128 fp32 accumulators of a wave live in a[0:127], driven by inline-asm MFMAs.  They are outside the
//    compiler's register allocation on purpose: with compiler-owned accumulators the three fused segment loops
//    made hipcc copy and spill them (hundreds of scratch dwords per lane, measured on ROCm 7.2).
//  * one 128-deep K slab per pipeline stage, three LDS stages (two with fp8 weights); operands AND the
//    scale-factor atoms arrive by LDS-DMA (buffer_load_dwordx4 ... lds) issued up to three slabs ahead behind
//    counted vmcnt waits, one DMA instruction between consecutive MFMAs so that their issue hides in the MFMA
//    shadow; one workgroup barrier per slab, placed between the two K steps, after the second step's
//    fragments are already in registers.
//  * with tokens on MFMA rows the accumulator has the feature index on the lane, so the epilogue transposes
//    each wave's tile through LDS (free at that point) and stores whole 256-byte rows.
#include "mx_gemm_prelude.h"
#include <string.h>

namespace mm {

#define MM_NS g256
#ifdef MM_G256_MAX_STAGES          // developer probe (tools/delivery_probes.sh): the 256-row tile's 128-deep segments on two stages
#define MM_MAX_STAGES MM_G256_MAX_STAGES
#else
#define MM_MAX_STAGES 3
#endif
#define MM_LDS_BUDGET (160 * 1024)
#define MM_WM 4
#define MM_TM 2
#define MM_TN 4
#define MM_ACC MM_ACC_CLOBBER
#include "mx_gemm_tile.inc"
#undef MM_NS
#undef MM_WM
#undef MM_TM
#undef MM_TN
#undef MM_ACC
#undef MM_MAX_STAGES
#undef MM_LDS_BUDGET
#define MM_NS g128
#define MM_MAX_STAGES 3
#define MM_LDS_BUDGET (160 * 1024)
#define MM_WM 4
#define MM_TM 1
#define MM_TN 4
#define MM_ACC MM_ACC_CLOBBER
#include "mx_gemm_tile.inc"
#undef MM_NS
#undef MM_WM
#undef MM_TM
#undef MM_TN
#undef MM_ACC
#undef MM_MAX_STAGES
#undef MM_LDS_BUDGET

// ---------------------------------------------------------------------------------------------------------
// split-K for shapes with few tiles (medium M, or small N): 128 x 256 tiles x `splits` workgroups, each on a slab range
// of one segment, raw fp32 partial sums in the caller's workspace, then a reduction kernel that adds them in split
// order (deterministic) and applies the reference's rounding chain D = bf16(N); D = bf16(S + D); D = bf16(O + D).
// ---------------------------------------------------------------------------------------------------------
static_assert(SPLIT_WG_FLOATS == g128::NACC * g128::NT, "32768 floats = 128 KiB of partial sums per workgroup (mx_gemm_plan.h)");

__global__ void __launch_bounds__(256) splitk_reduce_kernel(GemmArgs a, int tiles_n, int total) {
    // one thread = four consecutive accumulator registers of one lane of the GEMM workgroup (16 bytes of every split's partial sums,
    // the threads' pieces side by side): four consecutive tokens of one feature
    const int e = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= total) return;
    // e = (tile, register quad r4, thread tid of the GEMM workgroup, 4 registers): the layout AccLoop::store writes
    const int tid = (e >> 2) & (g128::NT - 1), r4 = (e >> 11) & (g128::NACC / 4 - 1), tile = e >> 15;
    const float *p = a.ws + (size_t)tile * a.splits * SPLIT_WG_FLOATS + (e & (SPLIT_WG_FLOATS - 1));
    float run[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int seg = 0; seg < 3; ++seg) {
        if (a.split_first[seg + 1] == a.split_first[seg]) continue;
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int q = a.split_first[seg]; q < a.split_first[seg + 1]; ++q) {
            const float4 v = *reinterpret_cast<const float4 *>(p + (size_t)q * SPLIT_WG_FLOATS);
            s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float t = s[i] + run[i];
            run[i] = a.round_per_segment ? bf16_bits_to_f32(f32_to_bf16_bits(t)) : t;
        }
    }
    // accumulator layout of the tile kernel: wave = 2 * wm + wn owns tokens wm*32.., features wn*128..; register r of
    // MFMA tile tn = r >> 4: token (r & 3) + 8 * ((r >> 2) & 3) + 4 * (lane >> 5), feature tn*32 + (lane & 31); r = 4 * r4 + i
    const int wave = tid >> 6, lane = tid & 63, wm = wave >> 1, wn = wave & 1;
    const int m = (tile / tiles_n) * g128::BM + wm * 32 + 8 * (r4 & 3) + 4 * (lane >> 5);      // + i
    const int n = (tile % tiles_n) * g128::BN + wn * 128 + (r4 >> 2) * 32 + (lane & 31);
    if (n >= a.N) return;
    if (a.out_f32) {     // MM_OUT_F32: the fp32 sums themselves
        float *d32 = reinterpret_cast<float *>(a.D) + (size_t)m * a.N + n;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (m + i < a.M) d32[(size_t)i * a.N] = run[i];
        return;
    }
    const float bias = a.bias != nullptr ? bf16_bits_to_f32(a.bias[n]) : 0.0f;
    uint16_t *dst = a.D + (size_t)m * a.N + n;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t b = f32_to_bf16_bits(run[i]);
        if (a.bias != nullptr) b = f32_to_bf16_bits(bf16_bits_to_f32(b) + bias);
        if (m + i < a.M) dst[(size_t)i * a.N] = (uint16_t)b;     // a wave's 32 lanes of one token: 64 bytes side by side
    }
}

MM_TILE_KERNELS(g256, TK_G256);
MM_TILE_KERNELS(g128, TK_G128);

// the developer overrides of the plan (mx_gemm_plan.h), read from the environment once per process
static const GemmOverrides &gemm_overrides() {
    static const GemmOverrides ov = [] {
        auto env_int = [](const char *name, int dflt) {
            const char *v = getenv(name);
            return v ? atoi(v) : dflt;
        };
        GemmOverrides o;
        o.tile = env_int("MICROMIX_GEMM_TILE", o.tile);
        o.tail = env_int("MICROMIX_GEMM_TAIL", o.tail);
        o.tile16 = env_int("MICROMIX_GEMM_TILE16", o.tile16);
        o.splitk = env_int("MICROMIX_SPLITK", o.splitk);
        o.small_m_tiles = env_int("MICROMIX_SMALL_M_TILES", o.small_m_tiles);
        o.mid_m_stream = env_int("MICROMIX_MID_M_STREAM", o.mid_m_stream);
        o.small_m_tile16 = env_int("MICROMIX_SMALL_M_TILE16", o.small_m_tile16);
        if (const char *pin = getenv("MICROMIX_SPLIT_SMALL"); pin && pin[0]) {
            o.split_small = (pin[0] == '0' && pin[1] == 0) ? 1 : 2;
            if (o.split_small == 2 && sscanf(pin, "%d:%d", &o.split_small_tile, &o.split_small_S) != 2) o.split_small_tile = 0;
        }
        return o;
    }();
    return ov;
}

// the plan for the device that is current at the call (w4: no rule depends on the weight mode today)
size_t mx_gemm_workspace_bytes(int M, int N, const int K[3], bool, bool force, bool tickets_zeroed) {
    return plan_workspace_bytes(M, N, K, force, tickets_zeroed, device_cus(), gemm_overrides());
}
bool mx_gemm_small_m_uses_tiles(int M, int N, const int K[3], bool, size_t ws_bytes, bool force_split) {
    return plan_small_m_uses_tiles(M, N, K, ws_bytes, force_split, device_cus(), gemm_overrides());
}
const char *describe_mx_gemm256(int M, int N, const int K[3], bool w4, size_t ws_bytes, bool force_split, bool tickets_zeroed, bool out_f32) {
    static thread_local char buf[224];
    return describe_tile_plan(buf, sizeof(buf), plan_tiles(M, N, K, ws_bytes, force_split, tickets_zeroed, device_cus(), gemm_overrides()), K, w4, out_f32,
                              MM_PINGPONG != 0);
}

// the 256 x 256 tile's variants (g256_variant, mx_gemm_plan.h); a launch of these never splits K
static hipError_t launch_g256(const GemmArgs &a, bool w4, int wgs, hipStream_t stream) {
    const DiagEvents ev{a.ev_start, a.ev_stop};
    switch (g256_variant(a.K, w4, a.out_f32 != 0, MM_PINGPONG != 0)) {
#if MM_PINGPONG
        case G256_PINGPONG: return launch_tile<g256::mx_gemm256_kernel<true, false, true, true>>(g256_row::dims<true>(wgs), stream, ev, a);
#endif
        case G256_TAIL: return launch_tile<g256::mx_gemm256_kernel<true, false, true>>(g256_row::dims<true>(wgs), stream, ev, a);
        default: return launch_gemm<g256_row>(w4, wgs, a, stream);
    }
}

// in-kernel split-K: equal slab ranges; a cut inside the fp4 segment moves down to an even unit (256-deep slabs stay whole lines)
// when that leaves the range before it non-empty
static void fill_small_split(GemmArgs &b, int S) {
    const int n0s = b.K[0] >> 7, total = n0s + (b.K[1] >> 7) + (b.K[2] >> 7);
    for (int q = 0; q <= S; ++q) {
        int c = (int)((long long)total * q / S);
        if (c < n0s && (c & 1) && q > 0 && q < S && c - 1 > b.split_cut[q - 1]) c -= 1;
        b.split_cut[q] = (unsigned short)c;
    }
    const int off[4] = {0, n0s, n0s + (b.K[1] >> 7), total};
    int slot = 0;
    b.slot_seg = 0;
    for (int q = 0; q < S; ++q) {
        b.split_slot[q] = (unsigned short)slot;
        for (int sg = 0; sg < 3; ++sg) {
            const int lo = b.split_cut[q] > off[sg] ? b.split_cut[q] : off[sg], hi = b.split_cut[q + 1] < off[sg + 1] ? b.split_cut[q + 1] : off[sg + 1];
            if (hi > lo) b.slot_seg |= (unsigned long long)sg << (2 * slot++);
        }
    }
    b.split_slot[S] = (unsigned short)slot;
}

hipError_t launch_mx_gemm256(const GemmArgs &a, bool w4, hipStream_t stream) {
    const TilePlan p = plan_tiles(a.M, a.N, a.K, a.ws != nullptr ? a.ws_bytes : 0, a.force_split != 0, a.tickets_zeroed != 0, device_cus(), gemm_overrides());
    GemmArgs b = a;
    b.splits = p.splits;
    if (p.kind == TK_SPLITK) {
        if (a.tickets_zeroed) b.ws = reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(a.ws) + MM_TICKET_BYTES);   // the ticket counters stay zero
        for (int i = 0; i < 4; ++i) b.split_first[i] = p.split_first[i];
    } else if (p.kind == TK_SMALL_SPLIT) {
        b.tickets = reinterpret_cast<unsigned *>(a.ws);
        b.ws = reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(a.ws) + MM_TICKET_BYTES);
        fill_small_split(b, p.splits);
    }
    for (int i = 0; i < p.launches; ++i) {
        const TileLaunch &l = p.launch[i];
        b.n_tile0 = l.n_tile0;
        b.n_tiles = l.n_tiles;
        const hipError_t e = l.tile == TK_G256   ? launch_g256(b, w4, l.wgs, stream)
                             : l.tile != TK_G128 ? launch_small_tile(l.tile, w4, p.splits != 0, l.wgs, b, stream)
                             : p.splits          ? launch_gemm<g128_row, true>(w4, l.wgs, b, stream)
                                                 : launch_gemm<g128_row>(w4, l.wgs, b, stream);
        if (e != hipSuccess) return e;
    }
    if (p.kind != TK_SPLITK) return hipSuccess;
    const int total = (int)tile_count(TK_G128, a.M, a.N) * SPLIT_WG_FLOATS;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((total / 4 + 255) / 256), dim3(256), 0, stream, b, (a.N + 255) / 256, total);
    return hipGetLastError();
}

// the fused gate / up epilogue (plan_act, mx_gemm_plan.h): fp4 weights only
bool mx_gemm_act_supported(int M, int N) { return plan_act_supported(M, N); }

const char *describe_mx_gemm_act(int M, int N) {
    static thread_local char buf[192];
    if (!plan_act_supported(M, N)) return "weight-streaming GEMM + mm::direct_quantize_kernel<0,true> (M <= 64)";
    return describe_act_plan(buf, sizeof(buf), plan_act(M, N, device_cus()));
}

hipError_t launch_mx_gemm_act(const GemmArgs &a, hipStream_t stream) {
    if (!plan_act_supported(a.M, a.N)) return hipErrorInvalidValue;
    const TilePlan p = plan_act(a.M, a.N, device_cus());
    const DiagEvents ev{a.ev_start, a.ev_stop};
    GemmArgs b = a;
    for (int i = 0; i < p.launches; ++i) {
        const TileLaunch &l = p.launch[i];
        b.n_tile0 = l.n_tile0;
        b.n_tiles = l.n_tiles;
        const hipError_t e = l.tile == TK_G256 ? launch_tile<g256::mx_gemm256_act_kernel>(g256_row::dims<true>(l.wgs), stream, ev, b)
                                               : launch_tile<g128::mx_gemm256_act_kernel>(g128_row::dims<true>(l.wgs), stream, ev, b);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// grouped launch of the tiled kernels (plan_grouped)
hipError_t launch_mx_gemm256_grouped(GroupedTileArgs &ga, bool w4, hipStream_t stream) {
    if (ga.ngroups < 1 || ga.ngroups > MM_MAX_GROUPS) return hipErrorInvalidValue;
    const int N = ga.g[0].N;
    int M[MM_MAX_GROUPS];
    for (int i = 0; i < ga.ngroups; ++i) M[i] = ga.g[i].M;
    const GroupPlan p = plan_grouped(M, ga.ngroups, N, device_cus());
    ga.first_block[0] = 0;
    for (int i = 0; i < ga.ngroups; ++i) ga.first_block[i + 1] = ga.first_block[i] + (int)tile_count(p.tile, M[i], N);
    for (int i = ga.ngroups + 1; i <= MM_MAX_GROUPS; ++i) ga.first_block[i] = ga.first_block[ga.ngroups];
    const int total = ga.first_block[ga.ngroups];
    if (p.tile == TK_G256) return launch_grouped<g256_row>(w4, total, ga, stream);
    if (p.tile == TK_G128) return launch_grouped<g128_row>(w4, total, ga, stream);
    return launch_small_tile_grouped(p.tile, w4, total, ga, stream);
}

// device-sized grouped launch of the tiled kernels (plan_moe): the grid is the host bound
hipError_t launch_mx_gemm256_moe(const GemmArgs &a, const MoeGroups &mg, bool w4, hipStream_t stream) {
    const GroupPlan p = plan_moe(mg.E, mg.n, a.N, device_cus());
    if (p.wgs > INT32_MAX) return hipErrorInvalidValue;
    if (p.tile == TK_G256) return launch_moe<g256_row>(w4, (int)p.wgs, a, mg, stream);
    if (p.tile == TK_G128) return launch_moe<g128_row>(w4, (int)p.wgs, a, mg, stream);
    return launch_small_tile_moe(p.tile, w4, (int)p.wgs, a, mg, stream);
}

// device-sized grouped launch with the fused gate / up epilogue (mm_moe_gate_up_activate): 256-feature tiles only, every expert of
// 1 .. max_rows rows in ONE grid.  The grid is the host bound of plan_moe on the experts' row tiles; 128-row tiles while that bound
// fits one round of workgroups (the round rule on the 256-feature tiles), 256-row tiles otherwise; no tail balancing, no split-K.
const char *describe_mx_gemm256_moe_act(int E, int n, int N) {
    static thread_local char buf[160];
    return describe_moe_act_plan(buf, sizeof(buf), plan_moe(E, n, N, device_cus(), true));
}

hipError_t launch_mx_gemm256_moe_act(const GemmArgs &a, const MoeGroups &mg, hipStream_t stream) {
    if (a.N <= 0 || (a.N % 256) || mg.E < 1 || mg.n < 1) return hipErrorInvalidValue;
    const GroupPlan p = plan_moe(mg.E, mg.n, a.N, device_cus(), true);
    if (p.wgs > INT32_MAX) return hipErrorInvalidValue;
    return p.tile == TK_G128 ? launch_tile<g128::mx_gemm256_moe_act_kernel>(g128_row::dims<true>((int)p.wgs), stream, DiagEvents{}, a, mg)
                             : launch_tile<g256::mx_gemm256_moe_act_kernel>(g256_row::dims<true>((int)p.wgs), stream, DiagEvents{}, a, mg);
}

}  // namespace mm
