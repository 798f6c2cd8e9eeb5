// Host side of the weight-streaming kernels (mx_gemm_stream.hip, every launch with M <= 64): which (F, T16, D, NW) a launch runs on, with
// what grid and how much LDS, and whether a shape is supported at all.  Plain C++ without a HIP include, in the manner of
// mx_gemm_plan.h: everything takes the CU count and the developer overrides as arguments (tools/stream_plan_host_check.cpp checks the
// invariants over CU counts from 1 to 1024, tests/test_stream_dispatch_cpu.py replays a sweep recorded before this header existed).
// The size functions are the kernel's own -- Ring<> and stream_body take them from here -- and the launchers read the plan: the LDS
// formula, the configuration ladder and every budget of a *_supported predicate are written once, below.
#pragma once
#include <stddef.h>

#include <initializer_list>

#include "mx_decode_quant_sizes.h"   // dq::operand_bytes, rms_bytes, early_fits: the LDS range of the quantization in front of the rings
#include "mx_launch_shape.h"

namespace mm {

namespace stream {

constexpr int MAX_GROUPS = 8;                   // = MM_MAX_GROUPS (mx_kernels.h; static_asserted in mx_gemm_stream.hip)
constexpr int STREAM_LDS_MAX = 160 * 1024;      // (the 64-token configuration on 16 features uses all of a CU's LDS)
// the quantizing launches: a CU's LDS (two workgroups share it where they can) and what one workgroup may take of it
constexpr size_t QUANT_LDS_CU = 160 * 1024, QUANT_LDS_WG = 156 * 1024;
constexpr int ACT_GROUP_BYTES = 16 * 32 * 4;    // ACT: the 32 values of a group for up to 16 tokens, behind the reduction image

// one workgroup = 16 F output features x T16 token tiles of 16, NW waves with a private ring of D slots each (see mx_gemm_stream.hip)
struct StreamCfg {
    int F, T16, D, NW;
    constexpr bool operator==(const StreamCfg &o) const { return F == o.F && T16 == o.T16 && D == o.D && NW == o.NW; }
};

// ---- sizes that host and kernel share ----
// launches without the quantization that take their scales from scale images (see stream_body): one token tile, and two with fp4 weights
constexpr bool scale_images_for(int T16, bool W4) { return T16 == 1 || (T16 == 2 && W4); }
// a wave's scale image of a tensor with 16 F rows per slab (see stream_body, "the scale image")
constexpr int scale_image_wave_bytes(int F, int NW, int T) {      // T = 128-deep slabs of the launch
    const int spi = 4 / F, per_wave = (T + NW - 1) / NW;
    return (per_wave + spi - 1) / spi * 256;
}
constexpr int scale_image_bytes(int F, int NW, int T) { return NW * scale_image_wave_bytes(F, NW, T); }
// both images of a launch without the quantization (weights' rows 16 F, activations' 16 T16): one token tile only, see stream_body
constexpr int scale_images_bytes(int F, int T16, int NW, int T, bool W4) {
    return scale_images_for(T16, W4) ? scale_image_bytes(F, NW, T) + scale_image_bytes(T16, NW, T) : 0;
}
// one slot of a wave's ring (Ring<>): F weight tiles (one 1 KB piece each with fp4 weights, two otherwise), T16 activation tiles of two
// pieces unless the workgroup quantizes the rows itself
constexpr int ring_weight_bytes(int F, bool W4) { return F * (W4 ? 1 : 2) * 1024; }
constexpr int ring_slot_bytes(int F, int T16, bool W4, bool QUANT) { return ring_weight_bytes(F, W4) + (QUANT ? 0 : T16 * 2048); }
constexpr int ring_bytes(const StreamCfg &c, bool W4, bool QUANT) { return c.NW * c.D * ring_slot_bytes(c.F, c.T16, W4, QUANT); }
// the reduction image over the rings: every wave's partial sums of the present segments side by side; with eight or more 16 x 16 tiles
// per wave one segment at a time through one image (stream_body, SEQ)
constexpr int red_image_bytes(const StreamCfg &c, int present) { return c.NW * (c.F * c.T16 >= 8 ? 1 : present) * c.F * c.T16 * 4 * 64 * 4; }
constexpr int present_segments(const int K[3]) { return (K[0] ? 1 : 0) + (K[1] ? 1 : 0) + (K[2] ? 1 : 0); }
constexpr int slabs_of(const int K[3]) { return (K[0] + K[1] + K[2]) >> 7; }
constexpr int max_of(int a, int b) { return a > b ? a : b; }

// ---- the LDS of a workgroup, once per family ----
// plain / grouped / device-sized: [rings | scale images] while the slabs stream, then the reduction image over both
constexpr int stage_bytes(const StreamCfg &c, bool W4, int T) { return ring_bytes(c, W4, false) + scale_images_bytes(c.F, c.T16, c.NW, T, W4); }
constexpr int gemm_lds_bytes(const StreamCfg &c, bool W4, const int K[3]) {
    return max_of(red_image_bytes(c, present_segments(K)), stage_bytes(c, W4, slabs_of(K)));
}
// the fused gate | up launch on quantized rows (ACT, fp4 weights): the same, and one token tile keeps the fp6 group buffer behind the
// reduction image (two token tiles reduce one segment at a time through one image; the group buffer lies inside it)
constexpr int act_lds_bytes(const StreamCfg &c, const int K[3]) {
    return max_of(red_image_bytes(c, present_segments(K)) + (c.T16 == 1 ? ACT_GROUP_BYTES : 0), stage_bytes(c, true, slabs_of(K)));
}
// the quantizing launches, behind the quantization's own range: [rings | weights' scale image], then the reduction image over both
// (ACT: the group buffer lies in the staged rows' range)
constexpr size_t quant_tail_bytes(const StreamCfg &c, bool W4, const int K[3]) {
    return (size_t)max_of(red_image_bytes(c, present_segments(K)), ring_bytes(c, W4, true) + scale_image_bytes(c.F, c.NW, slabs_of(K)));
}
constexpr size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }
// ... and that range without the staged rows: the quantized operands and, with the norm, its weights and partial sums
constexpr size_t quant_operand_bytes(int M, const int K[3], bool norm) { return round16(dq::operand_bytes(M, K)) + (norm ? round16(dq::rms_bytes(M, K)) : 0); }
// slots per thread of dq::quantize_rows_early (see there): 2 on the four-wave kernels, whose register count costs no resident workgroup
constexpr int early_npass(int NW) { return NW <= 4 ? 2 : 1; }

// The developer overrides, read from the environment once per process (stream_overrides(), mx_gemm_stream.hip); the defaults are "unset".
struct StreamOverrides {
    int stream = 1;                // MICROMIX_STREAM=0: mm_matmul never streams
    int grouped = 1;               // MICROMIX_STREAM_GROUPED=0: nor do the grouped and device-sized launches
    int grouped_max_m = 64;        // MICROMIX_STREAM_GROUPED_MAX_M: ... above this many rows in the largest group
    int decode_stream = 1;         // MICROMIX_DECODE_STREAM: 0 off, 2 every shape that fits (A/B runs)
    int decode_early = 1;          // MICROMIX_DECODE_EARLY=0: never the early quantization phase
    int decode_f4 = 0;             // MICROMIX_DECODE_F4: 64 features x 4 waves with this many slots (2, 3, 4; -1: never)
    int decode_depth = 2;          // MICROMIX_DECODE_DEPTH: ring slots of the 32-feature decode launch (2, 3, 4)
    int gate_up_act_stream = 1;    // MICROMIX_GATE_UP_ACT_STREAM=0: the fused gate | up launch never streams
    int cfg_f = 0, cfg_d = 0, cfg_nw = 0;   // MICROMIX_STREAM_CFG="F,D,NW" (-DMM_STREAM_SWEEP=1 builds only): pins the plain launch
};

// ---- the kernels that exist: one closed list per launch kind (the dispatch in mx_gemm_stream.hip instantiates exactly these) ----
enum StreamKind { SK_PLAIN, SK_GROUPED, SK_MOE, SK_ACT, SK_QUANT, SK_QUANT_ACT };
struct CfgRow { StreamCfg cfg; bool w4; };
#define MM_BOTH(...) {{__VA_ARGS__}, true}, {{__VA_ARGS__}, false}
// (17 .. 32 tokens, see select_gemm: the fp4 rows take their scales from images; (2, 2, 3, 4) with fp4 weights is no longer chosen)
#define MM_STREAM_ABOVE_16 {{2, 2, 2, 4}, true}, {{1, 2, 3, 8}, true}, {{1, 2, 2, 8}, true}, MM_BOTH(2, 2, 3, 4), {{1, 2, 3, 8}, false}, \
                           MM_BOTH(2, 3, 2, 4), MM_BOTH(1, 3, 2, 8), MM_BOTH(2, 4, 2, 4), MM_BOTH(1, 4, 2, 8)
constexpr CfgRow GROUPED_CFGS[] = {MM_BOTH(2, 1, 2, 8), MM_BOTH(1, 1, 3, 8), MM_STREAM_ABOVE_16};      // grouped and device-sized
constexpr CfgRow PLAIN_CFGS[] = {MM_BOTH(4, 1, 2, 4), MM_BOTH(2, 1, 2, 8), MM_BOTH(1, 1, 4, 8), MM_BOTH(1, 1, 3, 8), MM_STREAM_ABOVE_16,
#if defined(MM_STREAM_SWEEP) && MM_STREAM_SWEEP      // kernel-developer build: every (F, D, NW) combination that MICROMIX_STREAM_CFG may name, at 1 / 2 / 4 token tiles
#define MM_TRY(F, D, NW) MM_BOTH(F, 1, D, NW), MM_BOTH(F, 2, D, NW), MM_BOTH(F, 4, D, NW)
                                   MM_BOTH(4, 2, 2, 4), MM_BOTH(4, 4, 2, 4), MM_BOTH(4, 1, 2, 8), MM_BOTH(4, 2, 2, 8), MM_BOTH(4, 1, 3, 4), MM_BOTH(4, 2, 3, 4),
                                   MM_TRY(1, 4, 4), MM_TRY(1, 6, 4), MM_TRY(1, 4, 8), MM_TRY(1, 2, 8), MM_TRY(1, 3, 8), MM_TRY(1, 2, 16), MM_TRY(2, 3, 4),
                                   MM_TRY(2, 4, 4), MM_TRY(2, 4, 8), MM_TRY(2, 3, 8), MM_TRY(2, 2, 8), MM_TRY(2, 2, 16), MM_TRY(2, 1, 16),
#undef MM_TRY
#endif
};
#undef MM_STREAM_ABOVE_16
constexpr CfgRow ACT_CFGS[] = {{{4, 1, 2, 4}, true}, {{4, 2, 2, 4}, true}};      // the fused gate | up launch on quantized rows: fp4 weights
// the quantizing launches (one token tile).  Only the configurations the default selection uses have kernels with the norm (and the
// residual add) inside: NORM_CFGS.  The ACT form (SK_QUANT_ACT) is (4, 1, 2, 4) with fp4 weights alone, with and without the norm.
constexpr CfgRow QUANT_CFGS[] = {MM_BOTH(4, 1, 2, 4), MM_BOTH(4, 1, 3, 4), MM_BOTH(4, 1, 4, 4), MM_BOTH(2, 1, 3, 8),
                                 MM_BOTH(2, 1, 4, 8), MM_BOTH(2, 1, 2, 8), MM_BOTH(1, 1, 4, 8), MM_BOTH(1, 1, 3, 8)};
constexpr CfgRow QUANT_ACT_CFGS[] = {{{4, 1, 2, 4}, true}};
constexpr StreamCfg NORM_CFGS[] = {{4, 1, 2, 4}, {2, 1, 2, 8}, {1, 1, 3, 8}, {1, 1, 4, 8}};
#undef MM_BOTH
struct CfgList { const CfgRow *rows; size_t n; };
#define MM_LIST(a) CfgList{a, sizeof(a) / sizeof(a[0])}
constexpr CfgList cfg_list(StreamKind kind) {
    return kind == SK_PLAIN ? MM_LIST(PLAIN_CFGS) : kind == SK_ACT ? MM_LIST(ACT_CFGS) : kind == SK_QUANT ? MM_LIST(QUANT_CFGS)
         : kind == SK_QUANT_ACT ? MM_LIST(QUANT_ACT_CFGS) : MM_LIST(GROUPED_CFGS);
}
#undef MM_LIST
constexpr bool in_list(StreamKind kind, const StreamCfg &c, bool w4) {
    const CfgList list = cfg_list(kind);
    for (size_t i = 0; i < list.n; ++i)
        if (list.rows[i].cfg == c && list.rows[i].w4 == w4) return true;
    return false;
}
constexpr bool has_norm_kernel(const StreamCfg &c) {
    for (const StreamCfg &n : NORM_CFGS)
        if (n == c) return true;
    return false;
}

// what a launcher needs: the grid, the workgroup, the dynamic LDS and the limit to raise the kernel's to (0: the default 64 KB holds)
using StreamLaunch = LaunchShape;      // {grid_x, grid_y, threads, lds_bytes, raise_to}
struct GemmPlan { bool ok; StreamCfg cfg; StreamLaunch launch; };
struct QuantPlan {
    bool ok;
    StreamCfg cfg;
    bool rms, add, act;            // the kernel variant: norm inside, residual add in front of it, activation behind the reduction
    StreamLaunch launch;
    int stage_rows, early, qbytes; // QuantIn::stage_rows / early; the quantization's LDS range in front of the rings
};

// 16 features x two token tiles x 8 waves with fp4 weights and `depth` slots: rings of 1 + 4 KB slots and both images fit
constexpr bool two_tile_fits(int depth, int T) { return stage_bytes(StreamCfg{1, 2, depth, 8}, true, T) <= STREAM_LDS_MAX; }

// ---- the ladder: (F, T16, D, NW) of a plain / grouped / device-sized launch ----
// M: the rows (the largest group's; device-sized: min(max_rows, 64)); `groups`: the problems whose workgroups share the CUs (1 for a
// plain launch; device-sized: as the grouped launch counts them at its fullest, min(E, n, MAX_GROUPS)).
// (slots, waves) from sweeps on three boxes (profiles/r04_stream_ablation.txt, section 7): more waves with a shallow ring beat fewer
// with a deep one.  F, T16 and D leave every output bit alone; NW does not once a launch has more than four slabs (K > 512): slab j is
// summed in wave j % NW and the waves in wave order.
// How the launch's 32-feature workgroups compare with the CUs: fewer, at least one each, more than two each.
enum Rounds { R_PARTIAL, R_FULL, R_OVER_TWO };
constexpr Rounds rounds_of(int N, int groups, int cus) {
    const int wgs32 = (N + 31) / 32 * groups;
    return wgs32 > 2 * cus ? R_OVER_TWO : (wgs32 >= cus ? R_FULL : R_PARTIAL);
}
inline StreamCfg ladder(StreamKind kind, int M, int slabs, bool w4, Rounds rounds) {
    // 32 features per workgroup once those fill the CUs, 16 below (q/o at N = 4096: 256 workgroups instead of 128)
    const bool wide = rounds != R_PARTIAL;
    if (M <= 16) {
        // PLAIN ONLY, more than one round of 32-feature workgroups (fused gate + up, N = 28672): 64 features x 4 waves run in one
        // round -- the same time with resident weights, 1 us less at M = 16 when they come from HBM (18.2 -> 17.1; section 19 of the
        // record).  Never measured on a grouped launch.
        if (kind == SK_PLAIN && rounds == R_OVER_TWO) return StreamCfg{4, 1, 2, 4};
        if (wide) return StreamCfg{2, 1, 2, 8};
        // PLAIN ONLY, few features: four slots when a wave's slabs are at most four -- K <= 4096: everything is requested at once, no
        // phantom steps.  (The grouped predicate budgets four slots all the same: stream_images_fit.)
        if (kind == SK_PLAIN && slabs <= 32) return StreamCfg{1, 1, 4, 8};
        return StreamCfg{1, 1, 3, 8};
    }
    // 17 .. 32 tokens.  fp4 weights take their scales from images (round 6): on 32 features two slots instead of three keep the second
    // workgroup's place in the LDS (gate/up 10.1-10.8 -> 9.4-9.8 us), and four waves, so that two workgroups fit a CU's LDS; on 16
    // features (one workgroup per CU) three slots while rings and images fit, else two (down_proj 12.0 -> 11.1)
    if (M <= 32 && w4) return wide ? StreamCfg{2, 2, 2, 4} : (two_tile_fits(3, slabs) ? StreamCfg{1, 2, 3, 8} : StreamCfg{1, 2, 2, 8});
    if (M <= 32) return wide ? StreamCfg{2, 2, 3, 4} : StreamCfg{1, 2, 3, 8};
    // 33 .. 64 tokens: three / four token tiles; two slots of 8 / 10 KB and four waves, so that two workgroups fit a CU's LDS
    if (M <= 48) return wide ? StreamCfg{2, 3, 2, 4} : StreamCfg{1, 3, 2, 8};
    return wide ? StreamCfg{2, 4, 2, 4} : StreamCfg{1, 4, 2, 8};
}
inline StreamCfg select_gemm(StreamKind kind, int M, int N, const int K[3], bool w4, int groups, int cus, const StreamOverrides &ov) {
    if (kind == SK_PLAIN && ov.cfg_f) return StreamCfg{ov.cfg_f, M <= 16 ? 1 : (M <= 32 ? 2 : 4), ov.cfg_d, ov.cfg_nw};   // (MM_STREAM_SWEEP builds)
    return ladder(kind, M, slabs_of(K), w4, rounds_of(N, groups, cus));
}
constexpr int moe_rows(int max_rows) { return max_rows < 64 ? max_rows : 64; }
constexpr int moe_groups(int E, int n) { return (E < n ? E : n) < MAX_GROUPS ? (E < n ? E : n) : MAX_GROUPS; }

constexpr StreamLaunch stream_launch(int N, int F, int grid_y, int NW, size_t lds, size_t limit) {
    return StreamLaunch{(N + 16 * F - 1) / (16 * F), grid_y, 64 * NW, (int)lds, lds > 65536 ? (int)limit : 0};
}
// the plan of a plain (grid_y = 1) / grouped (the groups) / device-sized (the experts) launch; !ok: the launcher returns hipErrorInvalidValue
inline GemmPlan plan_gemm(StreamKind kind, int M, int N, const int K[3], bool w4, int groups, int grid_y, int cus, const StreamOverrides &ov) {
    const StreamCfg c = select_gemm(kind, M, N, K, w4, groups, cus, ov);
    if (!in_list(kind, c, w4)) return GemmPlan{false, c, {}};
    const int lds = gemm_lds_bytes(c, w4, K);
    return GemmPlan{lds <= STREAM_LDS_MAX, c, stream_launch(N, c.F, grid_y, c.NW, lds, STREAM_LDS_MAX)};      // (the *_supported predicates keep callers away from !ok)
}
// ... as the exported launchers ask for it: mm_matmul; the grouped launch, whose groups' workgroups all count towards filling the CUs; the
// device-sized launch, with the tier from max_rows and the groups counted as the grouped launch counts them at its fullest
inline GemmPlan plan_plain(int M, int N, const int K[3], bool w4, int cus, const StreamOverrides &ov) { return plan_gemm(SK_PLAIN, M, N, K, w4, 1, 1, cus, ov); }
inline GemmPlan plan_grouped(int max_m, int ngroups, int N, const int K[3], bool w4, int cus, const StreamOverrides &ov) {
    return plan_gemm(SK_GROUPED, max_m, N, K, w4, ngroups, ngroups, cus, ov);
}
inline GemmPlan plan_moe(int max_rows, int E, int rows, int N, const int K[3], bool w4, int cus, const StreamOverrides &ov) {
    return plan_gemm(SK_MOE, moe_rows(max_rows), N, K, w4, moe_groups(E, rows), E, cus, ov);
}
// the fused gate | up launch on quantized rows: 64-row workgroups (32 gate + 32 up), N a multiple of 256, M <= 32 (the predicate's)
inline GemmPlan plan_gate_up_act(int M, int N, const int K[3]) {
    const StreamCfg c = {4, M <= 16 ? 1 : 2, 2, 4};
    const int lds = act_lds_bytes(c, K);
    return GemmPlan{lds <= STREAM_LDS_MAX, c, StreamLaunch{N / 64, 1, 256, lds, lds > 65536 ? STREAM_LDS_MAX : 0}};
}

// ---- the quantizing launches (M <= 8: the workgroup quantizes the bf16 rows itself) ----
enum QuantKind { QK_QLINEAR, QK_DOWN_ACTIVATE, QK_GATE_UP_ACT };   // mm_*qlinear_decode; mm_down_activate_decode (QuantIn::mode 1); the ACT form
inline StreamCfg select_quant(QuantKind what, int N, const int K[3], bool norm, int cus, const StreamOverrides &ov) {
    if (what == QK_GATE_UP_ACT) return StreamCfg{4, 1, 2, 4};      // 64 rows (32 gate + 32 up) x 4 waves
    const int wgs32 = (N + 31) / 32;
    const bool wide = wgs32 >= cus;
    if (what == QK_DOWN_ACTIVATE) {
        // (A deeper ring does nothing here -- seven or fourteen slots, a wave's whole share of K = 14336 in flight at once, measured the
        // same 10.6 us as three, round 6, and with the weights coming from HBM 11.6 against 11.5: the launch is the sum of its
        // vector-memory instructions, not a chain of round trips.  The scale image is what took 1.6 us off it.)
        return wide ? StreamCfg{2, 1, 2, 8} : StreamCfg{1, 1, 3, 8};
    }
    // kernel-developer overrides: 64 features x 4 waves with this many slots (-1: never) / ring slots (2, 3, 4).  Ignored with the norm
    // inside the launch: only NORM_CFGS have norm variants (an override made a supported shape fail at launch)
    const int qf4 = norm ? 0 : ov.decode_f4, qd = norm ? 2 : ov.decode_depth;
    if (wide && qf4 >= 2 && qf4 <= 4) return StreamCfg{4, 1, qf4, 4};
    // more than one round of 32-feature workgroups (two per CU): 64 features x 4 waves halve the workgroups that repeat the quantization
    // and run in one round (fused gate + up, N = 28672, M = 1: 17.3 -> 14.2 us, from HBM 18.7 -> 16.1; at N = 14336 it loses 1 us from HBM)
    if (wide && qf4 == 0 && wgs32 > 2 * cus) return StreamCfg{4, 1, 2, 4};
    if (wide) return StreamCfg{2, 1, qd == 3 || qd == 4 ? qd : 2, 8};
    return slabs_of(K) <= 32 ? StreamCfg{1, 1, 4, 8} : StreamCfg{1, 1, 3, 8};
}
// the plan of configuration c: `norm` / `add`: the RMSNorm (and the residual add in front of it) runs inside the launch
inline QuantPlan plan_quant(QuantKind what, const StreamCfg &c, bool w4, int M, int N, const int K[3], bool norm, bool add, const StreamOverrides &ov) {
    const bool act = what == QK_GATE_UP_ACT, mode1 = what == QK_DOWN_ACTIVATE;
    QuantPlan p = {false, c, norm, add, act, {}, 0, 0, 0};
    if (!in_list(act ? SK_QUANT_ACT : SK_QUANT, c, w4) || (norm && !has_norm_kernel(c)) || (add && !norm)) return p;     // (a kernel-developer override picked a configuration without that variant)
    const size_t Kt = (size_t)K[0] + K[1] + K[2], tail = quant_tail_bytes(c, w4, K), ops = quant_operand_bytes(M, K, norm);
    // staged bf16 rows: all M if two workgroups still fit a CU's LDS, else as many as one workgroup can hold (at least one)
    size_t rows = mode1 ? 0 : M;       // (mode 1 quantizes straight from global memory: nothing is staged)
    if (!mode1 && 2 * (ops + tail + rows * Kt * 2) > QUANT_LDS_CU) {
        const size_t two = QUANT_LDS_CU / 2 > ops + tail ? (QUANT_LDS_CU / 2 - ops - tail) / (Kt * 2) : 0;
        const size_t one = QUANT_LDS_WG > ops + tail ? (QUANT_LDS_WG - ops - tail) / (Kt * 2) : 0;
        rows = two >= 1 ? two : one;
        if (rows > (size_t)M) rows = M;
    }
    if (rows < 1 && !mode1) return p;
    p.stage_rows = (int)rows;
    p.early = (!mode1 && rows >= (size_t)M && dq::early_fits(M, (int)Kt, 64 * c.NW, early_npass(c.NW))) ? 1 : 0;
    if (mode1) p.early = (size_t)M * (Kt / 32) <= 64u * c.NW ? 1 : 0;      // activate_rows_early: one pass of the workgroup's threads
    if (!ov.decode_early) p.early = 0;
    const size_t qbytes = rows * Kt * 2 + ops, lds = qbytes + tail;
    p.qbytes = (int)qbytes;
    p.launch = stream_launch(N, c.F, 1, c.NW, lds, QUANT_LDS_WG);
    p.ok = lds <= QUANT_LDS_WG;      // (every mode: the supported() predicates keep callers away from this)
    return p;
}

// ---- the *_supported predicates ----
// A predicate that says yes promises that the launch will not be refused: beside its own budget it asks the plan.  (Before the plan
// existed the budgets below were all there was, and three kinds of shape passed them and failed at launch: M <= 16 with K above 43000
// on the 32- and 64-feature configurations, whose scale images are larger than the 16-feature configuration's that is budgeted; and
// mm_qlinear_decode with MICROMIX_DECODE_F4 / _DEPTH pinning deeper rings than the budget's.)
// Launches of one or two (fp4) token tiles keep scale images behind their rings: the stage of the 16-feature configuration -- the
// largest of the tier -- must fit a workgroup's LDS.  One tile: the rings of (1, 1, 4 | 3, 8), four slots up to 32 slabs as the plain
// ladder has them, whatever the launch kind; two tiles with fp4 weights: (1, 2, 2, 8), what the ladder falls back to.  The
// 32- and 64-feature configurations of the same tier stage less.
inline bool stream_images_fit(int M, const int K[3], bool w4) {
    if (M > 32 || (M > 16 && !w4)) return true;
    const int T = slabs_of(K);
    if (M > 16) return two_tile_fits(2, T);
    return stage_bytes(StreamCfg{1, 1, T <= 32 ? 4 : 3, 8}, w4, T) <= STREAM_LDS_MAX;
}
// every width of M's tier fits a workgroup's LDS -- any K a model has: the answer then needs no CU count
inline bool every_width_fits(StreamKind kind, int M, const int K[3], bool w4) {
    for (Rounds r : {R_PARTIAL, R_FULL, R_OVER_TWO})
        if (gemm_lds_bytes(ladder(kind, M, slabs_of(K), w4, r), w4, K) > STREAM_LDS_MAX) return false;
    return true;
}
// `cus()`: the CU count, asked for only where the answer depends on it (for the caller it is a runtime call in front of a launch)
template <class Cus>
inline bool gemm_supported(int M, int N, const int K[3], bool w4, Cus &&cus, const StreamOverrides &ov) {
    if (!ov.stream || M > 64) return false;
    // few features, short K, a handful of tokens (q/k/v/o at M <= 8): the launch is all start-up, and the first kernel's is shorter
    // (q/o at M = 1: 4.65 against 5.0-5.5 us; from M = 16 on the two meet)
    if (M <= 8 && K[0] + K[1] + K[2] <= 8192 && (N + 15) / 16 <= cus()) return false;
    if (!stream_images_fit(M, K, w4)) return false;
    // (a configuration pinned in an MM_STREAM_SWEEP build is launched or refused, never replaced by the first kernel)
    return ov.cfg_f != 0 || every_width_fits(SK_PLAIN, M, K, w4) || plan_plain(M, N, K, w4, cus(), ov).ok;
}
// the grouped launch: every group M <= 64 (one to four token tiles); either weight mode
inline bool grouped_tier_supported(int max_m, int ngroups, const int K[3], const StreamOverrides &ov) {
    return ov.grouped && max_m >= 1 && max_m <= ov.grouped_max_m && max_m <= 64 && ngroups >= 1 && ngroups <= MAX_GROUPS &&
           stream_images_fit(max_m, K, false) && stream_images_fit(max_m, K, true);
}
template <class Cus>
inline bool grouped_supported(int max_m, int ngroups, int N, const int K[3], Cus &&cus, const StreamOverrides &ov) {
    if (!grouped_tier_supported(max_m, ngroups, K, ov)) return false;
    if (every_width_fits(SK_GROUPED, max_m, K, false) && every_width_fits(SK_GROUPED, max_m, K, true)) return true;
    return plan_grouped(max_m, ngroups, N, K, false, cus(), ov).ok && plan_grouped(max_m, ngroups, N, K, true, cus(), ov).ok;
}
// the device-sized grouped launch: supported where the host-sized path streams whatever its largest group of at most max_m rows is --
// every tier up to max_m's must fit (a very long K fits the 64-row tier and not the 16-row one), so that no group is on the skinny
// kernel there and streamed here.  The query knows neither N nor the experts: both widths of the tier must fit.
inline bool moe_tier_supported(int tier, const int K[3], const StreamOverrides &ov) {
    return grouped_tier_supported(tier, 1, K, ov) && every_width_fits(SK_MOE, tier, K, false) && every_width_fits(SK_MOE, tier, K, true);
}
inline bool moe_supported(int max_m, const int K[3], const StreamOverrides &ov) {
    max_m = moe_rows(max_m);
    for (int tier = 16; tier < max_m; tier += 16)
        if (!moe_tier_supported(tier, K, ov)) return false;
    return moe_tier_supported(max_m, K, ov);
}

// LDS that the ring / reduction tail of the quantizing launches may need beside the quantization's own range.  stream_tail_budget: the
// largest quant_tail_bytes without the scale image over the configurations the default selection uses -- three segments' reduction
// image of (4, 1, 2, 4) or (2, 1, 2, 8), 48 KB, and with matching-precision weights their rings, 64 KB.  The predicates budget this
// worst case so that a shape they accept always launches (they budgeted 48 KB whatever the weight mode).
constexpr size_t stream_tail_budget(bool w4) {
    return (size_t)max_of(red_image_bytes(StreamCfg{4, 1, 2, 4}, 3), ring_bytes(StreamCfg{2, 1, 2, 8}, w4, true));
}
// ... with the scale image of the default (F, NW) for N output features behind the largest default rings (32 KB with fp4 weights, 64 KB
// without): under the reduction image where that is the larger one
inline size_t quant_tail_budget(int N, size_t Kt, bool w4, int cus) {
    const int T = (int)(Kt >> 7), wgs32 = (N + 31) / 32;
    const size_t simg = wgs32 > 2 * cus ? scale_image_bytes(4, 4, T) : (wgs32 >= cus ? scale_image_bytes(2, 8, T) : scale_image_bytes(1, 8, T));
    const size_t rings = (size_t)ring_bytes(StreamCfg{2, 1, 2, 8}, w4, true) + simg;
    return rings > stream_tail_budget(w4) ? rings : stream_tail_budget(w4);
}
// mm_qlinear_decode on the streaming kernel: the quantized rows, one staged row and the rings fit a workgroup's LDS.
// Measured against the first fused kernel (qlinear_decode.hip; tools/time_decode.py, profiles/r04_stream_ablation.txt section 8):
// it wins where N / 32 fills the CUs and one pass quantizes the rows (gate/up at M = 1 / 2 / 4: 12.5 / 11.8 / 14.3 -> 10.2 / 9.2 /
// 12.3 us) and loses on q/k/v/o (few workgroups: all start-up) and at M = 8 (two passes per workgroup: quantize + GEMM wins there).
inline bool qlinear_supported(int M, int N, const int K[3], bool rms, bool w4, int cus, const StreamOverrides &ov) {
    const size_t Kt = (size_t)K[0] + K[1] + K[2];
    const size_t norm = rms ? dq::rms_bytes(M, K) : 0;
    if (rms && Kt > (size_t)dq::RMS_MAX_K) return false;
    const size_t need = dq::operand_bytes(M, K) + norm + Kt * 2 + quant_tail_budget(N, Kt, w4, cus) + 64;
    if (!(ov.decode_stream == 2 && M >= 1 && M <= 8)) {     // (2, A/B runs: every shape that fits)
        if (!ov.decode_stream || M < 1 || M > 4 || (N + 31) / 32 < cus) return false;
    }
    return need <= QUANT_LDS_WG && plan_quant(QK_QLINEAR, select_quant(QK_QLINEAR, N, K, rms, cus, ov), w4, M, N, K, rms, false, ov).ok;
}
// mm_down_activate_decode: down_proj at M <= 4 straight from the bf16 gate | up matrix (nothing is staged)
inline bool down_activate_supported(int M, int N, const int K[3], bool w4, int cus) {
    const size_t Kt = (size_t)K[0] + K[1] + K[2];
    return M >= 1 && M <= 4 && dq::operand_bytes(M, K) + quant_tail_budget(N, Kt, w4, cus) + 64 <= QUANT_LDS_WG;
}
// The fused gate | up launch with the activation inside: N = 2 I rows of weights, 128 gate | 128 up alternating
inline bool gate_up_act_supported(int M, int N, const int K[3], bool from_bf16, bool rms, int cus, const StreamOverrides &ov) {
    if (!ov.gate_up_act_stream || M < 1 || N < 256 || (N % 256) != 0) return false;
    if ((N + 63) / 64 < cus) return false;          // 64-row workgroups: at least one per CU, else the two-launch form
    const size_t Kt = (size_t)K[0] + K[1] + K[2];
    // on quantized rows, one or two token tiles: the stage of plan_gate_up_act's configuration (its reduction image is at most 64 KB)
    if (!from_bf16) return M <= 32 && stage_bytes(StreamCfg{4, M <= 16 ? 1 : 2, 2, 4}, true, (int)(Kt >> 7)) <= STREAM_LDS_MAX;
    if (M > 4 || (rms && Kt > (size_t)dq::RMS_MAX_K)) return false;
    const size_t norm = rms ? round16(dq::rms_bytes(M, K)) : 0;
    // (the tail: three segments' reduction image of (4, 1, 2, 4), 48 KB; the rings, 32 KB, + the scale image stay below it; the group
    // buffer lies in the staged row's range, which must hold it)
    const size_t tail = (size_t)red_image_bytes(StreamCfg{4, 1, 2, 4}, 3);
    return Kt * 2 >= (size_t)ACT_GROUP_BYTES && dq::operand_bytes(M, K) + 16 + norm + Kt * 2 + tail + 64 <= QUANT_LDS_WG &&
           scale_image_bytes(4, 4, (int)(Kt >> 7)) <= (int)tail - ring_bytes(StreamCfg{4, 1, 2, 4}, true, true);
}

}  // namespace stream
}  // namespace mm
