// What a translation unit that includes mx_gemm_tile.inc needs in front of it (mx_gemm256.hip; developer probes include it too).
#pragma once
#include <hip/hip_ext.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include <utility>

#include "mx_acc_regs.h"
#ifndef MM_FP4_KD256
#define MM_FP4_KD256 1  // fp4 x fp4 segment on 256-deep slabs (whole cache lines per row); 0 = 128-deep slabs like the other segments
#endif
#ifndef MM_PRIO
#define MM_PRIO 1        // s_setprio for waves 4-7 of the 8-wave tiles (mx_gemm_tile.inc, tile_body); 0 = none
#endif
#include "mx_instrument.h"   // MM_DBG ablation switches and MM_CLOCKS: constant 0 unless built with -DMM_INSTRUMENT
#ifndef MM_PINGPONG
#define MM_PINGPONG 1  // the ping-pong K loop for one-segment fp8 x fp4 launches on the 256-row tile (mx_gemm_tile.inc, run_pingpong); 0 = lock-step loop
#endif
#ifndef MM_CHAIN
#define MM_CHAIN 1  // chained segment hand-over on the 256-row tile (mx_gemm_tile.inc); 0 = every segment's own prologue (A/B builds)
#endif
#include "mx_common.h"
#include "mx_buffer_ops.h"   // MM_DEVICE_ONLY, make_rsrc / make_brsrc, lds_address, dma16: once, for every tile namespace
#include "mx_direct_convert.h"
#include "mx_group_convert.h"
#include "mx_kernels.h"
#include "mx_gemm_plan.h"    // the tile table and the whole host-side plan (no HIP in it)

namespace mm {

// in-kernel split-K (split_tile_reduce): scope of the ticket atomics and cache-policy bits of the partial-sum traffic
#define MM_SPLIT_SCOPE __HIP_MEMORY_SCOPE_AGENT
#define MM_SPLIT_AUX 16   // sc1 = device scope
#ifndef MM_SPLIT_FENCES
// 1 = spell the hand-over of the in-kernel split-K with agent-scope release / acquire fences and an acq_rel ticket (split_tile_reduce).
// Measured (round 4, tools/time_cases.py, k/v at M = 128, back-to-back launches through the Python shim, alternating processes):
// 23.3 / 23.6 us with the fences against 16.1 / 16.4 us without -- every wave's buffer_wbl2 sc1 walks the L2 although nothing of
// this kernel is dirty there -- so the default is 0: the same ordering from the instructions that are already needed (see there).
#define MM_SPLIT_FENCES 0
#endif

static_assert(MM_PLAN_MAX_SPLITS == MM_MAX_SPLITS, "the plan's split bound is GemmArgs' (mx_gemm_plan.h)");

// The one launch of a tile kernel: launch_kernel (mx_kernels.h; the streaming kernels' launch_stream is the same call), which owns the
// kernel's dynamic-LDS flag.  A tile kernel's limit is raised to its LDS before its first launch, whatever the size.
struct LaunchDims { int wgs, threads, lds_bytes; };
template <auto Kern, class... Args>
static hipError_t launch_tile(LaunchDims d, hipStream_t stream, DiagEvents ev, const Args &...args) {
    return launch_kernel<Kern>(LaunchShape{d.wgs, 1, d.threads, d.lds_bytes, d.lds_bytes}, stream, ev, args...);
}

// The kernel table: one row per tile namespace, made where mx_gemm_tile.inc was included for it.  A row names the namespace's kernels by
// family and weight mode and ties it to its entry of the plan's tile table; the launchers below are written once over a row.
#define MM_TILE_KERNELS(ns, KIND)                                                                                              \
    struct ns##_row {                                                                                                          \
        template <bool W4> static constexpr LaunchDims dims(int wgs) { return LaunchDims{wgs, ns::NTHREADS, ns::Lds<W4>::TOTAL}; } \
        template <bool W4, bool SPLITK> static constexpr auto gemm = ns::mx_gemm256_kernel<W4, SPLITK>;                        \
        template <bool W4> static constexpr auto grouped = ns::mx_gemm256_grouped_kernel<W4>;                                  \
        template <bool W4> static constexpr auto moe = ns::mx_gemm256_moe_kernel<W4>;                                          \
    };                                                                                                                         \
    static_assert(ns::BM == tile_shape(KIND).bm && ns::BN == tile_shape(KIND).bn, "the plan's tile table (mx_gemm_plan.h)")

template <class Row, bool SPLITK = false>
static hipError_t launch_gemm(bool w4, int wgs, const GemmArgs &a, hipStream_t stream) {
    const DiagEvents ev{a.ev_start, a.ev_stop};
    return w4 ? launch_tile<Row::template gemm<true, SPLITK>>(Row::template dims<true>(wgs), stream, ev, a)
              : launch_tile<Row::template gemm<false, SPLITK>>(Row::template dims<false>(wgs), stream, ev, a);
}
// grouped launch (launch_mx_gemm256_grouped has filled ga.first_block[]; wgs = all groups' tiles)
template <class Row>
static hipError_t launch_grouped(bool w4, int wgs, const GroupedTileArgs &ga, hipStream_t stream) {
    return w4 ? launch_tile<Row::template grouped<true>>(Row::template dims<true>(wgs), stream, DiagEvents{}, ga)
              : launch_tile<Row::template grouped<false>>(Row::template dims<false>(wgs), stream, DiagEvents{}, ga);
}
// device-sized grouped launch (wgs = the host bound of plan_moe)
template <class Row>
static hipError_t launch_moe(bool w4, int wgs, const GemmArgs &a, const MoeGroups &mg, hipStream_t stream) {
    return w4 ? launch_tile<Row::template moe<true>>(Row::template dims<true>(wgs), stream, DiagEvents{}, a, mg)
              : launch_tile<Row::template moe<false>>(Row::template dims<false>(wgs), stream, DiagEvents{}, a, mg);
}

// the tiles for launches with few tiles live in mx_gemm_tiles_small.hip (compiled beside mx_gemm256.hip): tile = TK_G64, TK_G32,
// TK_G32N or TK_G16 (gemm; splitk, the in-kernel split-K variants, on TK_G32 and TK_G32N only), the first three (grouped, moe)
hipError_t launch_small_tile(TileKind tile, bool w4, bool splitk, int wgs, const GemmArgs &a, hipStream_t stream);
hipError_t launch_small_tile_grouped(TileKind tile, bool w4, int total, const GroupedTileArgs &ga, hipStream_t stream);
hipError_t launch_small_tile_moe(TileKind tile, bool w4, int total, const GemmArgs &a, const MoeGroups &mg, hipStream_t stream);

}  // namespace mm
