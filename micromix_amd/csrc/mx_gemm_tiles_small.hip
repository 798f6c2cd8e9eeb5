// The tiles for launches that cannot fill the chip with 128-row tiles -- 128 x 128 (8 waves), 64 x 128 / 64 x 64 (4 compute + 4 loader
// waves), 32 x 64 (2 + 2) -- in a translation unit of their own, so that hipcc compiles them beside mx_gemm256.hip (round 6: one file
// took 100 s of a 105 s build).  plan_tiles / plan_small_split (mx_gemm_plan.h) choose; the launchers below are all that mx_gemm256.hip sees.
#include "mx_gemm_prelude.h"

namespace mm {

#define MM_NS g64
#define MM_MAX_STAGES 3
#define MM_LDS_BUDGET (160 * 1024)
#define MM_WM 4
#define MM_TM 1
#define MM_TN 2
#define MM_ACC MM_ACC_CLOBBER
#include "mx_gemm_tile.inc"
#undef MM_NS
#undef MM_WM
#undef MM_TM
#undef MM_TN
#undef MM_ACC
#undef MM_MAX_STAGES
#undef MM_LDS_BUDGET
#define MM_NS g32
#define MM_MAX_STAGES 3
#define MM_LDS_BUDGET (160 * 1024)
#define MM_WM 2
#define MM_TM 1
#define MM_TN 2
#define MM_ACC MM_ACC_CLOBBER32
#include "mx_gemm_tile.inc"
#undef MM_NS
#undef MM_WM
#undef MM_TM
#undef MM_TN
#undef MM_ACC
#undef MM_MAX_STAGES
#undef MM_LDS_BUDGET
#define MM_NS g32n
#define MM_MAX_STAGES 3
#define MM_LDS_BUDGET (160 * 1024)
#define MM_WM 2
#define MM_TM 1
#define MM_TN 1
#define MM_ACC MM_ACC_CLOBBER32
#include "mx_gemm_tile.inc"
#undef MM_NS
#undef MM_WM
#undef MM_TM
#undef MM_TN
#undef MM_ACC
#undef MM_MAX_STAGES
#undef MM_LDS_BUDGET
#define MM_NS g16
#define MM_MAX_STAGES 3
#define MM_LDS_BUDGET (160 * 1024)
#define MM_WM 1
#define MM_TM 1
#define MM_TN 1
#define MM_ACC MM_ACC_CLOBBER32
#include "mx_gemm_tile.inc"
#undef MM_NS
#undef MM_WM
#undef MM_TM
#undef MM_TN
#undef MM_ACC
#undef MM_MAX_STAGES
#undef MM_LDS_BUDGET


MM_TILE_KERNELS(g64, TK_G64);
MM_TILE_KERNELS(g32, TK_G32);
MM_TILE_KERNELS(g32n, TK_G32N);
MM_TILE_KERNELS(g16, TK_G16);
static_assert((size_t)g32n::NACC * g32n::NT * 4 == SMALL_PART_BYTES_64x64 && (size_t)g32::NACC * g32::NT * 4 == SMALL_PART_BYTES_64x128,
              "partial-sum slot sizes of the in-kernel split-K (mx_gemm_plan.h)");

// splitk: the in-kernel split-K variants (split_tile_reduce; 64 x 128 and 64 x 64 tiles only)
hipError_t launch_small_tile(TileKind tile, bool w4, bool splitk, int wgs, const GemmArgs &a, hipStream_t stream) {
    switch (tile) {
        case TK_G32N: return splitk ? launch_gemm<g32n_row, true>(w4, wgs, a, stream) : launch_gemm<g32n_row>(w4, wgs, a, stream);
        case TK_G32: return splitk ? launch_gemm<g32_row, true>(w4, wgs, a, stream) : launch_gemm<g32_row>(w4, wgs, a, stream);
        case TK_G64: return splitk ? hipErrorInvalidValue : launch_gemm<g64_row>(w4, wgs, a, stream);
        case TK_G16: return splitk ? hipErrorInvalidValue : launch_gemm<g16_row>(w4, wgs, a, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_small_tile_grouped(TileKind tile, bool w4, int total, const GroupedTileArgs &ga, hipStream_t stream) {
    switch (tile) {
        case TK_G32N: return launch_grouped<g32n_row>(w4, total, ga, stream);
        case TK_G32: return launch_grouped<g32_row>(w4, total, ga, stream);
        case TK_G64: return launch_grouped<g64_row>(w4, total, ga, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_small_tile_moe(TileKind tile, bool w4, int total, const GemmArgs &a, const MoeGroups &mg, hipStream_t stream) {
    switch (tile) {
        case TK_G32N: return launch_moe<g32n_row>(w4, total, a, mg, stream);
        case TK_G32: return launch_moe<g32_row>(w4, total, a, mg, stream);
        case TK_G64: return launch_moe<g64_row>(w4, total, a, mg, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mm
