// Host side of the tiled GEMM (mx_gemm256.hip, mx_gemm_tiles_small.hip): which tile a launch runs on, with what grid, split and
// workspace, and the string that says so.  Plain C++ without a HIP include: everything takes the CU count and the developer overrides
// as arguments, so the whole plan can be computed for any machine on any machine (tools/gemm_plan_host_check.cpp checks its invariants
// over CU counts from 1 to 1024, tests/test_gemm_dispatch_cpu.py replays a recorded sweep).  The launchers read the plan and the tile
// table below, the describe functions print them: there is no second copy of a rule.  The constants that come from the kernels are
// static_asserted against the tile namespaces where those are compiled (MM_TILE_KERNELS, mx_gemm_prelude.h).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdio.h>

namespace mm {

// Which kernel(s) a problem runs on: decided once here, used by the launcher and by mm_matmul_describe.  The six kinds that are one
// launch of one tile namespace also name that tile (tile_shape): what launch_small_tile* and the grouped plans take and return.
enum TileKind { TK_SPLITK, TK_SMALL_SPLIT, TK_G64, TK_G256_TAIL, TK_G256, TK_G128, TK_G32, TK_G32N, TK_G16 };

// the tile table: one entry per tile namespace of mx_gemm_tile.inc (BM tokens x BN features per workgroup)
struct TileShape { TileKind kind; const char *ns; int bm, bn; };
constexpr TileShape TILE_SHAPES[6] = {{TK_G256, "g256", 256, 256}, {TK_G128, "g128", 128, 256}, {TK_G64, "g64", 128, 128},
                                      {TK_G32, "g32", 64, 128},    {TK_G32N, "g32n", 64, 64},   {TK_G16, "g16", 32, 64}};
constexpr const TileShape &tile_shape(TileKind kind) {
    for (const TileShape &t : TILE_SHAPES)
        if (t.kind == kind) return t;
    return TILE_SHAPES[kind == TK_SPLITK ? 1 : 0];     // the two-launch split-K runs on the 128 x 256 tiles, the tail split starts on 256 x 256
}
constexpr long long tile_count(const TileShape &t, long long M, long long N) { return ((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn); }
constexpr long long tile_count(TileKind kind, long long M, long long N) { return tile_count(tile_shape(kind), M, N); }

constexpr int MM_PLAN_MAX_SPLITS = 16;                 // in-kernel split-K: splits per tile (= MM_MAX_SPLITS, mx_kernels.h)
constexpr int SPLIT_WG_FLOATS = 32768;                 // two-launch split-K: 128 KiB of fp32 partial sums per 128 x 256 workgroup
constexpr size_t SMALL_PART_BYTES_64x64 = 16 * 256 * 4, SMALL_PART_BYTES_64x128 = 32 * 256 * 4;   // fp32 accumulators of one workgroup (in-kernel split-K)
constexpr size_t MM_TICKET_BYTES = 4096;   // = mm_matmul_ticket_bytes(): room for 1024 tiles (a launch of this kind has at most CUs / 2)

// The developer overrides, read from the environment once per process (gemm_overrides(), mx_gemm256.hip); the defaults are "unset".
struct GemmOverrides {
    int tile = 0;              // MICROMIX_GEMM_TILE: 256, 128, 64 (128 x 128), 32 (64 x 128), 33 (64 x 64) or 16 (32 x 64) pins the tile
    int tail = 1;              // MICROMIX_GEMM_TAIL=0: no tail balancing
    int tile16 = 1;            // MICROMIX_GEMM_TILE16=0: no 32 x 64 tiles above M = 64
    int splitk = -1;           // MICROMIX_SPLITK: 0 disables the two-launch split-K, S pins its split count
    int split_small = 0;       // MICROMIX_SPLIT_SMALL: 0 unset, 1 "=0" (disabled), 2 "=<tile>:<S>" pinned to ...
    int split_small_tile = 0;  // ... tile 33 (64 x 64) or 32 (64 x 128; anything else: no split) ...
    int split_small_S = 0;     // ... and S splits
    int small_m_tiles = 0;     // MICROMIX_SMALL_M_TILES=1: M <= 16 may run on the tiles (A/B runs)
    int mid_m_stream = 0;      // MICROMIX_MID_M_STREAM=1: 32 < M <= 64 always on the weight-streaming kernel
    int small_m_tile16 = 1;    // MICROMIX_SMALL_M_TILE16=0: no 32 x 64 tiles for 32 < M <= 64
};

// ---------------------------------------------------------------------------------------------------------
// The round rule.  One workgroup fits per CU, so a launch runs in rounds of `cus` tiles; `tiles(kind)` is the launch's tile count on
// that tile (one problem, the sum over a group, or a host bound on it).
//  * Fewer than a CU's worth of 128-row tiles: the 4-wave tiles (64 rows, loader / compute waves, see mx_gemm_tile.inc) fill more
//    CUs.  64 x 64 while those fit one round of workgroups (M <= 256 at N = 4096: 11-12 us against 17 us at K = 4096), 64 x 128
//    while THEY fit one round and the 128 x 128 tiles would leave half of the CUs idle (M = 512 at N = 4096: 14.7 against 17.7).
//  * 256-row tiles move the fewest L2->LDS bytes per flop; a round of 128-row tiles takes ~0.62 of a round of 256-row tiles
//    (measured).  So 128-row tiles pay exactly when they still fit in ONE round (tiles128 <= cus, i.e. at most half of the CUs would
//    get a 256-row tile): M=2048, N=4096 46.5 -> 33 us; with 160 256-row tiles (320 128-row tiles = two rounds) the 256-row tiles
//    win, 62 vs 76 us.
//  * ... and when even the 128-row tiles would occupy at most half of the CUs, 128 x 128 tiles double the workgroups once
//    more (1.5x the L2->LDS bytes per flop, which does not matter while half of the chip idles): M = 1024, N = 4096.
// wide_only: the fused gate / up epilogue exists on the 256-feature tiles alone, so only the last two lines apply.
// ---------------------------------------------------------------------------------------------------------
template <class Tiles>
inline TileKind round_rule(Tiles tiles, int cus, bool wide_only = false) {
    const long long t128 = tiles(TK_G128);
    if (!wide_only) {
        const long long t64 = tiles(TK_G64);
        if (tiles(TK_G32N) <= cus) return TK_G32N;
        if (tiles(TK_G32) <= cus && 2 * t64 <= cus) return TK_G32;
        if (2 * t128 <= cus && t64 <= cus) return TK_G64;
    }
    return t128 <= cus ? TK_G128 : TK_G256;
}
inline TileKind round_rule(int M, int N, int cus, bool wide_only = false) {
    return round_rule([&](TileKind k) { return tile_count(k, M, N); }, cus, wide_only);
}

// Tail balancing: tiles256 = q * CUs + R runs q + 1 rounds and the last one leaves CUs idle.
// When R <= CUs / 2 and R is a whole number of tile columns, those columns are run as 128-row tiles instead (2R
// workgroups of half the work: the last round takes half the time).  gate/up at M = 4096: 896 tiles = 3.5 rounds.
// Returns that number of 256-feature tile columns, 0 for none (a launch the round rule gave the 256 x 256 tile).
inline int tail_columns(int M, int N, int cus) {
    const int tm256 = (M + 255) / 256, tiles256 = tm256 * ((N + 255) / 256), rem = tiles256 % cus;
    return (tiles256 > cus && rem > 0 && 2 * rem <= cus && rem % tm256 == 0) ? rem / tm256 : 0;
}

// Number of K splits for (M, N, K) and the segment each split works on; 0 = do not split.
// Cost model fitted to MI355X measurements (tools/bench_shapes.py): a workgroup of a launch with few tiles walks one
// 128-deep slab in ~0.7 us (DMA-latency bound), and every split adds tiles * 128 KiB of fp32 partial sums that are
// written and read back at ~4 TB/s (0.064 us per tile and split), plus ~5 us for the second launch:
//     t(S) = 0.7 * slabs / S + 0.064 * tiles * S (+ 5)   ->   S* = 3.3 * sqrt(slabs / tiles)
// Split only when that beats the unsplit launch (the tile the round rule would pick at these tile counts) by a margin.
// `force` (MM_SPLIT_K_ALWAYS, tests and tuning) skips the model.  MICROMIX_SPLITK=0 disables splitting, =S pins the split count.
inline int plan_splits(int M, int N, const int K[3], bool force, int first[4], int cus, const GemmOverrides &ov) {
    const int pinned = ov.splitk;
    if (pinned == 0 || M <= 32) return 0;
    const int tiles = (int)tile_count(TK_G128, M, N);
    int n[3], total = 0, nonempty = 0;
    for (int i = 0; i < 3; ++i) {
        n[i] = K[i] >> 7;
        total += n[i];
        nonempty += n[i] > 0;
    }
    int cap = cus / tiles; // one wave of workgroups on the CUs
    cap = cap > 16 ? 16 : cap;
    cap = cap > total / 2 ? total / 2 : cap;  // at least two slabs per split on average
    if (cap < 2 || cap < nonempty) return 0;
    int S;
    if (pinned > 0 || force) {
        S = pinned > 0 ? pinned : cap;
    } else {
        S = (int)(3.3f * sqrtf((float)total / (float)tiles) + 0.5f);
        S = S < nonempty ? nonempty : S;
        S = S > cap ? cap : S;
        // unsplit: 128 x 128 tiles walk a slab in ~0.5 us; the 4-wave tiles (when the round rule would pick them: one round of
        // workgroups) in ~0.32 us (64 x 64) / ~0.36 us (64 x 128).  Margins fitted to tools/mid_m_sweep.py (down_proj, K = 14336:
        // split at M <= 384, unsplit 64 x 128 tiles at M = 512; k/v and q/o at K = 4096: never split).
        const TileKind un = round_rule(M, N, cus);
        const float unsplit = (un == TK_G32N ? 0.32f : un == TK_G32 ? 0.36f : 0.5f) * total, margin = un == TK_G32 ? 0.95f : 0.85f;
        const float split = 0.7f * total / S + 0.064f * tiles * S + 5.0f;
        if (S < 2 || split > margin * unsplit) return 0;
    }
    S = S > cap ? cap : S;
    if (S < 2 || S < nonempty) return 0;
    // segments get splits in proportion to their slab counts, at least one each and never more than their slabs
    int parts[3], used = 0;
    for (int i = 0; i < 3; ++i) {
        parts[i] = n[i] ? (S * n[i]) / total : 0;
        if (n[i] && parts[i] == 0) parts[i] = 1;
        used += parts[i];
    }
    while (used != S) {
        int best = -1;
        for (int i = 0; i < 3; ++i) {
            if (!n[i]) continue;
            if (used < S) {  // give a split to the segment with the longest slab run per split
                if (parts[i] < n[i] && (best < 0 || n[i] * parts[best] > n[best] * parts[i])) best = i;
            } else {         // take one from the segment with the shortest
                if (parts[i] > 1 && (best < 0 || n[i] * parts[best] < n[best] * parts[i])) best = i;
            }
        }
        if (best < 0) break;
        parts[best] += used < S ? 1 : -1;
        used += used < S ? 1 : -1;
    }
    first[0] = 0;
    for (int i = 0; i < 3; ++i) first[i + 1] = first[i] + parts[i];
    return first[3];
}
// workspace of that plan: with MM_WS_TICKETS_ZEROED the head of the workspace belongs to the ticket counters, the partial sums start behind it
inline size_t splitk_bytes(int M, int N, int splits, bool tickets_zeroed) {
    return (tickets_zeroed ? MM_TICKET_BYTES : 0) + (size_t)tile_count(TK_G128, M, N) * splits * SPLIT_WG_FLOATS * sizeof(float);
}

// ---------------------------------------------------------------------------------------------------------
// In-kernel split-K of the 4-wave tiles (split_tile_reduce in mx_gemm_tile.inc): a launch whose 64 x 64 tiles occupy at most half
// of the CUs cuts K into `splits` equal slab ranges, one workgroup each, and the last workgroup of a tile to finish
// reduces.  Workspace: [tickets: MM_TICKET_BYTES, one 32-bit counter per tile, zero between launches][tiles x (<= splits + 2)
// partial-sum slots].
// What it is worth, measured on MI355X.  Phases of ONE cold launch (tools/split_clock.py, in-kernel clock stamps): a workgroup needs
// ~2.5-3.5 us from its start to its first finished slab and ~0.3 us per 128-deep slab after that; the split adds ~0.6 us (partial
// sums acknowledged, ticket) and one round trip of ~2 us for the reducing workgroup's reads (the partial sums are written through to
// memory: the eight XCDs' L2s are not coherent for plain accesses).  Kernel durations in a queue of back-to-back launches
// (tools/split_small_sweep.py: dispatch events, settled; K = 4096, (2048,128,1920)), unsplit / 2 / 4 / 6 splits:
//   32 tiles (k/v, N = 1024, M = 128)   11.3 / 10.7 /  9.5 /  8.9 us        64 tiles (N = 2048, M = 128)  12.7 / 11.2 / 11.5 / 15.2
//   48 tiles (N = 1024, M = 192)        11.4 / 10.9 / 10.0 / 12.6           128 tiles (q/o, M = 128)      12.9 / 12.0 / 19.8 / 19.9
//   64 tiles (N = 1024, M = 256)        11.2 / 11.2 / 10.8 / 13.9           256 tiles (q/o, M = 256)      12.8 / 22.7
// More than one round of workgroups (tiles x splits > CUs) always loses.  Two splits at 64 ... 128 tiles are a wash: an A/B on a second
// box (alternating processes, profiles/notes_r03.md section 14) had the unsplit launch at 11.4 / 11.4 / 12.7 us and two splits at
// 12.0 / 12.3 / 12.0 for q/o at M = 128.  Hence the rule below: six splits up to 32 tiles, four up to 48, none above, at least four
// slabs per split.  MICROMIX_SPLIT_SMALL=0 disables it, =<tile>:<S> (tile 33 = 64 x 64,
// 32 = 64 x 128; the latter never won) pins a plan (tools, tests); MM_SPLIT_K_ALWAYS relaxes the rule to "any split that fits one
// round of workgroups".
// ---------------------------------------------------------------------------------------------------------
struct SmallSplit {
    TileKind kind;     // TK_G32N (64 x 64 tiles) or TK_G32 (64 x 128 tiles)
    int splits;        // 0 = none
    int tiles;
};
constexpr size_t small_part_bytes(TileKind kind) { return kind == TK_G32N ? SMALL_PART_BYTES_64x64 : SMALL_PART_BYTES_64x128; }
// a split leaves one partial sum per segment it touches: at most splits + 2 slots per tile
inline size_t small_split_bytes(const SmallSplit &p) { return p.splits ? MM_TICKET_BYTES + (size_t)p.tiles * (p.splits + 2) * small_part_bytes(p.kind) : 0; }

inline SmallSplit plan_small_split(int M, int N, const int K[3], bool force, int cus, const GemmOverrides &ov) {
    const SmallSplit none{TK_G32N, 0, 0};
    if (M <= 64 || ov.split_small == 1) return none;   // (M <= 64: the weight-streaming kernels, mx_gemm.hip)
    const int total = (K[0] >> 7) + (K[1] >> 7) + (K[2] >> 7);
    const int t32n = (int)tile_count(TK_G32N, M, N), t32 = (int)tile_count(TK_G32, M, N);
    if (ov.split_small == 2) {
        const int kind = ov.split_small_tile, S = ov.split_small_S;
        if ((kind == 33 || kind == 32) && S >= 2 && S <= MM_PLAN_MAX_SPLITS && S <= total)
            return kind == 33 ? SmallSplit{TK_G32N, S, t32n} : SmallSplit{TK_G32, S, t32};
        return none;
    }
    if (force) {    // tests: the most splits that fit one round of workgroups, 64 x 64 tiles while those fit, else 64 x 128
        for (TileKind kind : {TK_G32N, TK_G32}) {
            const int tiles = kind == TK_G32N ? t32n : t32;
            int S = cus / (tiles > 0 ? tiles : 1);
            S = S > MM_PLAN_MAX_SPLITS ? MM_PLAN_MAX_SPLITS : S;
            S = S > total / 2 ? total / 2 : S;
            if (S >= 2) return SmallSplit{kind, S, tiles};
        }
        return none;
    }
    // measured rule (see above): six splits up to 32 tiles, four up to 48, none above (two splits at 64 ... 128 tiles measured equal
    // to the unsplit launch within the box-to-box spread); never more than one round of workgroups, at least four slabs per split
    // (longer K -- down_proj, 112 slabs -- stays with the two-launch split-K of the 128-row tiles, which cuts it into up to 16)
    if (total > 64) return none;
    int S = t32n <= 32 ? 6 : t32n <= 48 ? 4 : 0;
    S = S > total / 4 ? total / 4 : S;
    S = (S == 5 || S == 3) ? S - 1 : S;
    return S >= 2 && t32n * S <= cus ? SmallSplit{TK_G32N, S, t32n} : none;
}

// one kernel launch of a plan: `wgs` workgroups of tile `tile` over the 256-feature tile columns [n_tile0, n_tile0 + n_tiles) (0, 0 = all)
struct TileLaunch { TileKind tile; int wgs, n_tile0, n_tiles; };
struct TilePlan {
    TileKind kind;
    TileLaunch launch[2];      // TK_G256_TAIL: two launches; every other kind: one (TK_SPLITK: + the reduction kernel)
    int launches;
    int tail_cols;             // TK_G256_TAIL: the last tail_cols tile columns run as 128 x 256 tiles
    int splits, split_first[4];   // TK_SPLITK: splits [split_first[i], split_first[i+1]) work on segment i; TK_SMALL_SPLIT: splits = small.splits
    SmallSplit small;
};

inline TilePlan one_launch(TileKind kind, TileKind tile, int M, int N, int per_tile = 1) {
    TilePlan p{};
    p.kind = kind;
    p.launch[0] = TileLaunch{tile, (int)tile_count(tile, M, N) * per_tile, 0, 0};
    p.launches = 1;
    return p;
}
// tile k of the round rule, with the tail balancing when that is the 256 x 256 tile and `tail` allows it
inline TilePlan balanced_launch(TileKind k, int M, int N, int cus, bool tail) {
    const int c = k == TK_G256 && tail ? tail_columns(M, N, cus) : 0;
    if (c == 0) return one_launch(k, k, M, N);
    const int tn = (N + 255) / 256;
    TilePlan p{};
    p.kind = TK_G256_TAIL;
    p.tail_cols = c;
    p.launch[0] = TileLaunch{TK_G256, (int)tile_count(TK_G256, M, 256) * (tn - c), 0, tn - c};
    p.launch[1] = TileLaunch{TK_G128, (int)tile_count(TK_G128, M, 256) * c, tn - c, c};
    p.launches = 2;
    return p;
}

// ws_bytes: the caller's workspace, 0 for none (never split)
inline TilePlan plan_tiles(int M, int N, const int K[3], size_t ws_bytes, bool force_split, bool tickets_zeroed, int cus, const GemmOverrides &ov) {
    if (ws_bytes > 0) {
        const SmallSplit small = tickets_zeroed ? plan_small_split(M, N, K, force_split, cus, ov) : SmallSplit{TK_G32N, 0, 0};
        if (small.splits && small.tiles * 4 <= (int)MM_TICKET_BYTES && small_split_bytes(small) <= ws_bytes) {
            TilePlan p = one_launch(TK_SMALL_SPLIT, small.kind, M, N, small.splits);
            p.small = small;
            p.splits = small.splits;
            return p;
        }
        int first[4];
        const int S = plan_splits(M, N, K, force_split, first, cus, ov);
        if (S && splitk_bytes(M, N, S, tickets_zeroed) <= ws_bytes) {
            TilePlan p = one_launch(TK_SPLITK, TK_G128, M, N, S);
            p.splits = S;
            for (int i = 0; i < 4; ++i) p.split_first[i] = first[i];
            return p;
        }
    }
    switch (ov.tile) {         // kernel-developer override: the tile, no tail balancing
        case 0: break;
        case 32: return one_launch(TK_G32, TK_G32, M, N);
        case 33: return one_launch(TK_G32N, TK_G32N, M, N);
        case 16: return one_launch(TK_G16, TK_G16, M, N);
        case 64: return one_launch(TK_G64, TK_G64, M, N);
        case 128: return one_launch(TK_G128, TK_G128, M, N);
        case 256: return one_launch(TK_G256, TK_G256, M, N);
        default: return balanced_launch(round_rule(M, N, cus, true), M, N, cus, false);     // any other value: the 256-feature tiles by the round rule
    }
    // 64 x 64 tiles on at most half of the CUs (q/o at M <= 128: 128 tiles): 32 x 64 tiles (two compute + two loader waves) double the
    // workgroups; every workgroup then walks its K with half the LDS traffic per slab (round 4, tools/time_cases.py)
    if (ov.tile16 && tile_count(TK_G16, M, N) <= 2 * cus && (2 * tile_count(TK_G32N, M, N) <= cus || M <= 32))   // (M <= 32: one row of tiles, see plan_small_m_uses_tiles)
        return one_launch(TK_G16, TK_G16, M, N);
    return balanced_launch(round_rule(M, N, cus), M, N, cus, ov.tail != 0);
}

// mm_matmul_workspace_bytes: what the plan above would use when it is offered everything; 0 when mm_matmul would not split K for this shape
inline size_t plan_workspace_bytes(int M, int N, const int K[3], bool force, bool tickets_zeroed, int cus, const GemmOverrides &ov) {
    const SmallSplit sp = tickets_zeroed ? plan_small_split(M, N, K, force, cus, ov) : SmallSplit{TK_G32N, 0, 0};
    if (sp.splits) return small_split_bytes(sp);
    int first[4];
    const int S = plan_splits(M, N, K, force, first, cus, ov);
    return S ? splitk_bytes(M, N, S, tickets_zeroed) : 0;
}

// 32 < M <= 64: the weight-streaming kernel (two token tiles per workgroup, N / 32 workgroups) against the tiles.  Measured
// (tools/mid_m_sweep.py 40 48 56 64): the skinny kernel costs ~10-13 us per ROUND of its workgroups at K = 4096, the 64-row tiles
// 11-14 us flat, so the tiles win once N / 32 exceeds the CUs (gate/up, N = 14336: 22-25 -> 14 us); and a long K that the model
// would split (down_proj, K = 14336: 25-30 us skinny) goes to the split-K tiles when the caller brought a workspace.
inline bool plan_small_m_uses_tiles(int M, int N, const int K[3], size_t ws_bytes, bool force_split, int cus, const GemmOverrides &ov) {
    // 16 < M <= 32: only with more than three rounds of 32-feature workgroups (fused gate + up, N = 28672: the 64-row tiles take
    // 19.2-20.0 us at M = 17 / 24 / 32, the weight-streaming kernel 20.7 / 22.1 / 23.9; at N <= 24576 the latter wins or ties:
    // tools/time_skinny_big_n.py, profiles/notes_r03.md section 24)
    // (round 4: with the 32 x 64 tiles also M <= 16 -- N = 28672, us at M = 1 / 8 / 16 / 24 / 32: weight-streaming or 64 x 64 tiles
    // 17.4 / 18.6 / 20.3 / 18.6 / 18.6, 32 x 64 tiles 16.7 / 16.8 / 16.7 / 16.9 / 16.9; at N <= 14336 the weight-streaming kernel wins by 1-4 us)
    // (round 4, later: the second weight-streaming kernel, mx_gemm_stream.hip, takes 14.3-14.6 us at N = 28672 and M <= 16, 20.2 at
    // M = 32 where the 32 x 64 tiles take 16.8; MICROMIX_SMALL_M_TILES=1 restores the rule above for A/B runs)
    if (M <= 16 && !ov.small_m_tiles) return false;
    if (M <= 32) return (N + 31) / 32 > 3 * cus;
    if (M > 64) return true;
    if (ov.mid_m_stream) return false;      // kernel-developer override: 32 < M <= 64 always on the weight-streaming kernel
    if ((N + 31) / 32 > cus) return true;
    // 32 < M <= 64 on one round of 32 x 64 tiles (round 4; profiles/r04_small_tiles.txt, (2048,128,1920), us): a workgroup of those
    // tiles walks K = 4096 in ~9.8 us however many of them there are.  The second weight-streaming kernel (mx_gemm_stream.hip, three /
    // four token tiles) takes 6.7 / 6.8 / 7.7 at M = 33 / 48 / 64 for N = 4096 and 14.0 / 14.7 / 17.3 on down_proj's K = 14336 (the
    // two-launch split-K: 19.5), but 14.1-16.3 against the tiles' 13.5-14.0 at N = 14336: so the tiles from N / 32 > CUs / 2 on, the
    // streaming kernel below, and the split-K plan only when the caller forces it.
    if (ov.small_m_tile16 && tile_count(TK_G16, M, N) <= cus && 2 * ((N + 31) / 32) > cus) return true;
    if (ws_bytes == 0 || !force_split) return false;
    const size_t need = plan_workspace_bytes(M, N, K, force_split, false, cus, ov);   // (the in-kernel split starts above M = 64)
    return need > 0 && need <= ws_bytes;
}

// The 256 x 256 tile's kernel variants.
// PINGPONG: a launch that is ONE fp8 x fp4 segment (K[0] = K[1] = 0: nothing is chained in) of at least two slabs walks it with the
// ping-pong K loop (mx_gemm_tile.inc, run_pingpong) in front of the tail: fp4 weights, bf16 output, no split-K (the 256-row tiles
// never split).  Mixed splits, the "w" mode, fp32 output, the fused gate / up and the grouped kernels and the 128-row tiles keep the
// lock-step loop.  -DMM_PINGPONG=0 (`pingpong_built` false) restores that selection everywhere (A/B builds of one tree).
// This kernel alone starts on accumulators that nothing has zeroed: its first K step writes them (srcC = 0), and it requests slab 0
// before any other set-up, slab 1 behind a head barrier (run_pingpong, "The head").  Every other kernel zeroes in tile_body as before.
// TAIL: the 256-row tiles with fp4 weights end with the tile-major tail (mx_gemm_tile.inc, run_tail) when it applies: bf16 output and
// at least two slabs in the last (fp8 x fp4) segment.  The "w" mode (fp8 / fp6 weights) keeps the old path, PLAIN: its kernel already
// sits at the 128-VGPR limit, and its fp8 x fp8 stage (66 KiB) leaves no third stage to free.
enum G256Variant { G256_PLAIN, G256_TAIL, G256_PINGPONG };
inline G256Variant g256_variant(const int K[3], bool w4, bool out_f32, bool pingpong_built) {
    if (!w4 || out_f32 || (K[2] >> 7) < 2) return G256_PLAIN;
    return pingpong_built && K[0] == 0 && K[1] == 0 ? G256_PINGPONG : G256_TAIL;
}

// mm_matmul_describe for a launch on the tiles: the plan's launches, named from the tile table
inline const char *describe_tile_plan(char *buf, size_t size, const TilePlan &p, const int K[3], bool w4, bool out_f32, bool pingpong_built) {
    const char *w = w4 ? "true" : "false";
    const TileShape &t = tile_shape(p.launch[0].tile);
    int n = snprintf(buf, size, "mm::%s::mx_gemm256_kernel<%s,%s> x %d workgroups (%dx%d tiles", t.ns, w, p.splits ? "true" : "false", p.launch[0].wgs, t.bm, t.bn);
    if (p.kind == TK_SPLITK) n += snprintf(buf + n, size - n, ", split-K %d) + mm::splitk_reduce_kernel", p.splits);
    else if (p.kind == TK_SMALL_SPLIT) n += snprintf(buf + n, size - n, ", in-kernel split-K %d)", p.splits);
    else n += snprintf(buf + n, size - n, ")");
    if (p.launches == 2) {
        const TileShape &u = tile_shape(p.launch[1].tile);
        n += snprintf(buf + n, size - n, " + mm::%s::mx_gemm256_kernel<%s,false> x %d (last %d tile columns as %dx%d tiles)", u.ns, w, p.launch[1].wgs, p.tail_cols, u.bm, u.bn);
    }
    if (p.launch[0].tile == TK_G256 && g256_variant(K, w4, out_f32, pingpong_built) == G256_PINGPONG) snprintf(buf + n, size - n, ", ping-pong K loop");
    return buf;
}

// ---------------------------------------------------------------------------------------------------------
// Tiled GEMM with the fused gate / up epilogue (write_tile_act in mx_gemm_tile.inc; mm_gate_up_activate): 256-feature tiles only
// (one tile = 128 gate + the 128 up features of the same indices), i.e. the 256 x 256 and 128 x 256 kernels; no split-K.  M <= 64
// stays with the weight-streaming kernels + the stand-alone activation quantizer (capi.hip).
// ---------------------------------------------------------------------------------------------------------
constexpr bool plan_act_supported(int M, int N) { return M > 64 && N > 0 && (N % 256) == 0; }
// a supported (M, N): the round rule on the 256-feature tiles and the tail balancing (kind TK_G128, TK_G256 or TK_G256_TAIL)
inline TilePlan plan_act(int M, int N, int cus) { return balanced_launch(round_rule(M, N, cus, true), M, N, cus, true); }

inline const char *describe_act_plan(char *buf, size_t size, const TilePlan &p) {
    const TileShape &t = tile_shape(p.launch[0].tile);
    const int n = snprintf(buf, size, "mm::%s::mx_gemm256_act_kernel x %d workgroups (%dx%d tiles", t.ns, p.launch[0].wgs, t.bm, t.bn);
    if (p.launches == 2) snprintf(buf + n, size - n, ") + mm::%s::mx_gemm256_act_kernel x %d", tile_shape(p.launch[1].tile).ns, p.launch[1].wgs);
    else snprintf(buf + n, size - n, ", fused silu*up + quantize)");
    return buf;
}

// ---------------------------------------------------------------------------------------------------------
// Grouped launches: ONE grid of one tile for all groups, the tile chosen for the sum of the groups' tiles with the same round rule as
// a single problem (no split-K, no tail balancing).
// ---------------------------------------------------------------------------------------------------------
struct GroupPlan { TileKind tile; long long wgs; };
inline GroupPlan plan_grouped(const int *M, int ngroups, int N, int cus) {
    auto tiles = [&](TileKind k) {
        long long t = 0;
        for (int i = 0; i < ngroups; ++i) t += tile_count(k, M[i], N);
        return t;
    };
    const TileKind k = round_rule(tiles, cus);
    return GroupPlan{k, tiles(k)};
}
// Device-sized grouped launches: the E groups' row counts (n rows in all) are on the device, so the tile comes from a host bound on
// the sum of their tiles -- n / bm + min(E, n) row tiles, since sum ceil(M_e / bm) <= sum M_e / bm + the experts with rows -- by the
// same rule, and the grid is that bound.  wide_only: the fused gate / up epilogue (mm_moe_gate_up_activate), 256-feature tiles only.
inline long long moe_tile_bound(TileKind k, int E, int n, int N) {
    const TileShape &t = tile_shape(k);
    return (long long)(n / t.bm + (E < n ? E : n)) * ((N + t.bn - 1) / t.bn);
}
inline GroupPlan plan_moe(int E, int n, int N, int cus, bool wide_only = false) {
    const TileKind k = round_rule([&](TileKind kind) { return moe_tile_bound(kind, E, n, N); }, cus, wide_only);
    return GroupPlan{k, moe_tile_bound(k, E, n, N)};
}
inline const char *describe_moe_act_plan(char *buf, size_t size, const GroupPlan &p) {
    const TileShape &t = tile_shape(p.tile);
    snprintf(buf, size, "mm::%s::mx_gemm256_moe_act_kernel x %lld workgroups (%dx%d tiles, fused silu*up + quantize)", t.ns, p.wgs, t.bm, t.bn);
    return buf;
}

}  // namespace mm
