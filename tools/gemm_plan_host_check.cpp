// Stand-alone check of the tiled GEMM's host side (micromix_amd/csrc/mx_gemm_plan.h: tile choice, grids, splits, workspace sizes, the
// grouped and device-sized choices) for CU counts other than the current device's and at the edge values of M, N, K around every tile
// size.  It makes no HIP call, so it runs anywhere, and under the host sanitizers:
//   c++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/gemm_plan_host_check.cpp -o gemm_plan_host_check
//   ./gemm_plan_host_check
// (tests/test_gemm_dispatch_cpu.py compiles it without the sanitizers and runs it.)  Exit status 0: every invariant held.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/micromix_hip.h"
#include "../micromix_amd/csrc/mx_gemm_plan.h"

using namespace mm;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (++failures <= 40) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd(unsigned n) {      // xorshift: the same partitions on every run
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (unsigned)((rng_state >> 32) % n);
}

// the launches of a plan cover the M x N outputs exactly once
static void check_cover(const TilePlan &p, int M, int N, const char *what) {
    const int tn = (N + 255) / 256;
    EXPECT(p.launches == (p.kind == TK_G256_TAIL ? 2 : 1), "%s: kind %d with %d launches", what, p.kind, p.launches);
    long long cols = 0;
    for (int i = 0; i < p.launches; ++i) {
        const TileLaunch &l = p.launch[i];
        const TileShape &t = tile_shape(l.tile);
        const int per = p.splits ? p.splits : 1;
        if (p.launches == 1) {
            EXPECT(l.n_tile0 == 0 && l.n_tiles == 0, "%s: one launch over columns %d + %d", what, l.n_tile0, l.n_tiles);
            EXPECT(l.wgs == tile_count(t, M, N) * per && l.wgs > 0, "%s: M %d N %d tile %s: %d workgroups", what, M, N, t.ns, l.wgs);
        } else {
            EXPECT(t.bn == 256 && l.n_tile0 == cols && l.n_tiles > 0, "%s: launch %d starts at column %d, not %lld", what, i, l.n_tile0, cols);
            EXPECT(l.wgs == ((M + t.bm - 1) / t.bm) * l.n_tiles, "%s: launch %d: %d workgroups for %d columns", what, i, l.wgs, l.n_tiles);
            cols += l.n_tiles;
        }
    }
    if (p.launches == 2) {
        EXPECT(cols == tn, "%s: the two launches cover %lld of %d tile columns", what, cols, tn);
        EXPECT(p.launch[0].tile == TK_G256 && p.launch[1].tile == TK_G128 && p.launch[1].n_tiles == p.tail_cols, "%s: tail split of tiles %d, %d", what,
               p.launch[0].tile, p.launch[1].tile);
        EXPECT(0 < p.tail_cols && p.tail_cols < tn, "%s: %d tail columns of %d", what, p.tail_cols, tn);
    } else {
        EXPECT(p.tail_cols == 0, "%s: %d tail columns without a tail launch", what, p.tail_cols);
    }
}

static size_t mul_ok(size_t a, size_t b) {
    const unsigned __int128 r = (unsigned __int128)a * b;
    EXPECT(r <= SIZE_MAX, "a workspace size overflows size_t");
    return (size_t)r;
}

static void check_plan(int M, int N, const int K[3], bool force, bool tz, size_t ws, int cus, const GemmOverrides &ov, bool pinned) {
    char what[160];
    snprintf(what, sizeof(what), "cus %d M %d N %d K %d,%d,%d force %d tz %d ws %zu", cus, M, N, K[0], K[1], K[2], force, tz, ws);
    const TilePlan p = plan_tiles(M, N, K, ws, force, tz, cus, ov);
    check_cover(p, M, N, what);
    const int n[3] = {K[0] >> 7, K[1] >> 7, K[2] >> 7}, total = n[0] + n[1] + n[2];
    const size_t tiles128 = (size_t)((M + 127) / 128) * ((N + 255) / 256);
    if (p.kind == TK_SPLITK) {
        EXPECT(p.splits >= 2 && p.splits <= 16 && p.split_first[0] == 0 && p.split_first[3] == p.splits, "%s: split-K %d", what, p.splits);
        for (int i = 0; i < 3; ++i) {
            const int parts = p.split_first[i + 1] - p.split_first[i];
            EXPECT(parts >= 0 && (n[i] ? parts >= 1 && parts <= n[i] : parts == 0), "%s: segment %d of %d slabs in %d parts", what, i, n[i], parts);
        }
        if (ov.splitk <= 0) EXPECT((long long)tiles128 * p.splits <= cus, "%s: split-K %d on %zu tiles is more than one round", what, p.splits, tiles128);
        const size_t need = (tz ? (size_t)MM_WS_TICKET_BYTES : 0) + mul_ok(mul_ok(tiles128, (size_t)p.splits), 128u * 1024u);
        EXPECT(splitk_bytes(M, N, p.splits, tz) == need && need <= ws, "%s: split-K workspace %zu, formula %zu", what, splitk_bytes(M, N, p.splits, tz), need);
    } else if (p.kind == TK_SMALL_SPLIT) {
        const SmallSplit &s = p.small;
        EXPECT(tz && M > 64, "%s: in-kernel split without zeroed tickets or at M <= 64", what);
        EXPECT((s.kind == TK_G32N || s.kind == TK_G32) && s.kind == p.launch[0].tile && s.tiles == tile_count(s.kind, M, N), "%s: in-kernel split on tile %d", what, s.kind);
        EXPECT(s.splits == p.splits && s.splits >= 2 && s.splits <= 16 && s.splits <= total, "%s: in-kernel split-K %d of %d slabs", what, s.splits, total);
        if (!pinned) EXPECT((long long)s.tiles * s.splits <= cus, "%s: %d tiles x %d splits is more than one round", what, s.tiles, s.splits);
        EXPECT((size_t)s.tiles * 4 <= MM_TICKET_BYTES, "%s: %d tickets do not fit", what, s.tiles);
        const size_t part = s.kind == TK_G32N ? 64u * 64u * 4u : 64u * 128u * 4u;      // one workgroup's fp32 outputs
        const size_t need = (size_t)MM_WS_TICKET_BYTES + mul_ok(mul_ok((size_t)s.tiles, (size_t)s.splits + 2), part);
        EXPECT(small_split_bytes(s) == need && need <= ws, "%s: in-kernel split workspace %zu, formula %zu", what, small_split_bytes(s), need);
    } else {
        EXPECT(p.splits == 0 && p.small.splits == 0, "%s: kind %d with splits", what, p.kind);
    }
    // the size query is the plan's own need when everything is offered, and a plan that is offered less falls back to an unsplit kind
    const size_t want = plan_workspace_bytes(M, N, K, force, tz, cus, ov);
    const TilePlan all = plan_tiles(M, N, K, SIZE_MAX, force, tz, cus, ov);
    if (want == 0) {
        EXPECT(all.splits == 0, "%s: a split although the size query says 0", what);
    } else {
        // (a tail of in-kernel tickets that do not fit falls through to the two-launch split-K: both are splits)
        EXPECT(all.splits > 0 || all.small.tiles * 4 > (int)MM_TICKET_BYTES, "%s: %zu bytes wanted and no split with them", what, want);
        const TilePlan exact = plan_tiles(M, N, K, want, force, tz, cus, ov);
        EXPECT(exact.kind == all.kind && exact.splits == all.splits, "%s: the exact workspace gives kind %d, everything gives %d", what, exact.kind, all.kind);
        const TilePlan none = plan_tiles(M, N, K, 0, force, tz, cus, ov);
        EXPECT(none.splits == 0 && none.kind != TK_SPLITK && none.kind != TK_SMALL_SPLIT, "%s: a split without workspace", what);
        if (all.kind == TK_SMALL_SPLIT) {
            const TilePlan less = plan_tiles(M, N, K, want - 1, force, tz, cus, ov);
            EXPECT(less.kind != TK_SMALL_SPLIT, "%s: the in-kernel split with one byte too few", what);
            check_cover(less, M, N, what);
        }
    }
    char buf[224];
    describe_tile_plan(buf, sizeof(buf), p, K, true, false, true);
    EXPECT(strlen(buf) < sizeof(buf) - 1 && strstr(buf, tile_shape(p.launch[0].tile).ns) != nullptr, "%s: describe string '%s'", what, buf);
}

int main() {
    static_assert(MM_TICKET_BYTES == MM_WS_TICKET_BYTES, "MM_WS_TICKET_BYTES of include/micromix_hip.h");
    const int cu_counts[] = {1, 8, 32, 64, 80, 228, 256, 304, 1024};
    std::vector<int> edges;
    for (int t : {32, 64, 128, 256})
        for (int mult : {1, 2, 3, 4, 8, 16, 33})
            for (int d : {-1, 0, 1}) edges.push_back(t * mult + d);
    edges.push_back(1);
    edges.push_back(16);
    edges.push_back(17);
    const int Ks[][3] = {{0, 0, 128}, {0, 0, 256}, {128, 0, 0}, {128, 128, 128}, {0, 0, 4096}, {2048, 128, 1920}, {1024, 1024, 12288}, {0, 0, 8192}, {256, 0, 128}};
    const GemmOverrides dflt;
    long long plans = 0;
    for (int cus : cu_counts) {
        for (int M : edges)
            for (int N : edges) {
                for (const auto &K : Ks)
                    for (int mode = 0; mode < 5; ++mode) {
                        const bool force = mode == 2 || mode == 4, tz = mode >= 3;
                        check_plan(M, N, K, force, tz, mode == 0 ? 0 : (size_t)1 << 40, cus, dflt, false);
                        ++plans;
                    }
                // the fused gate / up epilogue and the 256-feature tiles
                if (plan_act_supported(M, N)) {
                    const TilePlan p = plan_act(M, N, cus);
                    check_cover(p, M, N, "plan_act");
                    EXPECT(p.launch[0].tile == TK_G256 || p.launch[0].tile == TK_G128, "plan_act: M %d N %d on tile %d", M, N, p.launch[0].tile);
                    EXPECT(p.launch[0].tile != TK_G128 || tile_count(TK_G128, M, N) <= cus, "plan_act: M %d N %d: 128-row tiles over one round", M, N);
                }
                // the small-M rule hands M > 64 to the tiles and never M <= 16
                EXPECT(plan_small_m_uses_tiles(M, N, Ks[4], 0, false, cus, dflt) == (M > 64) || (M > 16 && M <= 64), "small M rule at M %d", M);
                // grouped: one group of M > 64 rows gets the tile of a single problem without workspace (tail and 32 x 64 tiles aside)
                if (M > 64) {
                    GemmOverrides plain;
                    plain.tail = 0, plain.tile16 = 0;
                    const GroupPlan g = plan_grouped(&M, 1, N, cus);
                    const TilePlan p = plan_tiles(M, N, Ks[4], 0, false, false, cus, plain);
                    EXPECT(p.launches == 1 && g.tile == p.launch[0].tile && g.wgs == p.launch[0].wgs, "grouped: cus %d M %d N %d: tile %d x %lld, single %d x %d", cus,
                           M, N, g.tile, g.wgs, p.launch[0].tile, p.launch[0].wgs);
                }
            }
        // overrides: every pinned tile covers, pinned splits keep their bounds
        for (int tile : {16, 32, 33, 64, 128, 256, 7})
            for (int M : {65, 257, 4000})
                for (int N : {256, 3000, 14336}) {
                    GemmOverrides ov;
                    ov.tile = tile;
                    check_plan(M, N, Ks[4], false, true, (size_t)1 << 40, cus, ov, false);
                    check_plan(M, N, Ks[4], false, false, 0, cus, ov, false);
                }
        for (int S : {0, 2, 4, 16, 40})
            for (int kind : {33, 32, 5})
                for (int M : {65, 129, 513})
                    for (int N : {256, 1024, 4096}) {
                        GemmOverrides ov;
                        ov.splitk = S;
                        check_plan(M, N, Ks[5], false, false, (size_t)1 << 40, cus, ov, true);
                        GemmOverrides os;
                        os.split_small = S == 0 ? 1 : 2, os.split_small_tile = kind, os.split_small_S = S;
                        check_plan(M, N, Ks[5], false, true, (size_t)1 << 40, cus, os, true);
                    }
        // device-sized groups: the host bound is at least the tiles of any partition of n rows into E groups, on every tile
        for (int E : {1, 2, 8, 64})
            for (int n : {1, 63, 64, 65, 771, 3400, 20000})
                for (int N : {256, 384, 2048, 14336})
                    for (int wide = 0; wide < 2; ++wide) {
                        const GroupPlan g = plan_moe(E, n, N, cus, wide != 0);
                        EXPECT(g.wgs == moe_tile_bound(g.tile, E, n, N) && g.wgs > 0, "moe: E %d n %d N %d: %lld workgroups", E, n, N, g.wgs);
                        EXPECT(!wide || g.tile == TK_G128 || g.tile == TK_G256, "moe: the fused epilogue on tile %d", g.tile);
                        const TileShape &t = tile_shape(g.tile);
                        for (int trial = 0; trial < 8; ++trial) {
                            int left = n;
                            long long row_tiles = 0;
                            for (int e = 0; e < E; ++e) {
                                const int m = e == E - 1 ? left : (trial == 0 ? (left > 0) : (int)rnd((unsigned)left + 1));
                                row_tiles += (m + t.bm - 1) / t.bm;
                                left -= m;
                            }
                            EXPECT(g.wgs >= row_tiles * ((N + t.bn - 1) / t.bn), "moe: E %d n %d N %d tile %s: bound %lld under %lld row tiles", E, n, N, t.ns, g.wgs, row_tiles);
                        }
                    }
    }
    printf("%lld plans checked; %d failures\n", plans, failures);
    return failures ? 1 : 0;
}
