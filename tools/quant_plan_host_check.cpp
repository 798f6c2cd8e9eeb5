// Stand-alone check of the activation quantizers' host side (micromix_amd/csrc/mx_quant_plan.h: threads, kernel choice, LDS sizes, limits to
// raise and grids of reorder_quantize.hip, rmsnorm_quantize.hip and qlinear_decode.hip) for twelve CU counts between 1 and 1024 and every
// K that is a multiple of 128 up to 32768.  The invariants are the ones the kernels depend on and state only in comments.  It makes no
// HIP call, so it runs anywhere, and under the host sanitizers:
//   c++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/quant_plan_host_check.cpp -o quant_plan_host_check
//   c++ -std=c++20 -O1 tools/quant_plan_host_check.cpp -o quant_plan_host_check        (tests/test_quant_dispatch_cpu.py: without them)
//   ./quant_plan_host_check                    the invariants; exit status 0: every one held
//   ./quant_plan_host_check --list             the sweep of tests/golden/quant_dispatch_v1.json for 256 CUs, one line per case
//   ./quant_plan_host_check --cases            the sweep's cases alone
//   ./quant_plan_host_check --plan "CASE" ...  the plan of each case for 256 CUs (--cus N: another count).  A case is one of
//       reorder MODE ROWS K KN KS KO | grouped MODE MAX_ROWS GROUPS K KN KS KO | moe MODE SLOTS K KN KS KO | moeact SLOTS K KN KS KO
//       rms ROWS K KN KS KO INT ADD | decode M N KN KS KO NORM W4
//     MODE: x, w (both the mixed formats) or w4; INT: the integer rounding; ADD: the residual; NORM: 0 none, 1 RMSNorm, 2 residual add +
//     RMSNorm; K: the input row length (>= KN + KS + KO); with an optional MICROMIX_RMS_RING=v / MICROMIX_DECODE_PERSIST=0 behind it.
// A line: the case, then the launch: the kernel, threads, LDS bytes, the kernel whose dynamic-LDS limit is raised and to what (or none),
// the grid when the occupancy query answers 1 and when it answers 6, and what the kernel is told (slot: the ring's slot bytes; rows: the
// decode launch's staged rows) -- "none" where the launcher returns without a launch, "error" where it refuses.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../micromix_amd/csrc/mx_quant_plan.h"

using namespace mm::quant;

static long long failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (++failures <= 40) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

enum CaseKind { C_REORDER, C_GROUPED, C_MOE, C_MOEACT, C_RMS, C_DECODE };
struct Case {
    CaseKind kind;
    std::string mode;      // reorder family: x, w, w4
    int rows;              // reorder / rms: rows; grouped: the largest group's; moe: the slots; decode: M
    int groups, N;
    int K, Kseg[3];
    int int_round, add;    // rms
    int norm, w4;          // decode
    int ring_pin = -1, persist = 1;
    std::string ov_text;
};

static bool set_override(Case &c, const char *text) {
    const char *eq = strchr(text, '=');
    if (!eq) return false;
    const std::string name(text, eq - text);
    if (name == "MICROMIX_RMS_RING") c.ring_pin = atoi(eq + 1);
    else if (name == "MICROMIX_DECODE_PERSIST") c.persist = !(eq[1] == '0');
    else return false;
    c.ov_text = text;
    return true;
}

static bool parse_case(const char *text, Case &c) {
    char kind[16] = "", mode[16] = "", ov[64] = "";
    int used = 0, v[8] = {}, n = 0;
    c = Case{};
    if (sscanf(text, "%15s%n", kind, &used) != 1) return false;
    const char *p = text + used;
    const char *const names[] = {"reorder", "grouped", "moe", "moeact", "rms", "decode"};
    int k = -1;
    for (int i = 0; i < 6; ++i)
        if (!strcmp(kind, names[i])) k = i;
    if (k < 0) return false;
    c.kind = (CaseKind)k;
    if (k <= C_MOE) {
        if (sscanf(p, "%15s%n", mode, &used) != 1 || (strcmp(mode, "x") && strcmp(mode, "w") && strcmp(mode, "w4"))) return false;
        p += used, c.mode = mode;
    }
    while (n < 8 && sscanf(p, "%d%n", &v[n], &used) == 1) p += used, ++n;
    sscanf(p, "%63s", ov);
    const int want[] = {5, 6, 5, 5, 7, 7};
    if (n != want[k]) return false;
    int i = 0;
    c.rows = v[i++];
    if (k == C_GROUPED) c.groups = v[i++];
    if (k == C_DECODE) c.N = v[i++];
    else c.K = v[i++];
    for (int g = 0; g < 3; ++g) c.Kseg[g] = v[i++];
    if (k == C_DECODE) c.K = c.Kseg[0] + c.Kseg[1] + c.Kseg[2], c.norm = v[i++], c.w4 = v[i++];
    if (k == C_RMS) c.int_round = v[i++], c.add = v[i++];
    return ov[0] == 0 || set_override(c, ov);
}

static std::string case_text(const Case &c) {
    char buf[256];
    int n = 0;
    switch (c.kind) {
        case C_REORDER: n = snprintf(buf, sizeof(buf), "reorder %s %d %d %d %d %d", c.mode.c_str(), c.rows, c.K, c.Kseg[0], c.Kseg[1], c.Kseg[2]); break;
        case C_GROUPED: n = snprintf(buf, sizeof(buf), "grouped %s %d %d %d %d %d %d", c.mode.c_str(), c.rows, c.groups, c.K, c.Kseg[0], c.Kseg[1], c.Kseg[2]); break;
        case C_MOE: n = snprintf(buf, sizeof(buf), "moe %s %d %d %d %d %d", c.mode.c_str(), c.rows, c.K, c.Kseg[0], c.Kseg[1], c.Kseg[2]); break;
        case C_MOEACT: n = snprintf(buf, sizeof(buf), "moeact %d %d %d %d %d", c.rows, c.K, c.Kseg[0], c.Kseg[1], c.Kseg[2]); break;
        case C_RMS: n = snprintf(buf, sizeof(buf), "rms %d %d %d %d %d %d %d", c.rows, c.K, c.Kseg[0], c.Kseg[1], c.Kseg[2], c.int_round, c.add); break;
        case C_DECODE: n = snprintf(buf, sizeof(buf), "decode %d %d %d %d %d %d %d", c.rows, c.N, c.Kseg[0], c.Kseg[1], c.Kseg[2], c.norm, c.w4); break;
    }
    if (!c.ov_text.empty()) snprintf(buf + n, sizeof(buf) - n, " %s", c.ov_text.c_str());
    return buf;
}

static const char *tf(bool b) { return b ? "true" : "false"; }

// the instantiation a plan names, as the launchers pick it (one place per file there; this is the same table as text)
static std::string reorder_kernel(const char *family, bool w4, const ReorderPlan &p) {
    char buf[96];
    if (!strcmp(family, "moe_activate_quantize_kernel")) snprintf(buf, sizeof(buf), "%s<%d>", family, p.max_threads);
    else snprintf(buf, sizeof(buf), "%s<%s,%d>", family, tf(w4), p.max_threads);
    return buf;
}
static std::string rms_kernel(const RmsPlan &p, bool int_round, bool add) {
    char buf[96];
    const char *stage = add ? "RowAddResidual" : "RowLoad";
    if (rms_ring_depth(p.kernel)) snprintf(buf, sizeof(buf), "rmsnorm_quantize_ring_kernel<%s,%d>", tf(int_round), rms_ring_depth(p.kernel));
    else if (p.kernel == RMS_PRODUCTS) snprintf(buf, sizeof(buf), "rmsnorm_quantize_products_kernel<%s,%s>", tf(int_round), stage);
    else snprintf(buf, sizeof(buf), "rmsnorm_quantize_kernel<%s,%d,%s>", tf(int_round), p.kernel == RMS_STAGED2 ? 2 : 1, stage);
    return buf;
}
static std::string decode_kernel(const DecodePlan &p, bool w4, int norm) {
    char buf[96];
    snprintf(buf, sizeof(buf), "qlinear_decode%s_kernel<%s,%s,%d,%s>", p.features == 16 ? "16" : "", tf(w4), tf(norm != 0), p.pairs ? 2 : 1, tf(norm == 2));
    return buf;
}

static std::string launch_text(const std::string &kern, const mm::LaunchShape &one, const mm::LaunchShape &six) {
    char buf[384];
    std::string raise = "none";
    if (one.raise_to) raise = kern + ":" + std::to_string(one.raise_to);
    snprintf(buf, sizeof(buf), "kern=%s thr=%d lds=%d raise=%s grid=%dx%d grid6=%dx%d", kern.c_str(), one.threads, one.lds_bytes, raise.c_str(), one.grid_x, one.grid_y,
             six.grid_x, six.grid_y);
    return buf;
}

// what the launcher of a case does, from the plan functions the launchers call
static std::string answer(const Case &c, int cus) {
    const bool w4 = c.mode == "w4";
    switch (c.kind) {
        case C_REORDER: {
            if (c.rows == 0) return "none";
            const ReorderPlan p = plan_reorder_quantize(c.K, c.Kseg[0], c.Kseg[1], c.Kseg[2], w4);
            return launch_text(reorder_kernel("reorder_quantize_kernel", w4, p), p.shape(resident_grid(c.rows, cus, 1)), p.shape(resident_grid(c.rows, cus, 6)));
        }
        case C_GROUPED: {
            if (c.groups < 1 || c.groups > 8 || c.rows < 1) return "error";
            const ReorderPlan p = plan_reorder_quantize(c.K, c.Kseg[0], c.Kseg[1], c.Kseg[2], w4);
            return launch_text(reorder_kernel("reorder_quantize_grouped_kernel", w4, p), p.shape(resident_grid(c.rows, cus, 1, c.groups), c.groups),
                               p.shape(resident_grid(c.rows, cus, 6, c.groups), c.groups));
        }
        case C_MOE:
        case C_MOEACT: {
            if (c.rows == 0) return "none";
            const bool act = c.kind == C_MOEACT;
            const ReorderPlan p = plan_reorder_quantize(c.K, c.Kseg[0], c.Kseg[1], c.Kseg[2], !act && w4);
            return launch_text(reorder_kernel(act ? "moe_activate_quantize_kernel" : "moe_quantize_kernel", w4, p), p.shape(c.rows), p.shape(c.rows));
        }
        case C_RMS: {
            if (c.rows == 0) return "none";
            const RmsPlan p = plan_rmsnorm_quantize(c.rows, c.K, c.Kseg[1], c.Kseg[2], c.add != 0, cus, c.ring_pin);
            std::string s = launch_text(rms_kernel(p, c.int_round != 0, c.add != 0), p.shape(resident_grid(c.rows, cus, 1)), p.shape(resident_grid(c.rows, cus, 6)));
            if (rms_ring_depth(p.kernel)) s += " slot=" + std::to_string(p.slot_bytes);
            return s;
        }
        case C_DECODE: {
            const DecodePlan p = plan_qlinear_decode(c.rows, c.N, c.Kseg, c.norm != 0, c.norm == 2, c.w4 != 0, cus, c.persist != 0);
            return launch_text(decode_kernel(p, c.w4 != 0, c.norm), p.shape(), p.shape()) + " rows=" + std::to_string(p.stage_rows);
        }
    }
    return "error";
}

// ---- the sweep of the fixture (256 CUs) ----
static const int LIST_K[] = {128, 384, 4096, 8192, 8320, 16384, 16512, 20480, 24576, 24704, 28672, 32768};
static const int LIST_ROWS[] = {0, 1, 2, 512, 513, 4096};      // 512 = 2 x 256 CUs: the ring's boundary
// a K split at the extremes: all N, all S, all O, mixed (half | quarter | the rest, in 128s)
static void split_of(int K, int which, int out[3]) {
    const int n = K / 128;
    out[0] = out[1] = out[2] = 0;
    if (which < 3) out[which] = K;
    else out[0] = n / 2 * 128, out[1] = (n - n / 2) / 2 * 128, out[2] = K - out[0] - out[1];
}
static Case make(CaseKind kind, const char *mode, int rows, int K, const int Kseg[3]) {
    Case c = {};
    c.kind = kind, c.mode = mode, c.rows = rows, c.K = K;
    for (int g = 0; g < 3; ++g) c.Kseg[g] = Kseg[g];
    return c;
}
// Every K with every row count on the mixed split (rows decide the grid, K and the split the rest); the other splits at three rows
static std::vector<Case> fixture_sweep() {
    std::vector<Case> out;
    int S[3];
    for (int K : LIST_K)
        for (int which = 3; which >= 0; --which) {
            const bool full = which == (K == 128 ? 2 : 3);      // (one slab: the mixed split is all O)
            if (which == 3 && !full) continue;
            split_of(K, which, S);
            for (const char *mode : {"x", "w", "w4"})
                for (int rows : LIST_ROWS)
                    if (full || (rows == 2 && strcmp(mode, "w"))) out.push_back(make(C_REORDER, mode, rows, K, S));
            for (int add = 0; add < 2; ++add)
                for (int rows : LIST_ROWS)
                    if (full || rows == 2) {
                        Case c = make(C_RMS, "", rows, K, S);
                        c.int_round = 1, c.add = add;
                        out.push_back(c);
                    }
            if (!full) continue;
            // the norm without the integer rounding, and with a pinned ring (K > 8192 has no ring to pin: one K beyond)
            for (int add = 0; add < 2; ++add)
                for (const char *ov : {"", "MICROMIX_RMS_RING=0", "MICROMIX_RMS_RING=3", "MICROMIX_RMS_RING=4"})
                    for (int int_round = 0; int_round < 2; ++int_round)
                        for (int rows : {1, 513}) {
                            if (int_round && !ov[0]) continue;      // (above)
                            if (ov[0] && (K > 8320 || (!int_round && (add || rows != 1)))) continue;
                            Case c = make(C_RMS, "", rows, K, S);
                            c.int_round = int_round, c.add = add;
                            if (ov[0] && !set_override(c, ov)) abort();
                            out.push_back(c);
                        }
            for (int slots : {0, 513}) {
                for (const char *mode : {"x", "w", "w4"}) out.push_back(make(C_MOE, mode, slots, K, S));
                out.push_back(make(C_MOEACT, "", slots, K, S));
            }
            if (K != 128 && K != 4096 && K != 8320 && K != 24576 && K != 24704 && K != 32768) continue;
            for (const char *mode : {"x", "w4"})
                for (int groups : {1, 3, 8})
                    for (int rows : LIST_ROWS) {
                        Case c = make(C_GROUPED, mode, rows, K, S);
                        c.groups = groups;
                        out.push_back(c);
                    }
        }
    // a gathering launch: the input row is longer than what is produced (mm_reorder_quantize_gather)
    for (const char *mode : {"x", "w4"})
        for (int K : {8192, 32768}) {
            const int small[3] = {128, 128, 128};
            out.push_back(make(C_REORDER, mode, 3, K, small));
        }
    // the decode launch, where at least one staged row fits and the norm's tree covers K; matching-precision weights and the A/B switch
    // (which only the 32-feature kernel reads: N / 32 above half the CUs) on a thinner grid
    const int DK[][3] = {{2048, 128, 1920}, {4096, 4096, 0}, {0, 0, 16384}};
    for (const char *ov : {"", "MICROMIX_DECODE_PERSIST=0"})
        for (const auto &K : DK)
            for (int w4 = 1; w4 >= 0; --w4)
                for (int norm = 0; norm < 3; ++norm)
                    for (int N : {4096, 8192, 14336, 28672})
                        for (int M = 1; M <= 8; ++M) {
                            if (!decode_fits(M, K, norm != 0) || (norm && K[0] + K[1] + K[2] > mm::dq::RMS_MAX_K)) continue;
                            if (!w4 && M != 1 && M != 4 && M != 8) continue;
                            if (ov[0] && (!w4 || norm == 2 || (M != 1 && M != 8))) continue;
                            Case c = make(C_DECODE, "", M, K[0] + K[1] + K[2], K);
                            c.N = N, c.norm = norm, c.w4 = w4;
                            if (ov[0] && !set_override(c, ov)) abort();
                            out.push_back(c);
                        }
    return out;
}

// ---- the invariants ----
static void check_shape(const char *what, int K, const int S[3], int threads, int max_threads, int lds, int raise_to) {
    EXPECT(threads > 0 && threads % 64 == 0 && threads <= max_threads, "%s K %d (%d,%d,%d): %d threads on a kernel bounded to %d", what, K, S[0], S[1], S[2], threads, max_threads);
    EXPECT(lds <= LDS_RAISE_ABOVE || raise_to != 0, "%s K %d (%d,%d,%d): %d bytes of LDS and no limit raised", what, K, S[0], S[1], S[2], lds);
    EXPECT(lds > 0 && (raise_to == 0 || (lds <= raise_to && raise_to <= 160 * 1024)), "%s K %d (%d,%d,%d): %d bytes of LDS with the limit at %d", what, K, S[0], S[1], S[2], lds,
           raise_to);
}

static long long check_invariants() {
    long long cases = 0;
    const int cu_counts[] = {1, 2, 8, 64, 80, 228, 255, 256, 257, 304, 512, 1024};
    int S[3];
    for (int K = 128; K <= 32768; K += 128)
        for (int which = 0; which < 5; ++which) {
            // (which == 4: a gathering launch -- a 32768-long input row, the split of K)
            split_of(K, which < 4 ? which : 3, S);
            const int Kin = which == 4 ? 32768 : K;
            for (int w4 = 0; w4 < 2; ++w4) {
                const ReorderPlan p = plan_reorder_quantize(Kin, S[0], S[1], S[2], w4 != 0);
                check_shape("reorder", Kin, S, p.threads, p.max_threads, p.lds_bytes, p.raise_to), ++cases;
                EXPECT(p.max_threads == 256 || p.max_threads == 1024, "reorder K %d: no kernel bounded to %d", Kin, p.max_threads);
                // one thread per group produced and per four 16-byte chunks staged
                EXPECT(p.threads >= K / 32 && 4 * p.threads >= Kin / 8, "reorder K %d of %d: %d threads", K, Kin, p.threads);
                EXPECT(p.lds_bytes >= Kin * 2 + (w4 ? 0 : S[1] / 4 * 3 + S[2]), "reorder K %d: %d bytes of LDS", Kin, p.lds_bytes);
            }
            if (which == 4) continue;
            for (int cus : cu_counts)
                for (int rows : {1, 2, 2 * cus, 2 * cus + 1, 4096})
                    for (int add = 0; add < 2; ++add)
                        for (int pin : {-1, 0, 3, 4}) {
                            const RmsPlan p = plan_rmsnorm_quantize(rows, K, S[1], S[2], add != 0, cus, pin);
                            const int T = K / 32, NTH = p.threads, R = rms_ring_depth(p.kernel);
                            ++cases;
                            check_shape("rms", K, S, p.threads, rms_max_threads(p.kernel), p.lds_bytes, p.raise_to);
                            EXPECT(p.P >= 64 && p.P >= T && (p.P == 64 || p.P / 2 < T) && (p.P & (p.P - 1)) == 0 && p.pslots >= p.P, "rms K %d: P %d, %d slots", K, p.P, p.pslots);
                            if (R) {
                                // the kernel's trap condition, its static_assert, and what a ring cannot do
                                EXPECT(K <= RMS_RING_MAX_K && !add, "rms K %d add %d: a ring plan", K, add);
                                EXPECT(NTH == roundup64(T), "rms K %d: the ring kernel with %d threads traps", K, NTH);
                                EXPECT(R == 3 || R == 4, "rms K %d: ring depth %d", K, R);
                                EXPECT(p.slot_bytes >= K * 2 && p.slot_bytes % 1024 == 0 && p.lds_bytes >= R * p.slot_bytes + 1024 + p.pslots * 4 + S[1] / 4 * 3 + S[2], "rms K %d: slot %d", K,
                                       p.slot_bytes);
                                EXPECT(pin >= 3 || (pin < 0 && rows <= 2 * cus), "rms K %d rows %d pin %d @ %d CUs: a ring plan", K, rows, pin, cus);
                            }
                            // rms_tree_rvar and the products kernel's tree walk at most four slots per lane
                            if (R || p.kernel == RMS_PRODUCTS) EXPECT(p.P <= 256 && NTH >= T && p.P <= 2 * NTH, "rms K %d: P %d on %d threads", K, p.P, NTH);
                            if (p.kernel == RMS_PRODUCTS) EXPECT(p.lds_bytes >= K * 4 + p.pslots * 4 + S[1] / 4 * 3 + S[2], "rms K %d: %d bytes for the products row", K, p.lds_bytes);
                            // one group thread per thread: every slot up to P is written or zeroed, every step of the tree is taken in full
                            if (p.kernel == RMS_STAGED1) EXPECT(NTH >= T && p.P <= 2 * NTH && p.pslots >= NTH, "rms K %d: P %d on %d threads", K, p.P, NTH);
                            // two group threads per thread: what the comment on part[] in rmsnorm_quantize_kernel argues from
                            if (p.kernel == RMS_STAGED2)
                                EXPECT(NTH >= 256 && 2 * NTH >= T && T <= 1024 && 512 + NTH >= T && 3 * NTH >= 512 + NTH && p.pslots >= 2 * NTH, "rms K %d: T %d on %d threads", K, T, NTH);
                            if (!R && p.kernel != RMS_PRODUCTS) EXPECT(p.lds_bytes >= K * 2 + p.pslots * 4 + S[1] / 4 * 3 + S[2], "rms K %d: %d bytes for the row", K, p.lds_bytes);
                        }
        }
    // one resident wave of workgroups, at most `rows`; a grouped launch's groups share it
    for (int cus : cu_counts)
        for (int per_cu : {1, 2, 6, 16})
            for (int groups : {1, 3, 8})
                for (int rows : {1, 2, cus - 1, cus, cus * per_cu, cus * per_cu + 1, 1 << 20}) {
                    if (rows < 1) continue;
                    const int g = resident_grid(rows, cus, per_cu, groups);
                    ++cases;
                    EXPECT(g >= 1 && g <= rows && (g * groups <= cus * per_cu || g == 1), "%d rows, %d groups @ %d x %d: grid %d", rows, groups, cus, per_cu, g);
                    EXPECT(g == rows || (g + 1) * groups > cus * per_cu, "%d rows, %d groups @ %d x %d: grid %d leaves room", rows, groups, cus, per_cu, g);
                }
    // the decode launch
    const int DK[][3] = {{0, 0, 128}, {128, 128, 128}, {2048, 128, 1920}, {0, 4096, 0}, {4096, 4096, 0}, {0, 0, 8192}, {0, 0, 8320}, {1024, 1024, 12288}, {0, 0, 16384},
                         {16384, 8192, 8192}, {32768, 0, 0}, {0, 0, 32768}};
    for (int cus : cu_counts)
        for (const auto &K : DK)
            for (int M = 1; M <= 8; ++M)
                for (int norm = 0; norm < 3; ++norm)
                    for (int persist = 0; persist < 2; ++persist)
                        for (int mult : {1, 2, 3})
                            for (int d : {-1, 0, 1})
                                for (int bn : {16, 32}) {
                                    const int N = (cus * mult + d) * bn - (d ? bn - 1 : 0), Kt = K[0] + K[1] + K[2];
                                    if (N < 1 || !decode_fits(M, K, norm != 0) || (norm && Kt > mm::dq::RMS_MAX_K)) continue;
                                    const DecodePlan p = plan_qlinear_decode(M, N, K, norm != 0, norm == 2, false, cus, persist != 0);
                                    ++cases;
                                    EXPECT(p.stage_rows >= 1 && p.stage_rows <= M, "decode M %d K %d: %d staged rows", M, Kt, p.stage_rows);
                                    EXPECT(p.lds_bytes <= DECODE_LDS_MAX && p.lds_bytes <= p.raise_to && p.raise_to <= 160 * 1024, "decode M %d K %d: %d bytes of LDS", M, Kt, p.lds_bytes);
                                    EXPECT((size_t)p.lds_bytes == (size_t)p.stage_rows * Kt * 2 + decode_operand_bytes(M, K, norm != 0), "decode M %d K %d: %d bytes of LDS", M, Kt, p.lds_bytes);
                                    EXPECT(p.pairs == (2 * p.stage_rows * (Kt / 32) <= 512), "decode M %d K %d: pairs %d with %d staged rows", M, Kt, p.pairs, p.stage_rows);
                                    EXPECT(p.features == 16 || p.features == 32, "decode N %d: %d features", N, p.features);
                                    const int all = (N + p.features - 1) / p.features;
                                    // 16 features and the A/B switch: one workgroup per block; else the 32-feature kernel walks its blocks, one workgroup per CU
                                    EXPECT(p.blocks == (p.features == 32 && persist && all > cus ? cus : all), "decode N %d @ %d CUs: %d workgroups for %d blocks", N, cus, p.blocks, all);
                                    EXPECT(p.shape().threads == DECODE_THREADS && p.shape().grid_y == 1, "decode: the workgroup");
                                }
    return cases;
}

int main(int argc, char **argv) {
    int cus = 256;
    if (argc >= 2 && (!strcmp(argv[1], "--list") || !strcmp(argv[1], "--cases"))) {
        for (const Case &c : fixture_sweep()) {
            if (argv[1][2] == 'l') printf("%s : %s\n", case_text(c).c_str(), answer(c, cus).c_str());
            else printf("%s\n", case_text(c).c_str());
        }
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "--plan")) {
        for (int i = 2; i < argc; ++i) {
            if (!strcmp(argv[i], "--cus") && i + 1 < argc) {
                cus = atoi(argv[++i]);
                continue;
            }
            Case c;
            if (!parse_case(argv[i], c)) {
                fprintf(stderr, "not a case: %s\n", argv[i]);
                return 2;
            }
            printf("%s : %s\n", case_text(c).c_str(), answer(c, cus).c_str());
        }
        return 0;
    }
    const long long cases = check_invariants();
    printf("%lld cases checked; %lld failures\n", cases, failures);
    return failures ? 1 : 0;
}
