// Stand-alone check of the weight-streaming kernels' host side (micromix_amd/csrc/mx_stream_plan.h: configuration ladders, LDS sizes, grids,
// the *_supported predicates) for twelve CU counts between 1 and 1024, around every threshold of M, N and K, with every developer
// override.  It makes no HIP call, so it runs anywhere, and under the host sanitizers:
//   c++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/stream_plan_host_check.cpp -o stream_plan_host_check
//   c++ -std=c++20 -O1 tools/stream_plan_host_check.cpp -o stream_plan_host_check        (tests/test_stream_dispatch_cpu.py: without them)
//   ./stream_plan_host_check                    the invariants; exit status 0: every one held
//   ./stream_plan_host_check --list             the sweep of tests/golden/stream_dispatch_v1.json for 256 CUs, one line per case
//   ./stream_plan_host_check --plan "CASE" ...  the plan of each case for 256 CUs (--cus N: another count).  A case is one of
//       plain M N KN KS KO W4 | grouped MAX_M GROUPS N KN KS KO W4 | moe MAX_ROWS E ROWS N KN KS KO W4 | qlinear M N KN KS KO W4 NORM
//       down M N KN KS KO W4 | act M N KN KS KO | actq M N KN KS KO NORM          (NORM: 0 none, 1 RMSNorm, 2 residual add + RMSNorm)
//     with an optional MICROMIX_...=value behind it.
// A line: the case, the predicate's answer, then the launch: cfg=F,T16,D,NW, the kernel variant, grid, threads, LDS bytes, whether the
// kernel's dynamic-LDS limit must be raised for it, and for the quantizing launches stage_rows and early -- or "invalid" where the
// launcher returns an error.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../micromix_amd/csrc/mx_stream_plan.h"

using namespace mm::stream;

static long long failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (++failures <= 40) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

enum CaseKind { C_PLAIN, C_GROUPED, C_MOE, C_QLINEAR, C_DOWN, C_ACT, C_ACTQ };
static const char *const KIND_NAMES[] = {"plain", "grouped", "moe", "qlinear", "down", "act", "actq"};
struct Case {
    CaseKind kind;
    int M, N, K[3], w4;
    int groups;        // grouped: the groups; moe: the experts
    int rows;          // moe: rows of the packed buffers
    int norm;          // qlinear / actq: 0, 1 (norm), 2 (residual add + norm)
    std::string ov_text;
    StreamOverrides ov;
};
struct Answer {
    bool supported, ok, quant;
    StreamCfg cfg;
    const char *variant;
    StreamLaunch launch;
    int stage_rows, early, qbytes;
};

static bool set_override(StreamOverrides &ov, const char *text) {
    const char *eq = strchr(text, '=');
    if (!eq) return false;
    const std::string name(text, eq - text);
    const int v = atoi(eq + 1);
    if (name == "MICROMIX_STREAM") ov.stream = v;
    else if (name == "MICROMIX_STREAM_GROUPED") ov.grouped = v;
    else if (name == "MICROMIX_STREAM_GROUPED_MAX_M") ov.grouped_max_m = v;
    else if (name == "MICROMIX_DECODE_STREAM") ov.decode_stream = v;
    else if (name == "MICROMIX_DECODE_EARLY") ov.decode_early = v;
    else if (name == "MICROMIX_DECODE_F4") ov.decode_f4 = v;
    else if (name == "MICROMIX_DECODE_DEPTH") ov.decode_depth = v;
    else if (name == "MICROMIX_GATE_UP_ACT_STREAM") ov.gate_up_act_stream = v;
    else if (name == "MICROMIX_STREAM_CFG") return sscanf(eq + 1, "%d,%d,%d", &ov.cfg_f, &ov.cfg_d, &ov.cfg_nw) == 3;
    else return false;
    return true;
}

static bool parse_case(const char *text, Case &c) {
    char kind[16] = "", ov[96] = "";
    int v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, n = 0, used = 0;
    if (sscanf(text, "%15s%n", kind, &used) != 1) return false;
    const char *p = text + used;
    while (n < 9 && sscanf(p, "%d%n", &v[n], &used) == 1) p += used, ++n;
    sscanf(p, "%95s", ov);
    c = Case{};
    int k = -1;
    for (int i = 0; i < 7; ++i)
        if (!strcmp(kind, KIND_NAMES[i])) k = i;
    if (k < 0) return false;
    c.kind = (CaseKind)k;
    const int want[] = {6, 7, 8, 7, 6, 5, 6};
    if (n != want[k]) return false;
    int i = 0;
    c.M = v[i++];
    if (k == C_GROUPED) c.groups = v[i++];
    if (k == C_MOE) c.groups = v[i++], c.rows = v[i++];
    c.N = v[i++];
    for (int g = 0; g < 3; ++g) c.K[g] = v[i++];
    c.w4 = (k == C_ACT || k == C_ACTQ) ? 1 : v[i++];
    if (k == C_QLINEAR || k == C_ACTQ) c.norm = v[i++];
    c.ov_text = ov;
    return ov[0] == 0 || set_override(c.ov, ov);
}

static std::string case_text(const Case &c) {
    char buf[256];
    int n = snprintf(buf, sizeof(buf), "%s %d", KIND_NAMES[c.kind], c.M);
    if (c.kind == C_GROUPED) n += snprintf(buf + n, sizeof(buf) - n, " %d", c.groups);
    if (c.kind == C_MOE) n += snprintf(buf + n, sizeof(buf) - n, " %d %d", c.groups, c.rows);
    n += snprintf(buf + n, sizeof(buf) - n, " %d %d %d %d", c.N, c.K[0], c.K[1], c.K[2]);
    if (c.kind != C_ACT && c.kind != C_ACTQ) n += snprintf(buf + n, sizeof(buf) - n, " %d", c.w4);
    if (c.kind == C_QLINEAR || c.kind == C_ACTQ) n += snprintf(buf + n, sizeof(buf) - n, " %d", c.norm);
    if (!c.ov_text.empty()) snprintf(buf + n, sizeof(buf) - n, " %s", c.ov_text.c_str());
    return buf;
}

// what the exported functions of mx_gemm_stream.hip answer and launch for a case, from the same plan functions
static Answer answer(const Case &c, int cus) {
    Answer a = {};
    const bool w4 = c.w4 != 0;
    a.variant = "-";
    auto count = [cus] { return cus; };
    auto gemm = [&](const GemmPlan &p) { a.ok = p.ok, a.cfg = p.cfg, a.launch = p.launch; };
    auto quant = [&](QuantKind what) {
        const StreamCfg cfg = select_quant(what, c.N, c.K, c.norm != 0, cus, c.ov);
        const QuantPlan p = plan_quant(what, cfg, w4, c.M, c.N, c.K, c.norm != 0, c.norm == 2, c.ov);
        a.quant = true, a.ok = p.ok, a.cfg = p.cfg, a.launch = p.launch, a.stage_rows = p.stage_rows, a.early = p.early, a.qbytes = p.qbytes;
        a.variant = p.act ? (p.add ? "ACT+ADD" : (p.rms ? "ACT+RMS" : "ACT")) : (p.add ? "ADD" : (p.rms ? "RMS" : "Q"));
    };
    switch (c.kind) {
        case C_PLAIN:
            a.supported = gemm_supported(c.M, c.N, c.K, w4, count, c.ov);
            gemm(plan_plain(c.M, c.N, c.K, w4, cus, c.ov));
            break;
        case C_GROUPED:
            a.supported = grouped_supported(c.M, c.groups, c.N, c.K, count, c.ov);
            gemm(plan_grouped(c.M, c.groups, c.N, c.K, w4, cus, c.ov));
            break;
        case C_MOE:
            a.supported = moe_supported(c.M, c.K, c.ov);
            gemm(plan_moe(c.M, c.groups, c.rows, c.N, c.K, w4, cus, c.ov));
            break;
        case C_QLINEAR:
            a.supported = qlinear_supported(c.M, c.N, c.K, c.norm != 0, w4, cus, c.ov);
            quant(QK_QLINEAR);
            break;
        case C_DOWN:
            a.supported = down_activate_supported(c.M, c.N, c.K, w4, cus);
            quant(QK_DOWN_ACTIVATE);
            break;
        case C_ACT:
            a.supported = gate_up_act_supported(c.M, c.N, c.K, false, false, cus, c.ov);
            gemm(plan_gate_up_act(c.M, c.N, c.K));
            break;
        case C_ACTQ:
            a.supported = gate_up_act_supported(c.M, c.N, c.K, true, c.norm != 0, cus, c.ov);
            quant(QK_GATE_UP_ACT);
            break;
    }
    return a;
}

static void print_line(const Case &c, const Answer &a) {
    printf("%s : sup=%d ", case_text(c).c_str(), a.supported ? 1 : 0);
    if (!a.ok) {
        printf("invalid\n");
        return;
    }
    printf("cfg=%d,%d,%d,%d var=%s grid=%dx%d thr=%d lds=%d raise=%d", a.cfg.F, a.cfg.T16, a.cfg.D, a.cfg.NW, a.variant, a.launch.grid_x, a.launch.grid_y,
           a.launch.threads, a.launch.lds_bytes, a.launch.raise_to ? 1 : 0);
    if (a.quant) printf(" rows=%d early=%d", a.stage_rows, a.early);
    printf("\n");
}

// ---- the sweep of the fixture (256 CUs): both sides of every threshold of the ladders and the predicates ----
// slabs: 1, 4, 32 (three segments), 33, 112 (three segments); then K around two_tile_fits(3, .), two_tile_fits(2, .) and the one-tile bounds
static const int LIST_KS[][3] = {{0, 0, 128},   {0, 0, 512},   {2048, 128, 1920}, {0, 0, 4224},  {1024, 1024, 12288}, {0, 0, 26624}, {0, 0, 26752},
                                 {0, 0, 53248}, {0, 0, 53376}, {0, 0, 65536},     {0, 0, 65664}, {0, 0, 90112},       {0, 0, 90240}};
static Case make(CaseKind kind, int M, int N, const int K[3], int w4, int groups = 0, int rows = 0, int norm = 0, const char *ov = "") {
    Case c = {};
    c.kind = kind, c.M = M, c.N = N, c.w4 = w4, c.groups = groups, c.rows = rows, c.norm = norm, c.ov_text = ov;
    for (int g = 0; g < 3; ++g) c.K[g] = K[g];
    if (ov[0] && !set_override(c.ov, ov)) abort();
    return c;
}
static std::vector<Case> fixture_sweep() {
    std::vector<Case> out;
    auto in = [](int v, std::initializer_list<int> set) { return std::find(set.begin(), set.end(), v) != set.end(); };
    // The whole grid at 32 slabs (LIST_KS[2]); the other slab counts where they decide something: K of 1 / 4 / 33 / 112 slabs at the
    // tier edges, the long K (index 5 on) at the tiers whose predicates depend on it.
    int ki = -1;
    for (const auto &K : LIST_KS) {
        const bool full = ++ki == 2, lng = ki >= 5;
        for (int w4 = 0; w4 < 2; ++w4) {
            // N / 32 against 256 and 512 workgroups, N / 16 against 256 (the plain predicate at M <= 8), one block either side; 264: a ragged last block
            for (int N : {264, 4096, 4097, 8160, 8192, 16384, 16416})
                for (int M : {1, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65}) {
                    if (lng ? !(in(M, {16, 17, 32}) && in(N, {4097, 16416})) : !full && !(in(M, {8, 9, 16, 17, 33, 64}) && in(N, {4096, 8192, 16416}))) continue;
                    out.push_back(make(C_PLAIN, M, N, K, w4));
                }
            // grouped: N / 32 x groups against 256
            for (int M : {1, 16, 17, 32, 33, 48, 49, 64, 65})
                for (int NG : {1024 * 100 + 7, 1024 * 100 + 8, 1056 * 100 + 8, 4096 * 100 + 1, 8192 * 100 + 1, 264 * 100 + 9}) {
                    if (!full && !(in(M, lng ? std::initializer_list<int>{16, 17, 32} : std::initializer_list<int>{16, 17, 48, 64}) && NG / 100 == 1024)) continue;
                    out.push_back(make(C_GROUPED, M, NG / 100, K, w4, NG % 100));
                }
            // device-sized: the tier from min(max_rows, 64), the groups min(E, rows, 8): 8 x 32 = 256, 8 x 31, 5 x 32, 5 x 64
            for (int R : {1, 16, 17, 32, 33, 48, 49, 64, 65, 200})
                for (int ENN : {8 * 10000000 + 771 * 10000 + 1024, 8 * 10000000 + 771 * 10000 + 992, 64 * 10000000 + 5 * 10000 + 1024, 8 * 10000000 + 5 * 10000 + 2048}) {
                    if (!full && !(in(R, lng ? std::initializer_list<int>{16, 17, 32} : std::initializer_list<int>{16, 17, 64}) && ENN / 10000000 == 8 && ENN / 10000 % 1000 == 771)) continue;
                    out.push_back(make(C_MOE, R, ENN % 10000, K, w4, ENN / 10000000, ENN / 10000 % 1000));
                }
        }
    }
    for (int M : {1, 16, 64}) out.push_back(make(C_PLAIN, M, 8192, LIST_KS[2], 1, 0, 0, 0, "MICROMIX_STREAM=0"));
    for (const char *ov : {"MICROMIX_STREAM_GROUPED=0", "MICROMIX_STREAM_GROUPED_MAX_M=32"})
        for (int M : {16, 32, 33, 64}) {
            out.push_back(make(C_GROUPED, M, 1024, LIST_KS[2], 1, 8, 0, 0, ov));
            out.push_back(make(C_MOE, M, 1024, LIST_KS[2], 1, 8, 771, 0, ov));
        }
    // the quantizing launches: every override value; K to the norm's bound (8192 | 8320) and the staging bounds (one row of K = 16384 is 32 KB of bf16)
    const int QKS[][3] = {{0, 0, 512}, {2048, 128, 1920}, {0, 0, 4224}, {0, 0, 8320}, {1024, 1024, 12288}, {0, 0, 16384}, {0, 0, 65536}};
    const char *const QOVS[] = {"", "MICROMIX_DECODE_STREAM=0", "MICROMIX_DECODE_STREAM=2", "MICROMIX_DECODE_EARLY=0", "MICROMIX_DECODE_F4=-1", "MICROMIX_DECODE_F4=2",
                                "MICROMIX_DECODE_F4=3", "MICROMIX_DECODE_F4=4", "MICROMIX_DECODE_DEPTH=3", "MICROMIX_DECODE_DEPTH=4"};
    for (const char *ov : QOVS) {
        ki = -1;
        for (const auto &K : QKS) {
            ++ki;
            for (int w4 = 0; w4 < 2; ++w4)
                for (int N : {8160, 8192, 16384, 16416})
                    for (int M : {1, 4, 5, 8})
                        for (int norm = 0; norm < 3; ++norm) {
                            if ((N == 8160 || N == 16384 || norm == 2) && (M != 1 || (norm && N != 8192))) continue;     // (not wide, exactly two rounds, the add: at M = 1)
                            if (!in(ki, {1, 4, 6}) && (!w4 || M == 4 || M == 5)) continue;      // (matching-precision weights and M = 4 | 5 at three of the K)
                            if (ov[0] && (in(M, {4, 5}) || !in(N, {8192, 16416}) || norm == 2 || (norm && M != 1) || !in(ki, {1, 4}))) continue;      // (the overrides on a thinner grid)
                            out.push_back(make(C_QLINEAR, M, N, K, w4, 0, 0, norm, ov));
                        }
        }
    }
    for (const auto &K : QKS)
        for (int w4 = 0; w4 < 2; ++w4)
            for (int N : {8160, 8192})
                for (int M : {1, 4, 5})
                    if (w4 || K[0]) out.push_back(make(C_DOWN, M, N, K, w4));      // (matching-precision weights at the two three-segment K)
    // the fused gate | up launches: N / 64 against 256, N a multiple of 256
    ki = -1;
    for (const auto &K : LIST_KS) {
        const bool full = ++ki == 2;
        for (int N : {16128, 16384, 16400, 28672})
            for (int M : {1, 16, 17, 32, 33}) {
                if (N == 16400 ? !(full && M == 16) : !full && !(in(M, {16, 17}) && N == 16384)) continue;
                out.push_back(make(C_ACT, M, N, K, 1));
            }
    }
    out.push_back(make(C_ACT, 16, 28672, LIST_KS[2], 1, 0, 0, 0, "MICROMIX_GATE_UP_ACT_STREAM=0"));
    for (const char *ov : {"", "MICROMIX_GATE_UP_ACT_STREAM=0", "MICROMIX_DECODE_EARLY=0"})
        for (const auto &K : QKS)
            for (int N : {16128, 16384, 28672})
                for (int M : {1, 4, 5})
                    for (int norm = 0; norm < 3; ++norm) {
                        if ((N != 28672 && (M != 1 || norm)) || (ov[0] && (M != 1 || N != 28672 || norm == 2)) || (M != 1 && !K[0])) continue;
                        out.push_back(make(C_ACTQ, M, N, K, 1, 0, 0, norm, ov));
                    }
    return out;
}

// ---- the invariants ----
static void check_case(const Case &c, int cus) {
    const Answer a = answer(c, cus);
    struct What {      // (the text of a failure only)
        const Case &c;
        int cus;
        operator const char *() { return (text = case_text(c) + " @ " + std::to_string(cus) + " CUs").c_str(); }
        std::string text;
    } w{c, cus, {}};
    if (a.supported) EXPECT(a.ok, "%s: supported, and the launcher would refuse it", (const char *)w);
    if (!a.ok) return;
    const StreamKind list = c.kind == C_PLAIN ? SK_PLAIN : c.kind == C_GROUPED ? SK_GROUPED : c.kind == C_MOE ? SK_MOE : c.kind == C_ACT ? SK_ACT
                          : c.kind == C_ACTQ ? SK_QUANT_ACT : SK_QUANT;
    EXPECT(in_list(list, a.cfg, c.w4 != 0), "%s: configuration %d,%d,%d,%d is not in its kind's list", (const char *)w, a.cfg.F, a.cfg.T16, a.cfg.D, a.cfg.NW);
    EXPECT(a.launch.lds_bytes > 0 && (size_t)a.launch.lds_bytes <= (a.quant ? QUANT_LDS_WG : (size_t)STREAM_LDS_MAX), "%s: %d bytes of LDS", (const char *)w, a.launch.lds_bytes);
    EXPECT((a.launch.raise_to != 0) == (a.launch.lds_bytes > 65536) && a.launch.raise_to <= STREAM_LDS_MAX && (!a.launch.raise_to || a.launch.raise_to >= a.launch.lds_bytes),
           "%s: %d bytes of LDS with the limit at %d", (const char *)w, a.launch.lds_bytes, a.launch.raise_to);
    EXPECT(a.launch.threads == 64 * a.cfg.NW && a.launch.threads <= 1024, "%s: %d threads", (const char *)w, a.launch.threads);
    // the grid covers the N features exactly once: whole workgroups of 16 F rows, the last one ragged; the ACT launches 64 rows each
    const int bn = 16 * a.cfg.F;
    if (c.kind == C_ACT || c.kind == C_ACTQ) {
        if (a.supported) EXPECT(a.launch.grid_x * 64 == c.N, "%s: %d workgroups of 64 rows", (const char *)w, a.launch.grid_x);
    } else {
        EXPECT(a.launch.grid_x * bn >= c.N && (a.launch.grid_x - 1) * bn < c.N, "%s: %d workgroups of %d features", (const char *)w, a.launch.grid_x, bn);
    }
    EXPECT(a.launch.grid_y == (c.kind == C_GROUPED || c.kind == C_MOE ? c.groups : 1), "%s: grid y %d", (const char *)w, a.launch.grid_y);
    if (!a.quant) EXPECT(16 * a.cfg.T16 >= (c.kind == C_MOE ? moe_rows(c.M) : c.M) || !a.supported, "%s: %d token tiles", (const char *)w, a.cfg.T16);
    if (a.quant) {
        const size_t Kt = (size_t)c.K[0] + c.K[1] + c.K[2];
        if (c.kind != C_DOWN) EXPECT(a.stage_rows >= 1 && a.stage_rows <= c.M, "%s: %d staged rows", (const char *)w, a.stage_rows);
        else EXPECT(a.stage_rows == 0, "%s: %d staged rows in mode 1", (const char *)w, a.stage_rows);
        EXPECT((size_t)a.qbytes == (size_t)a.stage_rows * Kt * 2 + quant_operand_bytes(c.M, c.K, c.norm != 0) && a.qbytes % 16 == 0 && a.qbytes < a.launch.lds_bytes,
               "%s: qbytes %d", (const char *)w, a.qbytes);
        if (a.early && c.kind != C_DOWN) EXPECT(a.stage_rows == c.M && c.ov.decode_early, "%s: early with %d of %d rows staged", (const char *)w, a.stage_rows, c.M);
        // (ACT: the fp6 group buffer lies in the staged rows' range)
        if (c.kind == C_ACTQ && a.supported) EXPECT((size_t)a.stage_rows * Kt * 2 >= (size_t)ACT_GROUP_BYTES, "%s: no room for the group buffer", (const char *)w);
        if (c.norm) EXPECT(has_norm_kernel(a.cfg), "%s: no norm kernel", (const char *)w);
    }
}

static long long check_invariants() {
    long long cases = 0;
    const int cu_counts[] = {1, 2, 8, 64, 80, 228, 255, 256, 257, 304, 512, 1024};
    const int IKS[][3] = {{0, 0, 128},   {0, 0, 384},   {128, 128, 128}, {0, 0, 512},   {0, 0, 640},   {2048, 128, 1920}, {0, 0, 4224},  {0, 4096, 0},  {4096, 4096, 0},
                          {0, 0, 8192},  {0, 0, 8320},  {1024, 1024, 12288}, {0, 0, 16384}, {0, 0, 26624}, {0, 0, 26752}, {0, 0, 28672}, {0, 0, 43008}, {0, 0, 45056},
                          {0, 0, 53248}, {0, 0, 53376}, {0, 0, 65536},   {0, 0, 65664}, {0, 0, 90112}, {0, 0, 90240}, {16384, 16384, 98304}, {0, 0, 1 << 20}};
    const char *const GOVS[] = {"", "MICROMIX_STREAM=0", "MICROMIX_STREAM_GROUPED=0", "MICROMIX_STREAM_GROUPED_MAX_M=32", "MICROMIX_STREAM_GROUPED_MAX_M=100"};
    const char *const QOVS[] = {"", "MICROMIX_DECODE_STREAM=0", "MICROMIX_DECODE_STREAM=2", "MICROMIX_DECODE_EARLY=0", "MICROMIX_DECODE_F4=-1", "MICROMIX_DECODE_F4=2",
                                "MICROMIX_DECODE_F4=3", "MICROMIX_DECODE_F4=4", "MICROMIX_DECODE_DEPTH=3", "MICROMIX_DECODE_DEPTH=4", "MICROMIX_GATE_UP_ACT_STREAM=0"};
    for (int cus : cu_counts) {
        // N around every threshold: ceil(N / 16), ceil(N / 32) and ceil(N / 64) against cus and 2 cus, one block either side
        std::vector<int> Ns = {1, 16, 17, 264};
        for (int bn : {16, 32, 64})
            for (int mult : {1, 2})
                for (int d : {-1, 0, 1})
                    if ((cus * mult + d) > 0) Ns.push_back((cus * mult + d) * bn), Ns.push_back((cus * mult + d) * bn - bn + 1);
        std::sort(Ns.begin(), Ns.end());
        Ns.erase(std::unique(Ns.begin(), Ns.end()), Ns.end());
        for (const auto &K : IKS)
            for (int w4 = 0; w4 < 2; ++w4)
                for (int N : Ns) {
                    for (const char *ov : GOVS) {
                        for (int M = 1; M <= 65; ++M) {
                            if (ov[0] && M % 16 > 1) continue;      // (the overrides at the tier edges only)
                            check_case(make(C_PLAIN, M, N, K, w4, 0, 0, 0, ov), cus), ++cases;
                            for (int G = 1; G <= MAX_GROUPS + 1; ++G) {
                                if ((M % 16 > 1 || ov[0]) && G != 1 && G != MAX_GROUPS) continue;
                                check_case(make(C_GROUPED, M, N, K, w4, G, 0, 0, ov), cus), ++cases;
                                check_case(make(C_MOE, M, N, K, w4, G, 3, 0, ov), cus);
                                check_case(make(C_MOE, M + 100, N, K, w4, 8 * G, 771, 0, ov), cus), cases += 2;
                            }
                        }
                        // the property mx_gemm_stream_moe_supported's comment promises: every 16-row tier below a supported max_m is supported
                        Case c = make(C_MOE, 0, N, K, w4, 8, 771, 0, ov);
                        for (int R = 1; R <= 80; ++R)
                            if (moe_supported(R, K, c.ov))
                                for (int tier = 16; tier < moe_rows(R); tier += 16)
                                    EXPECT(grouped_supported(tier, 1, N, K, [cus] { return cus; }, c.ov) && grouped_supported(tier, MAX_GROUPS, N, K, [cus] { return cus; }, c.ov), "moe_supported(%d) without the %d-row tier (K %d,%d,%d %s)", R, tier, K[0], K[1], K[2], ov);
                    }
                    // the three GEMM kinds pick the same configuration for the same (M tier, wide, slabs, weight mode), the two plain-only rules aside
                    const StreamOverrides dflt;
                    for (int M = 1; M <= 64; ++M)
                        for (int G : {1, 3, MAX_GROUPS}) {
                            const int NG = (N + 31) / 32 * 32 * G;        // a plain launch with as many 32-feature workgroups as the G groups have
                            const StreamCfg p = select_gemm(SK_PLAIN, M, NG, K, w4 != 0, 1, cus, dflt), g = select_gemm(SK_GROUPED, M, N, K, w4 != 0, G, cus, dflt),
                                            m = select_gemm(SK_MOE, M, N, K, w4 != 0, G, cus, dflt);
                            const bool plain_only = M <= 16 && (NG / 32 > 2 * cus || (NG / 32 < cus && slabs_of(K) <= 32));
                            EXPECT(g == m, "grouped and device-sized differ: M %d N %d G %d", M, N, G);
                            if (!plain_only) EXPECT(p == g, "plain %d,%d,%d,%d, grouped %d,%d,%d,%d: M %d N %d G %d cus %d", p.F, p.T16, p.D, p.NW, g.F, g.T16, g.D, g.NW, M, N, G, cus);
                            else EXPECT(p == (NG / 32 > 2 * cus ? StreamCfg{4, 1, 2, 4} : StreamCfg{1, 1, 4, 8}) && g.T16 == 1, "the plain-only rules: M %d N %d", M, N);
                        }
                    for (const char *ov : QOVS)
                        for (int M = 1; M <= 9; ++M) {
                            if (ov[0] && M != 1 && M != 4 && M != 5 && M != 8) continue;
                            for (int norm = 0; norm < 3; ++norm) {
                                check_case(make(C_QLINEAR, M, N, K, w4, 0, 0, norm, ov), cus), ++cases;
                                if (w4) check_case(make(C_ACTQ, M, N, K, 1, 0, 0, norm, ov), cus), ++cases;
                            }
                            check_case(make(C_DOWN, M, N, K, w4, 0, 0, 0, ov), cus), ++cases;
                        }
                    if (w4)
                        for (int M = 1; M <= 33; ++M) check_case(make(C_ACT, M, N, K, 1, 0, 0, 0, M & 1 ? "" : "MICROMIX_GATE_UP_ACT_STREAM=0"), cus), ++cases;
                }
    }
    // every row of every list is a configuration its kernel accepts (stream_body's static_asserts, restated)
    for (StreamKind kind : {SK_PLAIN, SK_GROUPED, SK_MOE, SK_ACT, SK_QUANT, SK_QUANT_ACT})
        for (int F : {1, 2, 4})
            for (int T16 = 1; T16 <= 4; ++T16)
                for (int D = 1; D <= 6; ++D)
                    for (int NW : {4, 8, 16})
                        for (int w4 = 0; w4 < 2; ++w4)
                            if (in_list(kind, StreamCfg{F, T16, D, NW}, w4 != 0)) {
                                const bool quant = kind == SK_QUANT || kind == SK_QUANT_ACT;
                                const int loads = F * (w4 ? 1 : 2) + (quant ? 0 : T16) + (quant || scale_images_for(T16, w4 != 0) ? 0 : 2);
                                EXPECT((D - 1) * loads < 64 && 12 * F * T16 <= 192 && (!quant || T16 == 1), "list %d holds %d,%d,%d,%d", kind, F, T16, D, NW);
                            }
    return cases;
}

int main(int argc, char **argv) {
    int cus = 256;
    if (argc >= 2 && !strcmp(argv[1], "--list")) {
        for (const Case &c : fixture_sweep()) print_line(c, answer(c, cus));
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "--cases")) {      // the sweep's cases alone
        for (const Case &c : fixture_sweep()) printf("%s\n", case_text(c).c_str());
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
            print_line(c, answer(c, cus));
        }
        return 0;
    }
    const long long cases = check_invariants();
    printf("%lld cases checked; %lld failures\n", cases, failures);
    return failures ? 1 : 0;
}
