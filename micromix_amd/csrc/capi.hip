// extern "C" surface of libmicromix_hip.so -- see include/micromix_hip.h.
#include "../../include/micromix_hip.h"
#include "../../include/micromix_calib.h"
#include "../../include/micromix_logprob.h"
#include "../../include/micromix_logits.h"
#include "../../include/micromix_spec.h"
#include "../../include/micromix_kvstep.h"
#include "../../include/micromix_tokens.h"
#include "../../include/micromix_random.h"
#include "mx_common.h"
#include "mx_kernels.h"
#include "mx_kv_shared_host.h"

#include <stdio.h>
#include <string.h>


static thread_local char g_last_error[256] = "";
// measurement hooks, per calling thread (see mm_diag_set_kernel_events / mm_diag_set_clock_buffer in the header)
static thread_local mm::DiagEvents g_ev = {nullptr, nullptr};
namespace mm { DiagEvents &diag_events() { return g_ev; } }
static thread_local unsigned long long *g_clock_buf = nullptr;

static int fail_hip(hipError_t e, const char *where) {
    snprintf(g_last_error, sizeof(g_last_error), "%s: %s", where, hipGetErrorString(e));
    return MM_ERR_LAUNCH;
}

// The weight mode a launch really runs in: MM_W_FP4 as given; MM_W_MATCH with KS = KO = 0 has only the N segment, whose weights are
// fp4 in both modes, so it takes the fp4-weight kernels too (the matching-precision 256 x 256 kernel sits at its register limit).
static bool weights_fp4(int wmode, int KS, int KO) { return wmode == MM_W_FP4 || (KS == 0 && KO == 0); }

// a decode split is well-formed: three non-negative multiples of 128, not all zero
static bool decode_split_ok(const int K[3]) {
    return K[0] >= 0 && K[1] >= 0 && K[2] >= 0 && (K[0] % 128) == 0 && (K[1] % 128) == 0 && (K[2] % 128) == 0 && K[0] + K[1] + K[2] > 0;
}

// ... and adds up to a K given separately
static bool split_ok(int K, int KN, int KS, int KO) {
    const int Kseg[3] = {KN, KS, KO};
    return decode_split_ok(Kseg) && KN + KS + KO == K;
}

// every non-empty segment has its data and its scale pointer
struct Ptr3 { const uint8_t *p[3]; };
static bool segments_ok(const int K[3], const Ptr3 &data, const Ptr3 &sf) {
    return !((K[0] && (!data.p[0] || !sf.p[0])) || (K[1] && (!data.p[1] || !sf.p[1])) || (K[2] && (!data.p[2] || !sf.p[2])));
}

// which of its extern "C" entries a shared body serves: the pointers cannot tell (a null norm weight is an error of the norm entries)
enum Variant { PLAIN, NORM, ADD_NORM };

extern "C" {

int mm_version(void) { return 660; /* 0.6.6: + mm_add_rmsnorm_quantize, mm_add_rmsnorm_qlinear_decode, mm_add_rmsnorm_gate_up_activate_decode (the residual add in front of the norm, s = x + r, computed while the quantizer stages the row; s leaves as the new residual stream); 0.6.5: + mm_moe_activate_quantize (silu(a) * b computed while the expert quantizer stages the row: the activation of a capturable MoE block in one launch); 0.6.4: + mm_moe_quantize, mm_moe_matmul(_supported), mm_moe_sf_bytes (device-sized grouped launches: a hipGraph-capturable MoE block); 0.6.3: + mm_moe_route, mm_moe_plan, mm_moe_gather, mm_moe_combine (top-k routing, dispatch and combine of a sparse MoE block around mm_matmul_grouped); 0.6.2: + mm_rope_kv_append (RoPE + paged KV append in one launch, from the packed q | k | v projection); 0.6.1: + mm_paged_prefill(_workspace_bytes) (causal multi-token attention over the paged KV cache); 0.6.0: + mm_kv_append, mm_paged_decode(_workspace_bytes), enum mm_kv_dtype (paged int4 / bf16 KV cache); 0.5.1: + mm_rmsnorm_gate_up_activate_decode(_supported), mm_gate_up_activate_decode_supported; mm_gate_up_activate(_decode) one launch at decode sizes; 0.5.0: + the *_supported_w queries (weight mode); 0.4.0: + mm_rmsnorm_qlinear_decode(_supported) (0.3.0: + mm_gate_up_activate(_decode), mm_down_activate_decode, mm_matmul_ws_reset; 0.2.0: diagnostics moved to libmicromix_diag.so, + mm_test_function) */ }

const char *mm_test_function(void) { return "Hello from test_function!"; /* bindings.cpp:700 */ }

const char *mm_strerror(int status) {
    switch (status) {
        case MM_OK: return "ok";
        case MM_ERR_BAD_SPLIT: return "KN, KS, KO must be non-negative multiples of 128 that sum to K";
        case MM_ERR_BAD_ARG: return "bad argument";
        case MM_ERR_LAUNCH: return "HIP error";
        case MM_ERR_UNSUPPORTED: return "unsupported configuration";
        case MM_ERR_NO_DEVICE: return "no gfx950 device";
        default: return "unknown status";
    }
}

const char *mm_last_error(void) { return g_last_error; }

size_t mm_sf_bytes_x(int M, int Kseg) { return (size_t)(M / 128 + 1) * 128u * (size_t)(Kseg / 32); }
size_t mm_sf_bytes_w(int N, int Kseg) { return (size_t)((N + 127) / 128) * 128u * (size_t)(Kseg / 32); }
size_t mm_sf_offset(int row, int block, int Kseg) { return mm::sf_offset(row, block, Kseg); }

int mm_reorder_quantize(const void *src_bf16, int rows, int K, const int16_t *reorder_index, int KN, int KS, int KO,
                        int mode, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO,
                        mm_stream_t stream) {
    if (!split_ok(K, KN, KS, KO)) return MM_ERR_BAD_SPLIT;
    if (rows < 0 || K > 32768 || (mode != MM_QUANT_MIXED && mode != MM_QUANT_W4)) return MM_ERR_BAD_ARG;
    if (rows == 0) return MM_OK;
    if (!src_bf16 || !reorder_index) return MM_ERR_BAD_ARG;
    const int Kseg[3] = {KN, KS, KO};
    if (!segments_ok(Kseg, {oN, oS, oO}, {sfN, sfS, sfO})) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_reorder_quantize(src_bf16, rows, K, reorder_index, KN, KS, KO, mode == MM_QUANT_W4, oN, oS,
                                               oO, sfN, sfS, sfO, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_reorder_quantize");
}

int mm_reorder_quantize_gather(const void *src_bf16, int rows, int K_in, const int16_t *index, int KN, int KS, int KO,
                               int mode, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO,
                               mm_stream_t stream) {
    if (!split_ok(KN + KS + KO, KN, KS, KO) || K_in <= 0 || (K_in % 128) || KN + KS + KO > K_in) return MM_ERR_BAD_SPLIT;
    if (rows < 0 || K_in > 32768 || (mode != MM_QUANT_MIXED && mode != MM_QUANT_W4)) return MM_ERR_BAD_ARG;
    if (rows == 0) return MM_OK;
    if (!src_bf16 || !index) return MM_ERR_BAD_ARG;
    const int Kseg[3] = {KN, KS, KO};
    if (!segments_ok(Kseg, {oN, oS, oO}, {sfN, sfS, sfO})) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_reorder_quantize(src_bf16, rows, K_in, index, KN, KS, KO, mode == MM_QUANT_W4, oN, oS, oO,
                                               sfN, sfS, sfO, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_reorder_quantize_gather");
}

int mm_activate_quantize(const void *A_bf16, const void *B_bf16, int rows, int KN, int KS, int KO, uint8_t *oN, uint8_t *oS,
                         uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, mm_stream_t stream) {
    if (!split_ok(KN + KS + KO, KN, KS, KO)) return MM_ERR_BAD_SPLIT;
    if (rows < 0) return MM_ERR_BAD_ARG;
    if (rows == 0) return MM_OK;
    if (!A_bf16 || !B_bf16) return MM_ERR_BAD_ARG;
    const int Kseg[3] = {KN, KS, KO};
    if (!segments_ok(Kseg, {oN, oS, oO}, {sfN, sfS, sfO})) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_direct_quantize(A_bf16, B_bf16, rows, KN, KS, KO, 0, oN, oS, oO, sfN, sfS, sfO, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_activate_quantize");
}

int mm_downproj_quantize(const void *W_bf16, int rows, int KN, int KS, int KO, int mode, uint8_t *oN, uint8_t *oS, uint8_t *oO,
                         uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, mm_stream_t stream) {
    if (!split_ok(KN + KS + KO, KN, KS, KO)) return MM_ERR_BAD_SPLIT;
    if (rows < 0 || (mode != MM_QUANT_MIXED && mode != MM_QUANT_W4)) return MM_ERR_BAD_ARG;
    if (rows == 0) return MM_OK;
    if (!W_bf16) return MM_ERR_BAD_ARG;
    const int Kseg[3] = {KN, KS, KO};
    if (!segments_ok(Kseg, {oN, oS, oO}, {sfN, sfS, sfO})) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_direct_quantize(W_bf16, nullptr, rows, KN, KS, KO, mode == MM_QUANT_W4 ? 2 : 1, oN, oS, oO, sfN, sfS,
                                              sfO, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_downproj_quantize");
}

// [a, a + na) and [b, b + nb) share a byte
static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// S_out of the add_ entries: non-null, 16-byte aligned like R, and clear of X and R -- every workgroup of the decode launches re-reads
// both while workgroup 0 writes S_out, so an in-place update would race
static bool residual_ok(const void *X, const void *R, const void *S_out, int M, int K) {
    if (!R || !S_out || ((uintptr_t)R & 15) || ((uintptr_t)S_out & 15)) return false;
    const size_t bytes = (size_t)M * (size_t)K * 2u;
    return !ranges_overlap(S_out, bytes, X, bytes) && !ranges_overlap(S_out, bytes, R, bytes);
}

// mm_rmsnorm_quantize (NORM) and mm_add_rmsnorm_quantize (ADD_NORM)
static int rmsnorm_quantize_entry(Variant v, const void *X_bf16, const void *R_bf16, void *S_out_bf16, const void *W_bf16, float eps, int rows, int K,
                                  const int16_t *reorder_index, int KN, int KS, int KO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO,
                                  uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, mm_stream_t stream) {
    if (!split_ok(K, KN, KS, KO)) return MM_ERR_BAD_SPLIT;
    if (rows < 0 || K > 32768) return MM_ERR_BAD_ARG;
    if (rows == 0) return MM_OK;
    if (!X_bf16 || !W_bf16 || !reorder_index) return MM_ERR_BAD_ARG;
    const int Kseg[3] = {KN, KS, KO};
    if (!segments_ok(Kseg, {oN, oS, oO}, {sfN, sfS, sfO})) return MM_ERR_BAD_ARG;
    const bool int_round = !(flags & MM_RMS_NO_INTEGER_ROUND);
    if (v == NORM) {    // (mm_rmsnorm_quantize asks no alignment of X and W)
        hipError_t e = mm::launch_rmsnorm_quantize(X_bf16, W_bf16, eps, rows, K, reorder_index, KN, KS, KO, int_round, oN, oS, oO, sfN, sfS, sfO,
                                                   (hipStream_t)stream);
        return e == hipSuccess ? MM_OK : fail_hip(e, "mm_rmsnorm_quantize");
    }
    // rows travel in 16-byte pieces; K % 128 == 0 keeps every row of an aligned tensor aligned
    if (((uintptr_t)X_bf16 & 15) || ((uintptr_t)W_bf16 & 15) || !residual_ok(X_bf16, R_bf16, S_out_bf16, rows, K)) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_add_rmsnorm_quantize(X_bf16, R_bf16, S_out_bf16, W_bf16, eps, rows, K, reorder_index, KN, KS, KO, int_round, oN, oS, oO,
                                                   sfN, sfS, sfO, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_add_rmsnorm_quantize");
}

int mm_rmsnorm_quantize(const void *X_bf16, const void *W_bf16, float eps, int rows, int K, const int16_t *reorder_index, int KN,
                        int KS, int KO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS,
                        uint8_t *sfO, mm_stream_t stream) {
    return rmsnorm_quantize_entry(NORM, X_bf16, nullptr, nullptr, W_bf16, eps, rows, K, reorder_index, KN, KS, KO, flags, oN, oS, oO, sfN, sfS, sfO,
                                  stream);
}

int mm_add_rmsnorm_quantize(const void *X_bf16, const void *R_bf16, void *S_out_bf16, const void *W_bf16, float eps, int rows, int K,
                            const int16_t *reorder_index, int KN, int KS, int KO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO,
                            uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, mm_stream_t stream) {
    return rmsnorm_quantize_entry(ADD_NORM, X_bf16, R_bf16, S_out_bf16, W_bf16, eps, rows, K, reorder_index, KN, KS, KO, flags, oN, oS, oO, sfN, sfS,
                                  sfO, stream);
}

// (the five-argument queries answer for the matching-precision weight mode, whose ring / reduction tail is the larger one: what they
// accept launches in either mode; the _w forms take the weight mode and accept the long-K fp4 shapes the 48 KB tail leaves room for)
static int decode_supported_w(int M, int N, int KN, int KS, int KO, int wmode, bool rms) {
    const int K[3] = {KN, KS, KO};
    if (N < 0 || !decode_split_ok(K) || KN + KS + KO > 32768) return 0;
    if (wmode != MM_W_MATCH && wmode != MM_W_FP4) return 0;
    return mm::qlinear_decode_supported(M, N, K, rms, weights_fp4(wmode, KS, KO));
}
int mm_qlinear_decode_supported_w(int M, int N, int KN, int KS, int KO, int wmode) { return decode_supported_w(M, N, KN, KS, KO, wmode, false); }
int mm_qlinear_decode_supported(int M, int N, int KN, int KS, int KO) { return decode_supported_w(M, N, KN, KS, KO, (KS | KO) ? MM_W_MATCH : MM_W_FP4, false); }
int mm_rmsnorm_qlinear_decode_supported_w(int M, int N, int KN, int KS, int KO, int wmode) { return decode_supported_w(M, N, KN, KS, KO, wmode, true); }
int mm_rmsnorm_qlinear_decode_supported(int M, int N, int KN, int KS, int KO) { return decode_supported_w(M, N, KN, KS, KO, (KS | KO) ? MM_W_MATCH : MM_W_FP4, true); }

static mm::NormArgs norm_args(const void *weight, float eps, int flags, const void *res = nullptr, void *s_out = nullptr) {
    return {weight, eps, (flags & MM_NORM_NO_INTEGER_ROUND) ? 0 : 1, res, s_out};
}

// mm_qlinear_decode (PLAIN, norm = mm::NO_NORM), mm_rmsnorm_qlinear_decode (NORM) and mm_add_rmsnorm_qlinear_decode (ADD_NORM: norm.res / norm.s_out)
static int qlinear_decode_entry(Variant v, const void *X_bf16, const mm::NormArgs &norm, const int16_t *reorder_index, const Ptr3 &B, const Ptr3 &SFB,
                                int M, int N, int KN, int KS, int KO, int wmode, int flags, const void *bias_bf16, void *D_bf16, mm_stream_t stream) {
    static const char *const name[] = {"mm_qlinear_decode", "mm_rmsnorm_qlinear_decode", "mm_add_rmsnorm_qlinear_decode"};
    const int K[3] = {KN, KS, KO};
    if (M < 0 || N < 0 || KN < 0 || KS < 0 || KO < 0) return MM_ERR_BAD_ARG;
    if (!decode_split_ok(K)) return MM_ERR_BAD_SPLIT;
    if (wmode != MM_W_MATCH && wmode != MM_W_FP4) return MM_ERR_BAD_ARG;
    if (v == PLAIN) {   // mm_qlinear_decode: fp32 partial sums come from mm_matmul only; it ignores every other unknown bit
        if (flags & MM_OUT_F32) return MM_ERR_UNSUPPORTED;
    } else if (flags & ~(MM_ROUND_ONCE | MM_NORM_NO_INTEGER_ROUND)) return MM_ERR_BAD_ARG;     // the norm entries refuse any unknown bit
    if (M == 0 || N == 0) return MM_OK;
    if (!decode_supported_w(M, N, KN, KS, KO, wmode, v != PLAIN)) return MM_ERR_UNSUPPORTED;
    if (!X_bf16 || !reorder_index || !D_bf16) return MM_ERR_BAD_ARG;
    // the norm entries stage rows and weights in 16-byte pieces; mm_qlinear_decode asks no alignment of X
    if (v != PLAIN && (!norm.weight || ((uintptr_t)X_bf16 & 15) || ((uintptr_t)norm.weight & 15))) return MM_ERR_BAD_ARG;
    if (v == ADD_NORM && !residual_ok(X_bf16, norm.res, norm.s_out, M, KN + KS + KO)) return MM_ERR_BAD_ARG;
    if (!segments_ok(K, B, SFB)) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_qlinear_decode(X_bf16, reorder_index, B.p, SFB.p, M, N, K, weights_fp4(wmode, KS, KO), (flags & MM_ROUND_ONCE) ? 0 : 1,
                                             bias_bf16, D_bf16, (hipStream_t)stream, norm);
    return e == hipSuccess ? MM_OK : fail_hip(e, name[v]);
}

int mm_qlinear_decode(const void *X_bf16, const int16_t *reorder_index, const uint8_t *BN, const uint8_t *BS, const uint8_t *BO,
                      const uint8_t *SFBN, const uint8_t *SFBS, const uint8_t *SFBO, int M, int N, int KN, int KS, int KO,
                      int wmode, int flags, const void *bias_bf16, void *D_bf16, mm_stream_t stream) {
    return qlinear_decode_entry(PLAIN, X_bf16, mm::NO_NORM, reorder_index, {BN, BS, BO}, {SFBN, SFBS, SFBO}, M, N, KN, KS, KO, wmode, flags, bias_bf16,
                                D_bf16, stream);
}

int mm_rmsnorm_qlinear_decode(const void *X_bf16, const void *norm_weight_bf16, float eps, const int16_t *reorder_index, const uint8_t *BN,
                              const uint8_t *BS, const uint8_t *BO, const uint8_t *SFBN, const uint8_t *SFBS, const uint8_t *SFBO, int M, int N,
                              int KN, int KS, int KO, int wmode, int flags, const void *bias_bf16, void *D_bf16, mm_stream_t stream) {
    return qlinear_decode_entry(NORM, X_bf16, norm_args(norm_weight_bf16, eps, flags), reorder_index, {BN, BS, BO}, {SFBN, SFBS, SFBO}, M, N, KN, KS, KO,
                                wmode, flags, bias_bf16, D_bf16, stream);
}

int mm_add_rmsnorm_qlinear_decode(const void *X_bf16, const void *R_bf16, void *S_out_bf16, const void *norm_weight_bf16, float eps,
                                  const int16_t *reorder_index, const uint8_t *BN, const uint8_t *BS, const uint8_t *BO, const uint8_t *SFBN,
                                  const uint8_t *SFBS, const uint8_t *SFBO, int M, int N, int KN, int KS, int KO, int wmode, int flags,
                                  const void *bias_bf16, void *D_bf16, mm_stream_t stream) {
    return qlinear_decode_entry(ADD_NORM, X_bf16, norm_args(norm_weight_bf16, eps, flags, R_bf16, S_out_bf16), reorder_index, {BN, BS, BO},
                                {SFBN, SFBS, SFBO}, M, N, KN, KS, KO, wmode, flags, bias_bf16, D_bf16, stream);
}

// The one place a GemmArgs is made: operands, shapes and flags.  Everything else starts at zero -- no workspace (mm_matmul_ws adds its
// own), no fused epilogue (gemm_args_act adds it); the launchers fill in splits, tickets and tile columns.  X / SFX: null where the launch
// quantizes its own rows.  M = 0: a device-sized grouped launch (every workgroup reads its group's rows).  hooks: the launch carries the
// calling thread's diagnostics hooks (mm_diag_set_kernel_events / mm_diag_set_clock_buffer).
static mm::GemmArgs gemm_args(const Ptr3 &X, const Ptr3 &SFX, const Ptr3 &W, const Ptr3 &SFW, int M, int N, const int K[3], int flags,
                              const void *bias_bf16, void *D, bool hooks) {
    mm::GemmArgs a = {};
    for (int i = 0; i < 3; ++i) {
        a.X[i] = X.p[i];
        a.W[i] = W.p[i];
        a.SFX[i] = SFX.p[i];
        a.SFW[i] = SFW.p[i];
        a.K[i] = K[i];
    }
    a.M = M;
    a.N = N;
    // the 128-row tiles that hold scales of real rows.  The reference allocates M/128 + 1 tiles (bindings.cpp:120) and never
    // writes the last one when M % 128 == 0; counting only the written tiles keeps every kernel's scale reads inside ANY tensor
    // that holds the scales of its M rows, whoever allocated it.
    a.sfx_row_tiles = (M + 127) / 128;
    a.sfw_row_tiles = (N + 127) / 128;
    a.round_per_segment = (flags & MM_ROUND_ONCE) ? 0 : 1;
    a.bias = (const uint16_t *)bias_bf16;
    a.D = (uint16_t *)D;
    a.out_f32 = (flags & MM_OUT_F32) ? 1 : 0;
    if (hooks) {
        a.clock_out = g_clock_buf;
        a.ev_start = g_ev.start;
        a.ev_stop = g_ev.stop;
    }
    return a;
}
// ... with the fused gate / up epilogue (GemmArgs::act): N = 2 I interleaved rows, no D; Kd, o, sf: the consumer GEMM's operand
struct Out3 { uint8_t *p[3]; };
static mm::GemmArgs gemm_args_act(const Ptr3 &X, const Ptr3 &SFX, const Ptr3 &W, const Ptr3 &SFW, int M, int I, const int K[3], int flags,
                                  const int Kd[3], const Out3 &o, const Out3 &sf, bool hooks) {
    mm::GemmArgs a = gemm_args(X, SFX, W, SFW, M, 2 * I, K, flags, nullptr, nullptr, hooks);
    a.act = 1;
    for (int i = 0; i < 3; ++i) {
        a.act_K[i] = Kd[i];
        a.act_o[i] = o.p[i];
        a.act_sf[i] = sf.p[i];
    }
    return a;
}

size_t mm_matmul_workspace_bytes(int M, int N, int KN, int KS, int KO, int wmode, int flags) {
    if (M <= 0 || N <= 0 || KN < 0 || KS < 0 || KO < 0 || (KN % 128) || (KS % 128) || (KO % 128)) return 0;
    const int K[3] = {KN, KS, KO};
    return mm::mx_gemm_workspace_bytes(M, N, K, weights_fp4(wmode, KS, KO), (flags & MM_SPLIT_K_ALWAYS) != 0, (flags & MM_WS_TICKETS_ZEROED) != 0);
}

const char *mm_matmul_describe(int M, int N, int KN, int KS, int KO, int wmode, int flags, size_t workspace_bytes) {
    const int K[3] = {KN, KS, KO};
    if (M <= 0 || N <= 0 || !decode_split_ok(K)) return "none";
    if (M <= 64 && !mm::mx_gemm_small_m_uses_tiles(M, N, K, weights_fp4(wmode, KS, KO), workspace_bytes, (flags & MM_SPLIT_K_ALWAYS) != 0))
        return mm::mx_gemm_stream_supported(M, N, K, weights_fp4(wmode, KS, KO)) ? "mm::stream::mx_gemm_stream_kernel (weight streaming, M <= 64)"
                                                                         : "mm::skinny::mx_gemm_skinny*_kernel (weight streaming, M <= 64)";
    return mm::describe_mx_gemm256(M, N, K, weights_fp4(wmode, KS, KO), workspace_bytes, (flags & MM_SPLIT_K_ALWAYS) != 0, (flags & MM_WS_TICKETS_ZEROED) != 0,
                                   (flags & MM_OUT_F32) != 0);
}

int mm_matmul(const uint8_t *AN, const uint8_t *BN, const uint8_t *AS, const uint8_t *BS, const uint8_t *AO,
              const uint8_t *BO, const uint8_t *SFAN, const uint8_t *SFBN, const uint8_t *SFAS, const uint8_t *SFBS,
              const uint8_t *SFAO, const uint8_t *SFBO, int M, int N, int KN, int KS, int KO, int wmode, int flags,
              const void *bias_bf16, void *D_bf16, mm_stream_t stream) {
    return mm_matmul_ws(AN, BN, AS, BS, AO, BO, SFAN, SFBN, SFAS, SFBS, SFAO, SFBO, M, N, KN, KS, KO, wmode, flags, bias_bf16,
                        D_bf16, nullptr, 0, stream);
}

int mm_matmul_ws(const uint8_t *AN, const uint8_t *BN, const uint8_t *AS, const uint8_t *BS, const uint8_t *AO,
                 const uint8_t *BO, const uint8_t *SFAN, const uint8_t *SFBN, const uint8_t *SFAS, const uint8_t *SFBS,
                 const uint8_t *SFAO, const uint8_t *SFBO, int M, int N, int KN, int KS, int KO, int wmode, int flags,
                 const void *bias_bf16, void *D_bf16, void *workspace, size_t workspace_bytes, mm_stream_t stream) {
    if (M < 0 || N < 0 || KN < 0 || KS < 0 || KO < 0) return MM_ERR_BAD_ARG;
    if ((KN % 128) || (KS % 128) || (KO % 128)) return MM_ERR_BAD_SPLIT;
    if (wmode != MM_W_MATCH && wmode != MM_W_FP4) return MM_ERR_BAD_ARG;
    if (M == 0 || N == 0) return MM_OK;
    if (!D_bf16) return MM_ERR_BAD_ARG;
    const bool out_f32 = (flags & MM_OUT_F32) != 0;
    if (out_f32 && (!(flags & MM_ROUND_ONCE) || bias_bf16)) return MM_ERR_BAD_ARG;   // fp32 partial sums: no chain rounding, no bias
    const int K[3] = {KN, KS, KO};
    if (!segments_ok(K, {AN, AS, AO}, {SFAN, SFAS, SFAO}) || !segments_ok(K, {BN, BS, BO}, {SFBN, SFBS, SFBO})) return MM_ERR_BAD_ARG;
    if (KN + KS + KO == 0) {  // reference: C = zeros, no segment runs (gemm.cu:48-50)
        hipError_t e = hipMemsetAsync(D_bf16, 0, (size_t)M * N * (out_f32 ? 4 : 2), (hipStream_t)stream);
        return e == hipSuccess ? MM_OK : fail_hip(e, "mm_matmul(memset)");
    }
    mm::GemmArgs a = gemm_args({AN, AS, AO}, {SFAN, SFAS, SFAO}, {BN, BS, BO}, {SFBN, SFBS, SFBO}, M, N, K, flags, bias_bf16, D_bf16, true);
    a.ws = (float *)workspace;
    a.ws_bytes = workspace ? workspace_bytes : 0;
    a.tickets_zeroed = (workspace && (flags & MM_WS_TICKETS_ZEROED)) ? 1 : 0;
    a.force_split = (flags & MM_SPLIT_K_ALWAYS) ? 1 : 0;
    hipError_t e = mm::launch_mx_gemm(a, weights_fp4(wmode, KS, KO), (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_matmul");
}

// A kernel, not hipMemsetAsync: captured into a hipGraph (ROCm 7.2, MI355X) a memset node in front of the GEMM gave the right result
// on the first replay only (later replays were wrong as if the clearing were no longer ordered before the kernel); a kernel node
// replays in order (tools/probe_capture.py, profiles/notes_r04.md).
static __global__ void ws_reset_kernel(uint4 *p) { p[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u); }

size_t mm_gate_up_activate_workspace_bytes(int M, int I) {
    if (M <= 0 || I <= 0 || (I % 128)) return 0;
    return mm::mx_gemm_act_supported(M, 2 * I) ? 0 : (size_t)M * (size_t)(2 * I) * sizeof(uint16_t);
}

const char *mm_gate_up_activate_describe(int M, int I) {
    if (M <= 0 || I <= 0 || (I % 128)) return "none";
    const int Kany[3] = {0, 0, 4096};      // (the answer depends on K only for K in the tens of thousands: LDS of the scale images)
    if (!mm::mx_gemm_act_supported(M, 2 * I) && mm::gate_up_act_stream_supported(M, 2 * I, Kany, false, false))
        return "mm::stream::mx_gemm_stream_act_kernel (weight streaming with silu(gate) * up and the consumer's quantization inside, M <= 32)";
    return mm::describe_mx_gemm_act(M, 2 * I);
}

// the fused gate | up weight with the activation inside the weight-streaming launch (mx_gemm_stream.hip, ACT): M <= 32, one scale tile
static mm::GemmArgs act_stream_args(const Ptr3 &A, const Ptr3 &SFA, const Ptr3 &B, const Ptr3 &SFB, int M, int I, const int Kin[3], int flags,
                                    const int Kd[3], const Out3 &o, const Out3 &sf) {
    return gemm_args_act(A, SFA, B, SFB, M, I, Kin, flags, Kd, o, sf, false);
}

int mm_gate_up_activate(const uint8_t *AN, const uint8_t *BN, const uint8_t *AS, const uint8_t *BS, const uint8_t *AO,
                        const uint8_t *BO, const uint8_t *SFAN, const uint8_t *SFBN, const uint8_t *SFAS, const uint8_t *SFBS,
                        const uint8_t *SFAO, const uint8_t *SFBO, int M, int I, int KN, int KS, int KO, int DN, int DS, int DO,
                        int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, void *workspace,
                        size_t workspace_bytes, mm_stream_t stream) {
    const int Kin[3] = {KN, KS, KO}, Kd[3] = {DN, DS, DO};
    if (M < 0 || I < 0 || KN < 0 || KS < 0 || KO < 0) return MM_ERR_BAD_ARG;
    if (!decode_split_ok(Kin)) return MM_ERR_BAD_SPLIT;
    if (!split_ok(I, DN, DS, DO)) return MM_ERR_BAD_SPLIT;
    if (flags & ~MM_ROUND_ONCE) return MM_ERR_BAD_ARG;
    if (M == 0) return MM_OK;
    if (!segments_ok(Kin, {AN, AS, AO}, {SFAN, SFAS, SFAO}) || !segments_ok(Kin, {BN, BS, BO}, {SFBN, SFBS, SFBO})) return MM_ERR_BAD_ARG;
    if (!segments_ok(Kd, {oN, oS, oO}, {sfN, sfS, sfO})) return MM_ERR_BAD_ARG;
    const int N = 2 * I;
    if (!mm::mx_gemm_act_supported(M, N) && mm::gate_up_act_stream_supported(M, N, Kin, false, false)) {
        // M <= 16 on a wide layer (round 6): ONE weight-streaming launch with the activation inside -- no scratch, the same bytes
        const mm::GemmArgs a = act_stream_args({AN, AS, AO}, {SFAN, SFAS, SFAO}, {BN, BS, BO}, {SFBN, SFBS, SFBO}, M, I, Kin, flags, Kd, {oN, oS, oO},
                                               {sfN, sfS, sfO});
        hipError_t e = mm::launch_gate_up_act_stream(a, (hipStream_t)stream);
        return e == hipSuccess ? MM_OK : fail_hip(e, "mm_gate_up_activate");
    }
    if (!mm::mx_gemm_act_supported(M, N)) {
        // M <= 64: the weight-streaming GEMM into the caller's scratch (columns alternate 128 gate | 128 up), then the activation
        // quantizer on that layout: the same bytes as the fused epilogue (tests/test_gate_up_gpu.py)
        if (!workspace || workspace_bytes < (size_t)M * N * sizeof(uint16_t) || ((uintptr_t)workspace & 15)) return MM_ERR_BAD_ARG;
        const int st = mm_matmul(AN, BN, AS, BS, AO, BO, SFAN, SFBN, SFAS, SFBS, SFAO, SFBO, M, N, KN, KS, KO, MM_W_FP4, flags, nullptr,
                                 workspace, stream);
        if (st != MM_OK) return st;
        hipError_t e = mm::launch_direct_quantize(workspace, (const uint16_t *)workspace + 128, M, DN, DS, DO, 3, oN, oS, oO, sfN, sfS, sfO,
                                                  (hipStream_t)stream);
        return e == hipSuccess ? MM_OK : fail_hip(e, "mm_gate_up_activate");
    }
    const mm::GemmArgs a = gemm_args_act({AN, AS, AO}, {SFAN, SFAS, SFAO}, {BN, BS, BO}, {SFBN, SFBS, SFBO}, M, I, Kin, flags, Kd, {oN, oS, oO},
                                         {sfN, sfS, sfO}, true);
    hipError_t e = mm::launch_mx_gemm_act(a, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_gate_up_activate");
}

// 2: ONE launch and expected to be the fastest way through the MLP's first half (M <= 2: at M = 3, 4 every workgroup repeating the
// quantization loses to mm_rmsnorm_quantize / mm_reorder_quantize -> mm_gate_up_activate, itself one launch at M <= 16 --
// tools/time_mlp_decode.py: Llama-3-8B MLP at M = 1 / 2 / 4 23.1 / 25.3 / 36.9 us against 26.3 / 26.7 / 27.2); 1: runs; 0: cannot
static int gate_up_decode_supported(int M, int I, int KN, int KS, int KO, bool rms) {
    const int Kin[3] = {KN, KS, KO};
    if (M < 1 || I < 128 || (I % 128) || !decode_split_ok(Kin)) return 0;
    if (mm::gate_up_act_stream_supported(M, 2 * I, Kin, true, rms)) return M <= 2 ? 2 : 1;
    return decode_supported_w(M, 2 * I, KN, KS, KO, MM_W_FP4, rms) ? 1 : 0;
}
int mm_rmsnorm_gate_up_activate_decode_supported(int M, int I, int KN, int KS, int KO) { return gate_up_decode_supported(M, I, KN, KS, KO, true); }
int mm_gate_up_activate_decode_supported(int M, int I, int KN, int KS, int KO) { return gate_up_decode_supported(M, I, KN, KS, KO, false); }

// mm_gate_up_activate_decode (PLAIN, norm = mm::NO_NORM), mm_rmsnorm_gate_up_activate_decode (NORM) and mm_add_rmsnorm_gate_up_activate_decode
// (ADD_NORM: norm.res / norm.s_out)
static int gate_up_decode_entry(Variant v, const void *X_bf16, const mm::NormArgs &norm, const int16_t *reorder_index, const Ptr3 &B, const Ptr3 &SFB,
                                int M, int I, int KN, int KS, int KO, int DN, int DS, int DO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO,
                                uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, void *workspace, size_t workspace_bytes, mm_stream_t stream) {
    static const char *const name[] = {"mm_gate_up_activate_decode", "mm_rmsnorm_gate_up_activate_decode", "mm_add_rmsnorm_gate_up_activate_decode"};
    const int Kin[3] = {KN, KS, KO}, Kd[3] = {DN, DS, DO};
    if (M < 0 || I < 0 || KN < 0 || KS < 0 || KO < 0) return MM_ERR_BAD_ARG;
    if (!decode_split_ok(Kin)) return MM_ERR_BAD_SPLIT;
    if (!split_ok(I, DN, DS, DO)) return MM_ERR_BAD_SPLIT;
    if (flags & ~(v == PLAIN ? MM_ROUND_ONCE : MM_ROUND_ONCE | MM_NORM_NO_INTEGER_ROUND)) return MM_ERR_BAD_ARG;
    if (M == 0) return MM_OK;
    const int N = 2 * I;
    // mm_gate_up_activate_decode asks what its two-launch form needs; the norm entries ask their own query (I >= 128, either form)
    if (!(v == PLAIN ? decode_supported_w(M, N, KN, KS, KO, MM_W_FP4, false) : gate_up_decode_supported(M, I, KN, KS, KO, true))) return MM_ERR_UNSUPPORTED;
    // M <= 4 on a wide layer (round 6): (norm,) quantization, GEMM, silu(gate) * up and the consumer's quantization in ONE launch
    const bool one_launch = mm::gate_up_act_stream_supported(M, N, Kin, true, v != PLAIN);
    if (!X_bf16 || !reorder_index || !segments_ok(Kin, B, SFB) || !segments_ok(Kd, {oN, oS, oO}, {sfN, sfS, sfO})) return MM_ERR_BAD_ARG;
    // mm_gate_up_activate_decode asks the alignment of X in its one-launch form only (its other form is mm_qlinear_decode, which asks none)
    if ((v != PLAIN || one_launch) && ((uintptr_t)X_bf16 & 15)) return MM_ERR_BAD_ARG;
    if (v != PLAIN && (!norm.weight || ((uintptr_t)norm.weight & 15))) return MM_ERR_BAD_ARG;
    if (v == ADD_NORM && !residual_ok(X_bf16, norm.res, norm.s_out, M, KN + KS + KO)) return MM_ERR_BAD_ARG;
    if (one_launch) {
        const mm::GemmArgs a = act_stream_args({}, {}, B, SFB, M, I, Kin, flags, Kd, {oN, oS, oO}, {sfN, sfS, sfO});   // the launch quantizes X itself
        hipError_t e = mm::launch_gate_up_act_stream_decode(X_bf16, reorder_index, a, (hipStream_t)stream, norm);
        return e == hipSuccess ? MM_OK : fail_hip(e, name[v]);
    }
    // two launches: (add + norm +) quantize + gate | up GEMM into the scratch (columns alternate 128 gate | 128 up), then the activation
    // quantizer on that layout: the bytes of mm_reorder_quantize -> mm_gate_up_activate (tests/test_gate_up_gpu.py)
    if (!workspace || workspace_bytes < (size_t)M * N * sizeof(uint16_t) || ((uintptr_t)workspace & 15)) return MM_ERR_BAD_ARG;
    const int st = qlinear_decode_entry(v, X_bf16, norm, reorder_index, B, SFB, M, N, KN, KS, KO, MM_W_FP4, flags, nullptr, workspace, stream);
    if (st != MM_OK) return st;
    hipError_t e = mm::launch_direct_quantize(workspace, (const uint16_t *)workspace + 128, M, DN, DS, DO, 3, oN, oS, oO, sfN, sfS, sfO,
                                              (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, name[v]);
}

int mm_gate_up_activate_decode(const void *X_bf16, const int16_t *reorder_index, const uint8_t *BN, const uint8_t *BS, const uint8_t *BO,
                               const uint8_t *SFBN, const uint8_t *SFBS, const uint8_t *SFBO, int M, int I, int KN, int KS, int KO, int DN,
                               int DS, int DO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO,
                               void *workspace, size_t workspace_bytes, mm_stream_t stream) {
    return gate_up_decode_entry(PLAIN, X_bf16, mm::NO_NORM, reorder_index, {BN, BS, BO}, {SFBN, SFBS, SFBO}, M, I, KN, KS, KO, DN, DS, DO, flags, oN, oS,
                                oO, sfN, sfS, sfO, workspace, workspace_bytes, stream);
}

int mm_rmsnorm_gate_up_activate_decode(const void *X_bf16, const void *norm_weight_bf16, float eps, const int16_t *reorder_index, const uint8_t *BN,
                                       const uint8_t *BS, const uint8_t *BO, const uint8_t *SFBN, const uint8_t *SFBS, const uint8_t *SFBO, int M,
                                       int I, int KN, int KS, int KO, int DN, int DS, int DO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO,
                                       uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, void *workspace, size_t workspace_bytes, mm_stream_t stream) {
    return gate_up_decode_entry(NORM, X_bf16, norm_args(norm_weight_bf16, eps, flags), reorder_index, {BN, BS, BO}, {SFBN, SFBS, SFBO}, M, I, KN, KS, KO,
                                DN, DS, DO, flags, oN, oS, oO, sfN, sfS, sfO, workspace, workspace_bytes, stream);
}

int mm_add_rmsnorm_gate_up_activate_decode(const void *X_bf16, const void *R_bf16, void *S_out_bf16, const void *norm_weight_bf16, float eps,
                                           const int16_t *reorder_index, const uint8_t *BN, const uint8_t *BS, const uint8_t *BO,
                                           const uint8_t *SFBN, const uint8_t *SFBS, const uint8_t *SFBO, int M, int I, int KN, int KS, int KO,
                                           int DN, int DS, int DO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS,
                                           uint8_t *sfO, void *workspace, size_t workspace_bytes, mm_stream_t stream) {
    return gate_up_decode_entry(ADD_NORM, X_bf16, norm_args(norm_weight_bf16, eps, flags, R_bf16, S_out_bf16), reorder_index, {BN, BS, BO},
                                {SFBN, SFBS, SFBO}, M, I, KN, KS, KO, DN, DS, DO, flags, oN, oS, oO, sfN, sfS, sfO, workspace, workspace_bytes, stream);
}

int mm_down_activate_decode_supported_w(int M, int N, int DN, int DS, int DO, int wmode) {
    const int K[3] = {DN, DS, DO};
    if (M < 1 || N < 1 || !decode_split_ok(K)) return 0;
    if (wmode != MM_W_MATCH && wmode != MM_W_FP4) return 0;
    if (!mm::down_activate_stream_supported(M, N, K, weights_fp4(wmode, DS, DO))) return 0;
    return M <= 2 ? 2 : 1;      // every workgroup repeats silu * up + the quantization: one pass of its threads up to M = 2 at I = 14336
}
int mm_down_activate_decode_supported(int M, int N, int DN, int DS, int DO) { return mm_down_activate_decode_supported_w(M, N, DN, DS, DO, (DS | DO) ? MM_W_MATCH : MM_W_FP4); }

int mm_down_activate_decode(const void *GU_bf16, const uint8_t *BN, const uint8_t *BS, const uint8_t *BO, const uint8_t *SFBN, const uint8_t *SFBS,
                            const uint8_t *SFBO, int M, int N, int DN, int DS, int DO, int wmode, int flags, const void *bias_bf16, void *D_bf16,
                            mm_stream_t stream) {
    const int K[3] = {DN, DS, DO};
    if (M < 0 || N < 0 || DN < 0 || DS < 0 || DO < 0) return MM_ERR_BAD_ARG;
    if (!decode_split_ok(K)) return MM_ERR_BAD_SPLIT;
    if (wmode != MM_W_MATCH && wmode != MM_W_FP4) return MM_ERR_BAD_ARG;
    if (flags & ~MM_ROUND_ONCE) return MM_ERR_BAD_ARG;
    if (M == 0 || N == 0) return MM_OK;
    if (!mm_down_activate_decode_supported_w(M, N, DN, DS, DO, wmode)) return MM_ERR_UNSUPPORTED;
    if (!GU_bf16 || !D_bf16 || ((uintptr_t)GU_bf16 & 15)) return MM_ERR_BAD_ARG;
    const uint8_t *W[3] = {BN, BS, BO}, *SFW[3] = {SFBN, SFBS, SFBO};
    if (!segments_ok(K, {BN, BS, BO}, {SFBN, SFBS, SFBO})) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_down_activate_stream(GU_bf16, W, SFW, M, N, K, weights_fp4(wmode, DS, DO), (flags & MM_ROUND_ONCE) ? 0 : 1, bias_bf16, D_bf16,
                                                   (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_down_activate_decode");
}

int mm_matmul_ws_reset(void *workspace, size_t workspace_bytes, mm_stream_t stream) {
    if (!workspace || workspace_bytes < MM_WS_TICKET_BYTES || ((uintptr_t)workspace & 15)) return MM_ERR_BAD_ARG;
    static_assert(MM_WS_TICKET_BYTES % 16 == 0 && MM_WS_TICKET_BYTES / 16 <= 1024, "one workgroup clears the ticket words");
    hipLaunchKernelGGL(ws_reset_kernel, dim3(1), dim3(MM_WS_TICKET_BYTES / 16), 0, (hipStream_t)stream, (uint4 *)workspace);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_matmul_ws_reset");
}

int mm_reorder_quantize_grouped(const mm_quant_group *groups, int ngroups, int K, int KN, int KS, int KO, int mode, mm_stream_t stream) {
    if (ngroups < 0 || (ngroups > 0 && !groups)) return MM_ERR_BAD_ARG;
    if (!split_ok(K, KN, KS, KO)) return MM_ERR_BAD_SPLIT;
    if (mode != MM_QUANT_MIXED && mode != MM_QUANT_W4) return MM_ERR_BAD_ARG;
    if (K > 32768) return MM_ERR_BAD_ARG;
    const int Kseg[3] = {KN, KS, KO};
    for (int i = 0; i < ngroups; ++i) {
        const mm_quant_group &g = groups[i];
        if (g.rows < 0) return MM_ERR_BAD_ARG;
        if (g.rows == 0) continue;
        if (!g.src_bf16 || !g.reorder_index || !segments_ok(Kseg, {g.oN, g.oS, g.oO}, {g.sfN, g.sfS, g.sfO})) return MM_ERR_BAD_ARG;
    }
    mm::GroupedQuantArgs ga;
    ga.K = K; ga.KN = KN; ga.KS = KS; ga.KO = KO;
    int count = 0, max_rows = 0;
    auto flush = [&]() -> int {
        if (count == 0) return MM_OK;
        ga.ngroups = count;
        hipError_t e = mm::launch_reorder_quantize_grouped(ga, max_rows, mode == MM_QUANT_W4, (hipStream_t)stream);
        count = 0;
        max_rows = 0;
        return e == hipSuccess ? MM_OK : fail_hip(e, "mm_reorder_quantize_grouped");
    };
    for (int i = 0; i < ngroups; ++i) {
        const mm_quant_group &g = groups[i];
        if (g.rows == 0) continue;
        mm::QuantArgs &q = ga.g[count];
        q.src = (const uint16_t *)g.src_bf16;
        q.idx = g.reorder_index;
        q.o[0] = g.oN; q.o[1] = g.oS; q.o[2] = g.oO;
        q.sf[0] = g.sfN; q.sf[1] = g.sfS; q.sf[2] = g.sfO;
        q.rows = g.rows;
        max_rows = g.rows > max_rows ? g.rows : max_rows;
        if (++count == mm::MM_MAX_GROUPS) {
            const int st = flush();
            if (st != MM_OK) return st;
        }
    }
    return flush();
}

int mm_matmul_grouped(const mm_group *groups, int ngroups, int N, int KN, int KS, int KO, int wmode, int flags, mm_stream_t stream) {
    if (ngroups < 0 || N < 0 || KN < 0 || KS < 0 || KO < 0 || (ngroups > 0 && !groups)) return MM_ERR_BAD_ARG;
    if ((KN % 128) || (KS % 128) || (KO % 128)) return MM_ERR_BAD_SPLIT;
    if (wmode != MM_W_MATCH && wmode != MM_W_FP4) return MM_ERR_BAD_ARG;
    if (flags & MM_OUT_F32) return MM_ERR_UNSUPPORTED;    // fp32 partial sums come from mm_matmul only
    if (ngroups == 0 || N == 0) return MM_OK;
    const int Ks[3] = {KN, KS, KO};
    for (int i = 0; i < ngroups; ++i) {
        const mm_group &g = groups[i];
        if (g.M < 0) return MM_ERR_BAD_ARG;
        if (g.M == 0) continue;
        if (!g.D || !segments_ok(Ks, {g.AN, g.AS, g.AO}, {g.SFAN, g.SFAS, g.SFAO}) || !segments_ok(Ks, {g.BN, g.BS, g.BO}, {g.SFBN, g.SFBS, g.SFBO}))
            return MM_ERR_BAD_ARG;
    }
    // groups of at most 64 token rows share launches of the weight-streaming kernels, larger groups launches of the tiled
    // kernels (up to MM_MAX_GROUPS argument blocks per launch, carried in the kernel arguments)
    auto fill = [&](mm::GemmArgs &a, const mm_group &g) {
        a = gemm_args({g.AN, g.AS, g.AO}, {g.SFAN, g.SFAS, g.SFAO}, {g.BN, g.BS, g.BO}, {g.SFBN, g.SFBS, g.SFBO}, g.M, N, Ks, flags, g.bias_bf16, g.D, false);
    };
    if (KN + KS + KO == 0) {   // no segment: every output is zero (gemm.cu:48-50)
        for (int i = 0; i < ngroups; ++i)
            if (groups[i].M) {
                const int st = mm_matmul(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, groups[i].M, N, 0, 0, 0, wmode, flags, nullptr, groups[i].D, stream);
                if (st != MM_OK) return st;
            }
        return MM_OK;
    }
    mm::GroupedGemmArgs small;
    mm::GroupedTileArgs big;
    int nsmall = 0, nbig = 0, max_m = 0;
    auto flush_small = [&]() -> int {
        if (nsmall == 0) return MM_OK;
        small.ngroups = nsmall;
        hipError_t e = mm::mx_gemm_stream_grouped_supported(max_m, nsmall, N, Ks)
                           ? mm::launch_mx_gemm_stream_grouped(small, max_m, weights_fp4(wmode, KS, KO), (hipStream_t)stream)
                           : mm::launch_mx_gemm_skinny_grouped(small, max_m, weights_fp4(wmode, KS, KO), (hipStream_t)stream);
        nsmall = 0;
        max_m = 0;
        return e == hipSuccess ? MM_OK : fail_hip(e, "mm_matmul_grouped");
    };
    auto flush_big = [&]() -> int {
        if (nbig == 0) return MM_OK;
        big.ngroups = nbig;
        hipError_t e = mm::launch_mx_gemm256_grouped(big, weights_fp4(wmode, KS, KO), (hipStream_t)stream);
        nbig = 0;
        return e == hipSuccess ? MM_OK : fail_hip(e, "mm_matmul_grouped");
    };
    for (int i = 0; i < ngroups; ++i) {
        const mm_group &g = groups[i];
        if (g.M == 0) continue;
        if (g.M > 64) {
            fill(big.g[nbig], g);
            if (++nbig == mm::MM_MAX_GROUPS) {
                const int st = flush_big();
                if (st != MM_OK) return st;
            }
        } else {
            fill(small.g[nsmall], g);
            max_m = g.M > max_m ? g.M : max_m;
            if (++nsmall == mm::MM_MAX_GROUPS) {
                const int st = flush_small();
                if (st != MM_OK) return st;
            }
        }
    }
    const int st = flush_small();
    return st != MM_OK ? st : flush_big();
}

// ---- paged KV cache (kv_cache.hip, rope_append.hip, kv_prefill.hip)
// What every entry point shares: kv_geometry checks the numbers and fills the descriptor, kv_pointers checks what it points to (int4
// and fp8 need their params).  Two steps: a call with nothing to do returns MM_OK between them, before any pointer is looked at.
static_assert(mm::KV_INT4 == MM_KV_INT4 && mm::KV_BF16 == MM_KV_BF16 && mm::KV_FP8 == MM_KV_FP8_E4M3, "PagedKV::kind holds mm_kv_dtype codes");
int mm_kv_dtype_supported(int kv_dtype) { return kv_dtype == MM_KV_INT4 || kv_dtype == MM_KV_BF16 || kv_dtype == MM_KV_FP8_E4M3; }

static int kv_geometry(const void *kv_data, const void *kv_param, int kv_dtype, int max_pages, int L, int layer, int Hkv, int P, int head_dim,
                       const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_len, int B, mm::PagedKV *kv) {
    if (!mm_kv_dtype_supported(kv_dtype) || max_pages <= 0 || L <= 0 || layer < 0 || layer >= L || Hkv <= 0 || Hkv > 65535 ||
        P <= 0 || B < 0 || B > 65535 || head_dim <= 0)
        return MM_ERR_BAD_ARG;
    *kv = {(uint8_t *)kv_data, (uint16_t *)kv_param, kv_indptr, kv_indices, last_page_len, max_pages, L, layer, Hkv, P, B, kv_dtype};
    return head_dim == 128 ? MM_OK : MM_ERR_UNSUPPORTED;
}
static bool kv_pointers(const mm::PagedKV &kv) { return kv.data && (kv.kind == mm::KV_BF16 || kv.param) && kv.indptr && kv.indices && kv.last_page_len; }

int mm_kv_append(void *kv_data, void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer, int num_kv_heads, int page_size,
                 int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_len, int batch,
                 const void *k_bf16, const void *v_bf16, const int32_t *append_indptr, int num_tokens, mm_stream_t stream) {
    mm::PagedKV kv;
    if (int st = kv_geometry(kv_data, kv_param, kv_dtype, max_pages, num_layers, layer, num_kv_heads, page_size, head_dim, kv_indptr, kv_indices,
                             last_page_len, batch, &kv)) return st;
    if (num_tokens < 0) return MM_ERR_BAD_ARG;
    if (num_tokens == 0 || batch == 0) return MM_OK;
    if (!kv_pointers(kv) || !k_bf16 || !v_bf16 || !append_indptr) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_kv_append(kv, k_bf16, v_bf16, append_indptr, num_tokens, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_kv_append");
}

int mm_rope_kv_append(void *kv_data, void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer, int num_kv_heads, int page_size,
                      int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_len, int batch,
                      const void *q_bf16, const void *k_bf16, const void *v_bf16, int64_t qkv_token_stride, int num_qo_heads,
                      const void *cos_bf16, const void *sin_bf16, int64_t cs_token_stride, const int32_t *append_indptr, int num_tokens,
                      void *q_out_bf16, mm_stream_t stream) {
    mm::PagedKV kv;
    if (int st = kv_geometry(kv_data, kv_param, kv_dtype, max_pages, num_layers, layer, num_kv_heads, page_size, head_dim, kv_indptr, kv_indices,
                             last_page_len, batch, &kv)) return st;
    if (num_tokens < 0 || num_qo_heads <= 0 || num_qo_heads % num_kv_heads) return MM_ERR_BAD_ARG;
    // a row of a token's q (the widest of the three) and of cos / sin must fit its stride; the kernel moves dwords
    if (qkv_token_stride < (int64_t)num_qo_heads * 128 || cs_token_stride < 128 || (qkv_token_stride & 1) || (cs_token_stride & 1))
        return MM_ERR_BAD_ARG;
    if (num_tokens == 0) return MM_OK;
    if (batch == 0) return MM_ERR_BAD_ARG;                    // tokens that belong to no sequence
    if (!kv_pointers(kv) || !q_bf16 || !k_bf16 || !v_bf16 || !cos_bf16 || !sin_bf16 || !append_indptr || !q_out_bf16) return MM_ERR_BAD_ARG;
    if (((uintptr_t)q_bf16 | (uintptr_t)k_bf16 | (uintptr_t)v_bf16 | (uintptr_t)cos_bf16 | (uintptr_t)sin_bf16 | (uintptr_t)q_out_bf16) & 3)
        return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_rope_kv_append(kv, q_bf16, k_bf16, v_bf16, qkv_token_stride, num_qo_heads, cos_bf16, sin_bf16, cs_token_stride,
                                             append_indptr, num_tokens, q_out_bf16, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_rope_kv_append");
}

int mm_kv_copy_pages(void *kv_data, void *kv_param, int kv_dtype, int max_pages, int num_layers, int num_kv_heads, int page_size,
                     int head_dim, const int32_t *src_pages, const int32_t *dst_pages, const int32_t *rows, int num_pairs,
                     mm_stream_t stream) {
    mm::PagedKV kv;                                           // no layer (0) and no page table: every layer of the named pages
    if (int st = kv_geometry(kv_data, kv_param, kv_dtype, max_pages, num_layers, 0, num_kv_heads, page_size, head_dim, nullptr, nullptr,
                             nullptr, 0, &kv)) return st;
    if (num_pairs < 0 || !kv.data || (kv.kind != mm::KV_BF16 && !kv.param)) return MM_ERR_BAD_ARG;
    if (((uintptr_t)kv_data & 15) || ((uintptr_t)kv_param & 3)) return MM_ERR_BAD_ARG;
    if ((int64_t)num_layers * num_kv_heads > INT32_MAX / 32 / page_size) return MM_ERR_UNSUPPORTED;   // 2 L Hkv P rows of up to 16 vectors
    if (num_pairs == 0) return MM_OK;
    if (!src_pages || !dst_pages) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_kv_copy_pages(kv, src_pages, dst_pages, rows, num_pairs, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_kv_copy_pages");
}

int mm_kv_move_rows(void *kv_data, void *kv_param, int kv_dtype, int max_pages, int num_layers, int num_kv_heads, int page_size,
                    int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices, int batch, const int32_t *move_indptr,
                    const int32_t *src_pos, const int32_t *dst_pos, int num_moves, mm_stream_t stream) {
    mm::PagedKV kv;                                           // no layer (0) and no lengths: every layer, positions within the listed pages
    if (int st = kv_geometry(kv_data, kv_param, kv_dtype, max_pages, num_layers, 0, num_kv_heads, page_size, head_dim, kv_indptr, kv_indices,
                             nullptr, batch, &kv)) return st;
    if (num_moves < 0 || !kv.data || (kv.kind != mm::KV_BF16 && !kv.param)) return MM_ERR_BAD_ARG;
    if (((uintptr_t)kv_data & 15) || ((uintptr_t)kv_param & 3)) return MM_ERR_BAD_ARG;
    if (num_layers > 65535 || num_kv_heads > 32767) return MM_ERR_UNSUPPORTED;   // the grid: (2 Hkv, L, B)
    if (num_moves == 0 || batch == 0) return MM_OK;
    if (!kv_indptr || !kv_indices || !move_indptr || !src_pos || !dst_pos) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_kv_move_rows(kv, move_indptr, src_pos, dst_pos, num_moves, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_kv_move_rows");
}

// ---- greedy verification of drafts (verify.hip)
size_t mm_argmax_rows_workspace_bytes(int rows, int vocab) {
    if (rows <= 0 || vocab < 1 || vocab > MM_ARGMAX_MAX_VOCAB || rows > MM_ARGMAX_MAX_ROWS) return 0;
    return mm::argmax_workspace_bytes(rows, vocab);
}

int mm_argmax_rows(const void *logits_bf16, int rows, int vocab, long long ld, int32_t *out_idx, void *workspace, size_t workspace_bytes,
                   mm_stream_t stream) {
    if (rows < 0 || vocab < 1 || ld < vocab) return MM_ERR_BAD_ARG;
    if (vocab > MM_ARGMAX_MAX_VOCAB || rows > MM_ARGMAX_MAX_ROWS) return MM_ERR_UNSUPPORTED;
    if (rows == 0) return MM_OK;
    if (!logits_bf16 || !out_idx || ((uintptr_t)logits_bf16 & 1) || ((uintptr_t)out_idx & 3)) return MM_ERR_BAD_ARG;
    const size_t need = mm::argmax_workspace_bytes(rows, vocab);
    if (need && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7))) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_argmax_rows(logits_bf16, rows, vocab, ld, out_idx, need ? workspace : nullptr, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_argmax_rows");
}

int mm_verify_greedy(const int32_t *target_tok, const int32_t *draft_tok, const int32_t *root_tok, const uint64_t *tree_mask,
                     const int32_t *qo_indptr, int num_tokens, const int32_t *kv_indptr, const int32_t *last_page_len, int page_size, int batch,
                     int32_t *result, int32_t *move_src, int32_t *move_dst, mm_stream_t stream) {
    if (num_tokens < 0 || batch < 0 || page_size < 1 || ((uintptr_t)tree_mask & 7)) return MM_ERR_BAD_ARG;
    if (batch == 0) return MM_OK;
    if (!root_tok || !qo_indptr || !kv_indptr || !last_page_len || !result) return MM_ERR_BAD_ARG;
    if (num_tokens > 0 && (!target_tok || !draft_tok || !move_src || !move_dst)) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_verify_greedy(target_tok, draft_tok, root_tok, tree_mask, qo_indptr, num_tokens, kv_indptr, last_page_len,
                                            page_size, batch, result, move_src, move_dst, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_verify_greedy");
}

// ---- sampling (sample.hip)
size_t mm_sample_rows_workspace_bytes(int rows, int vocab) {
    if (rows <= 0 || vocab < 1 || vocab > MM_ARGMAX_MAX_VOCAB || rows > MM_ARGMAX_MAX_ROWS) return 0;
    return mm::sample_workspace_bytes(rows, vocab);
}

int mm_sample_rows(const void *logits_bf16, int rows, int vocab, long long ld, const float *u, const float *temperature, const int32_t *top_k,
                   const float *top_p, const float *min_p, int32_t *out_idx, void *workspace, size_t workspace_bytes, mm_stream_t stream) {
    if (rows < 0 || vocab < 1 || ld < vocab) return MM_ERR_BAD_ARG;
    if (vocab > MM_ARGMAX_MAX_VOCAB || rows > MM_ARGMAX_MAX_ROWS) return MM_ERR_UNSUPPORTED;
    if (rows == 0) return MM_OK;
    if (!logits_bf16 || !u || !out_idx || ((uintptr_t)logits_bf16 & 1)) return MM_ERR_BAD_ARG;
    if ((((uintptr_t)u | (uintptr_t)temperature | (uintptr_t)top_k | (uintptr_t)top_p | (uintptr_t)min_p | (uintptr_t)out_idx) & 3)) return MM_ERR_BAD_ARG;
    const size_t need = mm::sample_workspace_bytes(rows, vocab);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7)) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_sample_rows(logits_bf16, rows, vocab, ld, u, temperature, top_k, top_p, min_p, out_idx, workspace, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_sample_rows");
}

// ---- speculative sampling of chain drafts (spec_sample.hip, include/micromix_spec.h)
size_t mm_spec_sample_rows_workspace_bytes(int rows, int vocab) {
    if (rows <= 0 || vocab < 1 || vocab > MM_ARGMAX_MAX_VOCAB || rows > MM_ARGMAX_MAX_ROWS) return 0;
    return mm::spec_sample_workspace_bytes(rows, vocab);
}

int mm_spec_sample_rows(const void *logits_bf16, long long ld, const void *draft_logits_bf16, long long draft_ld, int rows, int vocab,
                        const int32_t *cand_tok, const float *u_accept, const float *u_resample, const float *temperature,
                        const int32_t *top_k, const float *top_p, const float *min_p, int32_t *out_idx, int32_t *accepted, void *workspace,
                        size_t workspace_bytes, mm_stream_t stream) {
    if (rows < 0 || vocab < 1 || ld < vocab || (draft_logits_bf16 && draft_ld < vocab)) return MM_ERR_BAD_ARG;
    if (vocab > MM_ARGMAX_MAX_VOCAB || rows > MM_ARGMAX_MAX_ROWS) return MM_ERR_UNSUPPORTED;
    if (rows == 0) return MM_OK;
    if (!logits_bf16 || !cand_tok || !u_accept || !u_resample || !out_idx) return MM_ERR_BAD_ARG;
    if (((uintptr_t)logits_bf16 | (uintptr_t)draft_logits_bf16) & 1) return MM_ERR_BAD_ARG;
    if ((((uintptr_t)cand_tok | (uintptr_t)u_accept | (uintptr_t)u_resample | (uintptr_t)temperature | (uintptr_t)top_k | (uintptr_t)top_p |
          (uintptr_t)min_p | (uintptr_t)out_idx | (uintptr_t)accepted) & 3)) return MM_ERR_BAD_ARG;
    const size_t need = mm::spec_sample_workspace_bytes(rows, vocab);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7)) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_spec_sample_rows(logits_bf16, ld, draft_logits_bf16, draft_ld, rows, vocab, cand_tok, u_accept, u_resample,
                                               temperature, top_k, top_p, min_p, out_idx, accepted, workspace, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_spec_sample_rows");
}

// ---- one step of the device allocator (kv_step.hip, include/micromix_kvstep.h)
static int kv_step_refused(int batch, int max_pages, int pages_per_seq) {
    if (batch < 0 || max_pages < 1 || pages_per_seq < 1) return MM_ERR_BAD_ARG;
    if (batch > MM_KV_STEP_MAX_BATCH) return MM_ERR_UNSUPPORTED;
    if (MM_KV_STEP_HEADER_INTS + 3LL * batch + max_pages + (long long)batch * pages_per_seq > INT32_MAX) return MM_ERR_UNSUPPORTED;
    return MM_OK;
}

size_t mm_kv_step_state_ints(int batch, int max_pages, int pages_per_seq) {
    if (batch <= 0 || kv_step_refused(batch, max_pages, pages_per_seq)) return 0;
    return (size_t)MM_KV_STEP_HEADER_INTS + 3 * (size_t)batch + (size_t)max_pages + (size_t)batch * pages_per_seq;
}

int mm_kv_step(int32_t *state, int batch, int max_pages, int pages_per_seq, int page_size, int max_seq_len, const int32_t *keep,
               int keep_stride, const int32_t *next_new, int num_next_tokens, const int32_t *depths, int32_t *kv_indptr, int32_t *kv_indices,
               long long kv_indices_capacity, int32_t *last_page_len, int32_t *append_indptr, int32_t *token_pos, mm_stream_t stream) {
    const int refused = kv_step_refused(batch, max_pages, pages_per_seq);
    if (refused == MM_ERR_BAD_ARG || page_size < 1 || max_seq_len < 1 || num_next_tokens < 0 || kv_indices_capacity < 0) return MM_ERR_BAD_ARG;
    if ((keep && keep_stride < 1) || (depths && !token_pos)) return MM_ERR_BAD_ARG;
    if (refused) return refused;
    if (batch == 0) return MM_OK;
    if (!state || !next_new || !kv_indptr || !kv_indices || !last_page_len || !append_indptr) return MM_ERR_BAD_ARG;
    if (((uintptr_t)state | (uintptr_t)keep | (uintptr_t)next_new | (uintptr_t)depths | (uintptr_t)kv_indptr | (uintptr_t)kv_indices |
         (uintptr_t)last_page_len | (uintptr_t)append_indptr | (uintptr_t)token_pos) & 3) return MM_ERR_BAD_ARG;
    const mm::KVStep s{state, batch, max_pages, pages_per_seq, page_size, max_seq_len, keep, keep_stride, next_new, num_next_tokens, depths,
                       kv_indptr, kv_indices, kv_indices_capacity, last_page_len, append_indptr, token_pos};
    hipError_t e = mm::launch_kv_step(s, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_kv_step");
}

// ---- the token half of a step (token_step.hip, include/micromix_tokens.h)
static int tokens_refused(int batch, long long ld_tok, int num_tokens) { return batch < 0 || ld_tok < 1 || num_tokens < 0 ? MM_ERR_BAD_ARG : MM_OK; }
static int tokens_limits(int batch, long long ld_tok) { return batch > MM_TOKENS_MAX_BATCH || ld_tok > MM_TOKENS_MAX_LD ? MM_ERR_UNSUPPORTED : MM_OK; }

int mm_token_step(int32_t *tokens, long long ld_tok, int batch, int32_t *total_len, int32_t *finished, const int32_t *result, int result_stride,
                  const int32_t *target_tok, int num_tokens, const int32_t *qo_indptr, const int32_t *root_tok, const int32_t *max_total,
                  const int32_t *stop_tok, int n_stop, const int32_t *kv_state, int32_t *emitted, mm_stream_t stream) {
    if (tokens_refused(batch, ld_tok, num_tokens) || result_stride < MM_VERIFY_STRIDE || n_stop < 0 || (stop_tok != nullptr) != (n_stop > 0))
        return MM_ERR_BAD_ARG;
    if (batch > 0) {
        if (!tokens || !total_len || !finished || !result || !qo_indptr || !root_tok || !max_total || (!target_tok && num_tokens > 0))
            return MM_ERR_BAD_ARG;
        if (((uintptr_t)tokens | (uintptr_t)total_len | (uintptr_t)finished | (uintptr_t)result | (uintptr_t)target_tok | (uintptr_t)qo_indptr |
             (uintptr_t)root_tok | (uintptr_t)max_total | (uintptr_t)stop_tok | (uintptr_t)kv_state | (uintptr_t)emitted) & 3) return MM_ERR_BAD_ARG;
    }
    if (tokens_limits(batch, ld_tok) || n_stop > MM_TOKENS_MAX_STOP) return MM_ERR_UNSUPPORTED;
    if (batch == 0) return MM_OK;
    const mm::TokenStep s{tokens, ld_tok, batch, total_len, finished, result, result_stride, target_tok, num_tokens, qo_indptr, root_tok, max_total,
                          stop_tok, n_stop, kv_state, emitted};
    hipError_t e = mm::launch_token_step(s, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_token_step");
}

size_t mm_ngram_draft_workspace_bytes(int batch, long long ld_tok) {
    if (batch <= 0 || tokens_refused(batch, ld_tok, 0) || tokens_limits(batch, ld_tok)) return 0;
    return mm::ngram_workspace_bytes(batch, ld_tok);
}

int mm_ngram_draft(int32_t *tokens, long long ld_tok, int batch, const int32_t *total_len, const int32_t *next_indptr, int num_tokens, int min_n,
                   int max_n, int32_t *draft_tok, int32_t *root_tok, int32_t *cand_tok, int32_t *match_len, int32_t *row_seq, int32_t *row_total_len,
                   void *workspace, size_t workspace_bytes, mm_stream_t stream) {
    if (tokens_refused(batch, ld_tok, num_tokens) || min_n < 1 || max_n < min_n) return MM_ERR_BAD_ARG;
    const bool limits = tokens_limits(batch, ld_tok) || max_n > MM_NGRAM_MAX_N;
    if (batch > 0) {
        if (!tokens || !total_len || !next_indptr || !root_tok || (!draft_tok && num_tokens > 0)) return MM_ERR_BAD_ARG;
        if (((uintptr_t)tokens | (uintptr_t)total_len | (uintptr_t)next_indptr | (uintptr_t)draft_tok | (uintptr_t)root_tok | (uintptr_t)cand_tok |
             (uintptr_t)match_len | (uintptr_t)row_seq | (uintptr_t)row_total_len | (uintptr_t)workspace) & 3) return MM_ERR_BAD_ARG;
        const size_t need = limits ? 0 : mm::ngram_workspace_bytes(batch, ld_tok);
        if (need && (!workspace || workspace_bytes < need)) return MM_ERR_BAD_ARG;
    }
    if (limits) return MM_ERR_UNSUPPORTED;
    if (batch == 0) return MM_OK;
    const mm::NgramDraft s{tokens, ld_tok, batch, total_len, next_indptr, num_tokens, min_n, max_n, draft_tok, root_tok, cand_tok, match_len,
                           row_seq, row_total_len, (unsigned *)workspace};
    hipError_t e = mm::launch_ngram_draft(s, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_ngram_draft");
}

// ---- uniform numbers keyed by seed and position (random.hip, include/micromix_random.h)
int mm_uniform_rows(const int64_t *seed, const int32_t *sub, int batch, const int32_t *row_seq, const int32_t *pos, int rows, int n, unsigned domain,
                    float *out, uint32_t *bits, long long ld_out, mm_stream_t stream) {
    if (rows < 0 || batch < 0 || n < 1 || ld_out < rows) return MM_ERR_BAD_ARG;
    if (rows > 0 && ((!out && !bits) || !pos || (!seed && batch > 0))) return MM_ERR_BAD_ARG;
    if (((uintptr_t)seed & 7) || (((uintptr_t)sub | (uintptr_t)row_seq | (uintptr_t)pos | (uintptr_t)out | (uintptr_t)bits) & 3)) return MM_ERR_BAD_ARG;
    if (n > MM_UNIFORM_MAX_N || rows > MM_UNIFORM_MAX_ROWS) return MM_ERR_UNSUPPORTED;
    if (rows == 0) return MM_OK;
    const mm::UniformRows s{(const long long *)seed, sub, batch, row_seq, pos, rows, n, domain, out, bits, ld_out};
    hipError_t e = mm::launch_uniform_rows(s, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_uniform_rows");
}

// ---- calibration statistics (calib_stats.hip, include/micromix_calib.h)
static int calib_refused(int rows, int K) {
    if (rows < 0 || K < 0) return MM_ERR_BAD_ARG;
    if (K < 128 || K % 128 || K > 32768 || rows > (1 << 20)) return MM_ERR_UNSUPPORTED;
    return MM_OK;
}

size_t mm_calib_workspace_bytes(int rows, int K) { return calib_refused(rows, K) || rows == 0 ? 0 : mm::calib_workspace_bytes(rows, K); }

int mm_calib_accumulate(const void *x, int dtype, int rows, int K, long long ld, float lamda, void *score_f32, void *counts_i64,
                        void *workspace, size_t workspace_bytes, mm_stream_t stream) {
    if (rows < 0 || K < 0 || ld < K || !(lamda > 0.0f) || !(lamda < __builtin_inff())) return MM_ERR_BAD_ARG;
    if (calib_refused(rows, K) || (dtype != 0 && dtype != 1)) return MM_ERR_UNSUPPORTED;
    if (rows == 0) return MM_OK;
    if (!x || !score_f32 || !counts_i64 || !workspace) return MM_ERR_BAD_ARG;
    if (((uintptr_t)x & 15) || (ld & 7) || ((uintptr_t)score_f32 & 3) || ((uintptr_t)counts_i64 & 7) || ((uintptr_t)workspace & 15)) return MM_ERR_BAD_ARG;
    if (workspace_bytes < mm::calib_workspace_bytes(rows, K)) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_calib_accumulate(x, dtype == 1, rows, K, ld, lamda, (float *)score_f32, (long long *)counts_i64, workspace,
                                               (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_calib_accumulate");
}

// ---- token log-probabilities (logprob.hip, include/micromix_logprob.h)
static int logprob_refused(int rows, int vocab, long long ld, int top_n) {
    if (rows < 0 || vocab < 1 || ld < vocab || top_n < 0 || top_n > 32) return MM_ERR_BAD_ARG;
    if (vocab > MM_ARGMAX_MAX_VOCAB || rows > MM_ARGMAX_MAX_ROWS) return MM_ERR_UNSUPPORTED;
    return MM_OK;
}

size_t mm_logprob_rows_workspace_bytes(int rows, int vocab, int top_n) {
    return logprob_refused(rows, vocab, vocab, top_n) || rows == 0 ? 0 : mm::logprob_workspace_bytes(rows, vocab, top_n);
}

int mm_logprob_rows(const void *logits_bf16, int rows, int vocab, long long ld, const int32_t *target, const float *temperature,
                    float *logprob, int32_t *rank, float *lse, int top_n, int32_t *top_idx, float *top_logprob, void *workspace,
                    size_t workspace_bytes, mm_stream_t stream) {
    if (int st = logprob_refused(rows, vocab, ld, top_n)) return st;
    if (rows == 0) return MM_OK;
    if (!logits_bf16 || ((uintptr_t)logits_bf16 & 1)) return MM_ERR_BAD_ARG;
    if ((((uintptr_t)target | (uintptr_t)temperature | (uintptr_t)logprob | (uintptr_t)rank | (uintptr_t)lse | (uintptr_t)top_idx |
          (uintptr_t)top_logprob) & 3)) return MM_ERR_BAD_ARG;
    if (!target != !logprob || (rank && !target)) return MM_ERR_BAD_ARG;
    if (top_n > 0 && (!top_idx || !top_logprob)) return MM_ERR_BAD_ARG;
    if (!target && !lse && top_n == 0) return MM_ERR_BAD_ARG;                     // nothing asked for
    const size_t need = mm::logprob_workspace_bytes(rows, vocab, top_n);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7)) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_logprob_rows(logits_bf16, rows, vocab, ld, target, temperature, logprob, rank, lse, top_n, top_idx, top_logprob,
                                           workspace, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_logprob_rows");
}

// ---- penalties, bias and mask before a token is picked (logits_process.hip, include/micromix_logits.h)
int mm_process_logits(const void *logits_bf16, int rows, int vocab, long long ld_in, void *out_bf16, long long ld_out, const int32_t *tokens,
                      long long ld_tok, int n_seq, const int32_t *row_seq, const int32_t *prompt_len, const int32_t *total_len,
                      const float *repetition_penalty, const float *frequency_penalty, const float *presence_penalty,
                      const int32_t *bias_idx, const float *bias_val, int n_bias, const int32_t *allowed_mask, long long ld_mask,
                      mm_stream_t stream) {
    if (rows < 0 || vocab < 1 || ld_in < vocab || ld_out < vocab || n_bias < 0) return MM_ERR_BAD_ARG;
    if (tokens && (n_seq < 1 || ld_tok < 1)) return MM_ERR_BAD_ARG;
    if (allowed_mask && ld_mask < ((long long)vocab + 31) / 32) return MM_ERR_BAD_ARG;
    if (rows > 0) {                                                                 // every refusal of an argument comes before a limit
        const uintptr_t in = (uintptr_t)logits_bf16, out = (uintptr_t)out_bf16;
        if (!in || !out || ((in | out) & 1)) return MM_ERR_BAD_ARG;
        if (tokens ? !prompt_len || !total_len : prompt_len || total_len || row_seq || repetition_penalty || frequency_penalty || presence_penalty)
            return MM_ERR_BAD_ARG;
        if (!bias_idx != !bias_val || (n_bias > 0) != (bias_idx != nullptr)) return MM_ERR_BAD_ARG;
        if ((((uintptr_t)tokens | (uintptr_t)row_seq | (uintptr_t)prompt_len | (uintptr_t)total_len | (uintptr_t)repetition_penalty |
              (uintptr_t)frequency_penalty | (uintptr_t)presence_penalty | (uintptr_t)bias_idx | (uintptr_t)bias_val | (uintptr_t)allowed_mask) & 3))
            return MM_ERR_BAD_ARG;
        // the in-place form, or spans of (rows - 1) ld + vocab elements that do not meet
        const uintptr_t in_end = in + 2 * ((uintptr_t)(rows - 1) * (uintptr_t)ld_in + (uintptr_t)vocab);
        const uintptr_t out_end = out + 2 * ((uintptr_t)(rows - 1) * (uintptr_t)ld_out + (uintptr_t)vocab);
        if (!(in == out && ld_in == ld_out) && in < out_end && out < in_end) return MM_ERR_BAD_ARG;
    }
    if (vocab > MM_ARGMAX_MAX_VOCAB || rows > MM_ARGMAX_MAX_ROWS || n_bias > (1 << 20) || (tokens && ld_tok > (1 << 24))) return MM_ERR_UNSUPPORTED;
    if (rows == 0) return MM_OK;
    hipError_t e = mm::launch_process_logits(logits_bf16, rows, vocab, ld_in, out_bf16, ld_out, tokens, ld_tok, n_seq, row_seq, prompt_len,
                                             total_len, repetition_penalty, frequency_penalty, presence_penalty, bias_idx, bias_val, n_bias,
                                             allowed_mask, ld_mask, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_process_logits");
}

// the un-windowed entry points are the windowed ones at window = 0
size_t mm_paged_decode_window_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int max_seq_len, int window) {
    if (batch <= 0 || num_kv_heads <= 0 || num_qo_heads <= 0 || max_seq_len < 0 || window < 0 || num_qo_heads % num_kv_heads) return 0;
    return mm::kv_decode_workspace_bytes(batch, num_qo_heads, num_kv_heads, max_seq_len, window);
}

size_t mm_paged_decode_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int max_seq_len) {
    return mm_paged_decode_window_workspace_bytes(batch, num_qo_heads, num_kv_heads, max_seq_len, 0);
}

int mm_paged_decode_window(const void *q_bf16, const void *kv_data, const void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer,
                           int num_kv_heads, int page_size, int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices,
                           const int32_t *last_page_len, int batch, int num_qo_heads, int max_seq_len, float sm_scale, void *workspace,
                           size_t workspace_bytes, void *o_bf16, mm_stream_t stream, int window) {
    mm::PagedKV kv;
    if (int st = kv_geometry(kv_data, kv_param, kv_dtype, max_pages, num_layers, layer, num_kv_heads, page_size, head_dim, kv_indptr, kv_indices,
                             last_page_len, batch, &kv)) return st;
    if (num_qo_heads <= 0 || num_qo_heads % num_kv_heads || max_seq_len < 0 || window < 0) return MM_ERR_BAD_ARG;
    if (num_qo_heads / num_kv_heads > 16) return MM_ERR_UNSUPPORTED;
    if (batch == 0) return MM_OK;
    if (!q_bf16 || !kv_pointers(kv) || !o_bf16) return MM_ERR_BAD_ARG;
    const size_t need = mm_paged_decode_window_workspace_bytes(batch, num_qo_heads, num_kv_heads, max_seq_len, window);
    if (need && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15))) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_paged_decode(kv, q_bf16, num_qo_heads, max_seq_len, window, sm_scale, workspace, o_bf16, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, window ? "mm_paged_decode_window" : "mm_paged_decode");
}

int mm_paged_decode(const void *q_bf16, const void *kv_data, const void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer,
                    int num_kv_heads, int page_size, int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices,
                    const int32_t *last_page_len, int batch, int num_qo_heads, int max_seq_len, float sm_scale, void *workspace,
                    size_t workspace_bytes, void *o_bf16, mm_stream_t stream) {
    return mm_paged_decode_window(q_bf16, kv_data, kv_param, kv_dtype, max_pages, num_layers, layer, num_kv_heads, page_size, head_dim, kv_indptr,
                                  kv_indices, last_page_len, batch, num_qo_heads, max_seq_len, sm_scale, workspace, workspace_bytes, o_bf16, stream, 0);
}

// shared-prefix decode: the sizes, the split and the workspace rules are mx_kv_shared_host.h's
size_t mm_paged_decode_shared_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int max_shared_len, int max_suffix_len) {
    return mm::kv_shared_workspace_bytes(batch, num_qo_heads, num_kv_heads, max_shared_len, max_suffix_len);
}

int mm_paged_decode_shared(const void *q_bf16, const void *kv_data, const void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer,
                           int num_kv_heads, int page_size, int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices,
                           const int32_t *last_page_len, int batch, int num_qo_heads, const int32_t *group_indptr,
                           const int32_t *group_members, const int32_t *shared_len, int max_shared_len, int max_suffix_len, float sm_scale,
                           void *workspace, size_t workspace_bytes, void *o_bf16, mm_stream_t stream) {
    mm::PagedKV kv;
    if (int st = kv_geometry(kv_data, kv_param, kv_dtype, max_pages, num_layers, layer, num_kv_heads, page_size, head_dim, kv_indptr, kv_indices,
                             last_page_len, batch, &kv)) return st;
    if (int st = mm::kv_shared_sizes_status(batch, num_qo_heads, num_kv_heads, max_shared_len, max_suffix_len)) return st;
    if (batch == 0) return MM_OK;
    if (!q_bf16 || !kv_pointers(kv) || !o_bf16 || !group_indptr || !group_members || !shared_len) return MM_ERR_BAD_ARG;
    const size_t need = mm::kv_shared_workspace_bytes(batch, num_qo_heads, num_kv_heads, max_shared_len, max_suffix_len);
    if (int st = mm::kv_shared_workspace_status(workspace, workspace_bytes, need)) return st;
    hipError_t e = mm::launch_paged_decode_shared(kv, q_bf16, num_qo_heads, group_indptr, group_members, shared_len, max_shared_len,
                                                  max_suffix_len, sm_scale, workspace, o_bf16, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_paged_decode_shared");
}

size_t mm_paged_prefill_window_workspace_bytes(int num_tokens, int batch, int num_qo_heads, int num_kv_heads, int max_seq_len, int window) {
    if (num_tokens <= 0 || batch <= 0 || batch > 65535 || num_kv_heads <= 0 || num_kv_heads > 65535 || num_qo_heads <= 0 ||
        max_seq_len < 0 || window < 0 || num_qo_heads % num_kv_heads || num_qo_heads / num_kv_heads > 16)
        return 0;
    return mm::kv_prefill_workspace_bytes(num_tokens, batch, num_qo_heads, num_kv_heads, max_seq_len, window);
}

size_t mm_paged_prefill_workspace_bytes(int num_tokens, int batch, int num_qo_heads, int num_kv_heads, int max_seq_len) {
    return mm_paged_prefill_window_workspace_bytes(num_tokens, batch, num_qo_heads, num_kv_heads, max_seq_len, 0);
}

// the body of the three prefill entries: `tree` says whether the call is mm_paged_prefill_tree (a null tree_mask is then an error)
static int paged_prefill(const void *q_bf16, const int32_t *qo_indptr, int num_tokens, const void *kv_data, const void *kv_param, int kv_dtype,
                         int max_pages, int num_layers, int layer, int num_kv_heads, int page_size, int head_dim, const int32_t *kv_indptr,
                         const int32_t *kv_indices, const int32_t *last_page_len, int batch, int num_qo_heads, int max_seq_len,
                         float sm_scale, void *workspace, size_t workspace_bytes, void *o_bf16, mm_stream_t stream, int window, bool tree,
                         const uint64_t *tree_mask) {
    mm::PagedKV kv;
    if (int st = kv_geometry(kv_data, kv_param, kv_dtype, max_pages, num_layers, layer, num_kv_heads, page_size, head_dim, kv_indptr, kv_indices,
                             last_page_len, batch, &kv)) return st;
    if (num_qo_heads <= 0 || num_qo_heads % num_kv_heads || max_seq_len < 0 || num_tokens < 0 || window < 0) return MM_ERR_BAD_ARG;
    if (num_qo_heads / num_kv_heads > 16) return MM_ERR_UNSUPPORTED;
    if (num_tokens == 0 || batch == 0) return MM_OK;
    if (!q_bf16 || !qo_indptr || !kv_pointers(kv) || !o_bf16) return MM_ERR_BAD_ARG;
    if (tree && (!tree_mask || ((uintptr_t)tree_mask & 7))) return MM_ERR_BAD_ARG;
    const size_t need = mm_paged_prefill_window_workspace_bytes(num_tokens, batch, num_qo_heads, num_kv_heads, max_seq_len, window);
    if (need && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15))) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_paged_prefill(kv, q_bf16, qo_indptr, num_tokens, num_qo_heads, max_seq_len, window, tree ? tree_mask : nullptr,
                                            sm_scale, workspace, o_bf16, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, tree ? "mm_paged_prefill_tree" : window ? "mm_paged_prefill_window" : "mm_paged_prefill");
}

int mm_paged_prefill_window(const void *q_bf16, const int32_t *qo_indptr, int num_tokens, const void *kv_data, const void *kv_param, int kv_dtype,
                            int max_pages, int num_layers, int layer, int num_kv_heads, int page_size, int head_dim, const int32_t *kv_indptr,
                            const int32_t *kv_indices, const int32_t *last_page_len, int batch, int num_qo_heads, int max_seq_len,
                            float sm_scale, void *workspace, size_t workspace_bytes, void *o_bf16, mm_stream_t stream, int window) {
    return paged_prefill(q_bf16, qo_indptr, num_tokens, kv_data, kv_param, kv_dtype, max_pages, num_layers, layer, num_kv_heads, page_size,
                         head_dim, kv_indptr, kv_indices, last_page_len, batch, num_qo_heads, max_seq_len, sm_scale, workspace, workspace_bytes,
                         o_bf16, stream, window, false, nullptr);
}

int mm_paged_prefill_tree(const void *q_bf16, const int32_t *qo_indptr, int num_tokens, const void *kv_data, const void *kv_param, int kv_dtype,
                          int max_pages, int num_layers, int layer, int num_kv_heads, int page_size, int head_dim, const int32_t *kv_indptr,
                          const int32_t *kv_indices, const int32_t *last_page_len, int batch, int num_qo_heads, int max_seq_len,
                          float sm_scale, void *workspace, size_t workspace_bytes, void *o_bf16, mm_stream_t stream,
                          const uint64_t *tree_mask) {
    return paged_prefill(q_bf16, qo_indptr, num_tokens, kv_data, kv_param, kv_dtype, max_pages, num_layers, layer, num_kv_heads, page_size,
                         head_dim, kv_indptr, kv_indices, last_page_len, batch, num_qo_heads, max_seq_len, sm_scale, workspace, workspace_bytes,
                         o_bf16, stream, 0, true, tree_mask);
}

int mm_paged_prefill(const void *q_bf16, const int32_t *qo_indptr, int num_tokens, const void *kv_data, const void *kv_param, int kv_dtype,
                     int max_pages, int num_layers, int layer, int num_kv_heads, int page_size, int head_dim, const int32_t *kv_indptr,
                     const int32_t *kv_indices, const int32_t *last_page_len, int batch, int num_qo_heads, int max_seq_len, float sm_scale,
                     void *workspace, size_t workspace_bytes, void *o_bf16, mm_stream_t stream) {
    return mm_paged_prefill_window(q_bf16, qo_indptr, num_tokens, kv_data, kv_param, kv_dtype, max_pages, num_layers, layer, num_kv_heads, page_size,
                                   head_dim, kv_indptr, kv_indices, last_page_len, batch, num_qo_heads, max_seq_len, sm_scale, workspace,
                                   workspace_bytes, o_bf16, stream, 0);
}

// ---- sparse MoE block (moe.hip)
static int moe_shape(int T, int E, int top_k) {
    if (T < 0 || E < 0 || top_k < 0) return MM_ERR_BAD_ARG;
    if (top_k < 1 || top_k > 8 || E < top_k || E > 64 || (int64_t)T * top_k > INT32_MAX) return MM_ERR_UNSUPPORTED;
    return MM_OK;
}

int mm_moe_route(const void *logits_bf16, int num_tokens, int num_experts, int top_k, int32_t *topk_ids, void *topk_w_bf16,
                 mm_stream_t stream) {
    if (int st = moe_shape(num_tokens, num_experts, top_k)) return st;
    if (num_tokens == 0) return MM_OK;
    if (!logits_bf16 || !topk_ids || !topk_w_bf16) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_moe_route(logits_bf16, num_tokens, num_experts, top_k, topk_ids, topk_w_bf16, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_moe_route");
}

int mm_moe_plan(const int32_t *topk_ids, int num_tokens, int num_experts, int top_k, int32_t *expert_offsets, int32_t *sorted_token,
                int32_t *slot_of, mm_stream_t stream) {
    if (int st = moe_shape(num_tokens, num_experts, top_k)) return st;
    if (num_tokens == 0) return MM_OK;
    if (!topk_ids || !expert_offsets || !sorted_token || !slot_of) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_moe_plan(topk_ids, num_tokens * top_k, num_experts, top_k, expert_offsets, sorted_token, slot_of,
                                       (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_moe_plan");
}

int mm_moe_gather(const void *x_bf16, const int32_t *sorted_token, int num_tokens, int num_rows, int hidden, void *x_sorted_bf16,
                  mm_stream_t stream) {
    if (num_tokens < 0 || num_rows < 0 || hidden < 0) return MM_ERR_BAD_ARG;
    if (hidden % 8) return MM_ERR_UNSUPPORTED;
    if (num_tokens == 0 || num_rows == 0 || hidden == 0) return MM_OK;
    if (!x_bf16 || !sorted_token || !x_sorted_bf16 || (((uintptr_t)x_bf16 | (uintptr_t)x_sorted_bf16) & 15)) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_moe_gather(x_bf16, sorted_token, num_tokens, num_rows, hidden, x_sorted_bf16, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_moe_gather");
}

int mm_moe_combine(const void *y_sorted_bf16, const int32_t *topk_ids, const void *topk_w_bf16, const int32_t *slot_of, int num_tokens,
                   int top_k, int hidden, void *out_bf16, mm_stream_t stream) {
    if (num_tokens < 0 || top_k < 0 || hidden < 0) return MM_ERR_BAD_ARG;
    if (top_k < 1 || top_k > 8 || hidden % 8 || (int64_t)num_tokens * top_k > INT32_MAX) return MM_ERR_UNSUPPORTED;
    if (num_tokens == 0 || hidden == 0) return MM_OK;
    if (!y_sorted_bf16 || !topk_ids || !topk_w_bf16 || !slot_of || !out_bf16 || (((uintptr_t)y_sorted_bf16 | (uintptr_t)out_bf16) & 15))
        return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_moe_combine(y_sorted_bf16, topk_ids, topk_w_bf16, slot_of, num_tokens, top_k, hidden, out_bf16,
                                          (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_moe_combine");
}

// ---- device-sized grouped launches (reorder_quantize.hip, mx_gemm_stream.hip, mx_gemm_tile.inc: the *_moe_kernel)
static_assert(sizeof(mm_moe_expert) == sizeof(mm::MoeExpert) && sizeof(mm_moe_expert) == 64, "the device table is read as mm::MoeExpert");

size_t mm_moe_sf_bytes(int num_rows, int num_experts, int Kseg) {
    if (num_rows < 0 || num_experts < 0 || Kseg < 0) return 0;
    return mm::moe_sf_bytes(num_rows, num_experts, Kseg);
}

static int moe_groups(const int32_t *expert_offsets, const mm_moe_expert *expert_table, int E, int n, int max_rows, mm::MoeGroups *mg) {
    if (E < 0 || n < 0) return MM_ERR_BAD_ARG;
    if (E < 1 || E > 64) return MM_ERR_UNSUPPORTED;
    *mg = {expert_offsets, reinterpret_cast<const mm::MoeExpert *>(expert_table), E, n, max_rows};
    return MM_OK;
}

int mm_moe_quantize(const void *src_bf16, const int32_t *row_of_slot, const int32_t *expert_offsets, const mm_moe_expert *expert_table,
                    int num_experts, int num_rows, int src_rows, int K, int KN, int KS, int KO, int mode, uint8_t *oN, uint8_t *oS, uint8_t *oO,
                    uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, mm_stream_t stream) {
    mm::MoeGroups mg;
    if (src_rows < 0 || K < 0) return MM_ERR_BAD_ARG;
    if (int st = moe_groups(expert_offsets, expert_table, num_experts, num_rows, num_rows, &mg)) return st;
    if (!split_ok(K, KN, KS, KO)) return MM_ERR_BAD_SPLIT;
    if (K > 32768 || (mode != MM_QUANT_MIXED && mode != MM_QUANT_W4)) return MM_ERR_BAD_ARG;
    if (num_rows == 0 || src_rows == 0) return MM_OK;
    if (!src_bf16 || !expert_offsets || !expert_table || ((uintptr_t)src_bf16 & 15) || ((uintptr_t)expert_table & 7)) return MM_ERR_BAD_ARG;
    const int Kseg[3] = {KN, KS, KO};
    if (!segments_ok(Kseg, {oN, oS, oO}, {sfN, sfS, sfO})) return MM_ERR_BAD_ARG;
    // rows are stored in 16-byte pieces, scales as dwords
    if ((((uintptr_t)oN | (uintptr_t)oS | (uintptr_t)oO) & 15) || (((uintptr_t)sfN | (uintptr_t)sfS | (uintptr_t)sfO) & 3)) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_moe_quantize(src_bf16, row_of_slot, mg, src_rows, K, KN, KS, KO, mode == MM_QUANT_W4, oN, oS, oO, sfN, sfS, sfO,
                                           (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_moe_quantize");
}

int mm_moe_activate_quantize(const void *a_bf16, const void *b_bf16, const int32_t *expert_offsets, const mm_moe_expert *expert_table,
                             int num_experts, int num_rows, int K, int KN, int KS, int KO, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN,
                             uint8_t *sfS, uint8_t *sfO, void *h_out_bf16, mm_stream_t stream) {
    mm::MoeGroups mg;
    if (K < 0) return MM_ERR_BAD_ARG;
    if (int st = moe_groups(expert_offsets, expert_table, num_experts, num_rows, num_rows, &mg)) return st;
    if (!split_ok(K, KN, KS, KO)) return MM_ERR_BAD_SPLIT;
    if (K > 32768) return MM_ERR_BAD_ARG;
    if (num_rows == 0) return MM_OK;
    if (!a_bf16 || !b_bf16 || !expert_offsets || !expert_table || ((uintptr_t)expert_table & 7)) return MM_ERR_BAD_ARG;
    if (((uintptr_t)a_bf16 | (uintptr_t)b_bf16 | (uintptr_t)h_out_bf16) & 15) return MM_ERR_BAD_ARG;
    const int Kseg[3] = {KN, KS, KO};
    if (!segments_ok(Kseg, {oN, oS, oO}, {sfN, sfS, sfO})) return MM_ERR_BAD_ARG;
    if ((((uintptr_t)oN | (uintptr_t)oS | (uintptr_t)oO) & 15) || (((uintptr_t)sfN | (uintptr_t)sfS | (uintptr_t)sfO) & 3)) return MM_ERR_BAD_ARG;
    hipError_t e = mm::launch_moe_activate_quantize(a_bf16, b_bf16, h_out_bf16, mg, K, KN, KS, KO, oN, oS, oO, sfN, sfS, sfO, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_moe_activate_quantize");
}

int mm_moe_matmul_supported(int max_rows, int N, int KN, int KS, int KO, int wmode) {
    if (max_rows < 1 || N < 1 || KN < 0 || KS < 0 || KO < 0 || (KN % 128) || (KS % 128) || (KO % 128)) return 0;
    if (wmode != MM_W_MATCH && wmode != MM_W_FP4) return 0;
    if (KN + KS + KO == 0) return 1;
    const int K[3] = {KN, KS, KO};
    return mm::mx_gemm_stream_moe_supported(max_rows, K) ? 1 : 0;
}

int mm_moe_matmul(const uint8_t *AN, const uint8_t *AS, const uint8_t *AO, const uint8_t *SFAN, const uint8_t *SFAS, const uint8_t *SFAO,
                  const int32_t *expert_offsets, const mm_moe_expert *expert_table, int num_experts, int num_rows, int max_rows, int N, int KN,
                  int KS, int KO, int wmode, int flags, void *D_bf16, mm_stream_t stream) {
    mm::MoeGroups mg;
    if (max_rows < 0 || N < 0 || KN < 0 || KS < 0 || KO < 0) return MM_ERR_BAD_ARG;
    if (int st = moe_groups(expert_offsets, expert_table, num_experts, num_rows, max_rows, &mg)) return st;
    if ((KN % 128) || (KS % 128) || (KO % 128)) return MM_ERR_BAD_SPLIT;
    if (wmode != MM_W_MATCH && wmode != MM_W_FP4) return MM_ERR_BAD_ARG;
    if (flags & MM_OUT_F32) return MM_ERR_UNSUPPORTED;    // fp32 partial sums come from mm_matmul only
    if (num_rows == 0 || N == 0 || max_rows == 0) return MM_OK;
    if (!expert_offsets || !expert_table || ((uintptr_t)expert_table & 7) || !D_bf16 || ((uintptr_t)D_bf16 & 1)) return MM_ERR_BAD_ARG;
    const int K[3] = {KN, KS, KO};
    if (!segments_ok(K, {AN, AS, AO}, {SFAN, SFAS, SFAO})) return MM_ERR_BAD_ARG;
    if (KN + KS + KO == 0) {   // no segment: every owned row is zero (gemm.cu:48-50); a kernel, see ws_reset_kernel
        hipError_t e = mm::launch_moe_zero_rows(D_bf16, expert_offsets, num_experts, num_rows, N, (hipStream_t)stream);
        return e == hipSuccess ? MM_OK : fail_hip(e, "mm_moe_matmul(zero)");
    }
    if (!mm_moe_matmul_supported(max_rows, N, KN, KS, KO, wmode)) return MM_ERR_UNSUPPORTED;
    const mm::GemmArgs a = gemm_args({AN, AS, AO}, {SFAN, SFAS, SFAO}, {}, {}, 0, N, K, flags, nullptr, D_bf16, false);   // W, SFW, bias: the expert table's
    const bool w4 = weights_fp4(wmode, KS, KO);
    // experts of 1 .. 64 rows on the weight-streaming kernels, larger ones on the tiled kernels: the kernel family mm_matmul_grouped
    // gives each of them; an expert finds itself in one launch and returns at once from the other
    hipError_t e = mm::launch_mx_gemm_stream_moe(a, mg, w4, (hipStream_t)stream);
    if (e == hipSuccess && max_rows > 64) e = mm::launch_mx_gemm256_moe(a, mg, w4, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_moe_matmul");
}

// ---- w1 | w3, silu * mul and w2's quantizer in one device-sized launch (mx_gemm_tile.inc: mx_gemm256_moe_act_kernel)
int mm_moe_gate_up_activate_supported(int max_rows, int I, int KN, int KS, int KO, int DN, int DS, int DO, int wmode) {
    const int Kin[3] = {KN, KS, KO};
    if (max_rows < 1 || I < 128 || !decode_split_ok(Kin) || !split_ok(I, DN, DS, DO)) return 0;
    if (wmode != MM_W_MATCH && wmode != MM_W_FP4) return 0;
    return weights_fp4(wmode, KS, KO) ? 1 : 0;      // the fused epilogue exists for fp4 weights
}

const char *mm_moe_gate_up_activate_describe(int num_experts, int num_rows, int I) {
    if (num_experts < 1 || num_experts > 64 || num_rows < 1 || I < 128 || (I % 128)) return "none";
    return mm::describe_mx_gemm256_moe_act(num_experts, num_rows, 2 * I);
}

int mm_moe_gate_up_activate(const uint8_t *AN, const uint8_t *AS, const uint8_t *AO, const uint8_t *SFAN, const uint8_t *SFAS, const uint8_t *SFAO,
                            const int32_t *expert_offsets, const mm_moe_expert *gate_up_table, int num_experts, int num_rows, int max_rows, int I,
                            int KN, int KS, int KO, int DN, int DS, int DO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN,
                            uint8_t *sfS, uint8_t *sfO, mm_stream_t stream) {
    mm::MoeGroups mg;
    const int Kin[3] = {KN, KS, KO}, Kd[3] = {DN, DS, DO};
    if (max_rows < 1 || I < 0 || KN < 0 || KS < 0 || KO < 0) return MM_ERR_BAD_ARG;
    if (int st = moe_groups(expert_offsets, gate_up_table, num_experts, num_rows, max_rows, &mg)) return st;
    if (!decode_split_ok(Kin) || !split_ok(I, DN, DS, DO)) return MM_ERR_BAD_SPLIT;
    if (flags & ~MM_ROUND_ONCE) return MM_ERR_BAD_ARG;
    if (num_rows == 0) return MM_OK;
    if (!expert_offsets || !gate_up_table || ((uintptr_t)gate_up_table & 7)) return MM_ERR_BAD_ARG;
    if (!segments_ok(Kin, {AN, AS, AO}, {SFAN, SFAS, SFAO}) || !segments_ok(Kd, {oN, oS, oO}, {sfN, sfS, sfO})) return MM_ERR_BAD_ARG;
    // rows leave in 16-byte pieces, scale atoms 16 bytes per lane
    if ((((uintptr_t)oN | (uintptr_t)oS | (uintptr_t)oO) & 15) || (((uintptr_t)sfN | (uintptr_t)sfS | (uintptr_t)sfO) & 15)) return MM_ERR_BAD_ARG;
    const mm::GemmArgs a = gemm_args_act({AN, AS, AO}, {SFAN, SFAS, SFAO}, {}, {}, 0, I, Kin, flags, Kd, {oN, oS, oO}, {sfN, sfS, sfO}, false);
    hipError_t e = mm::launch_mx_gemm256_moe_act(a, mg, (hipStream_t)stream);
    return e == hipSuccess ? MM_OK : fail_hip(e, "mm_moe_gate_up_activate");
}

int mm_diag_set_kernel_events(void *start_event, void *stop_event) {
    g_ev.start = (hipEvent_t)start_event;
    g_ev.stop = (hipEvent_t)stop_event;
    return MM_OK;
}

#ifdef MM_INSTRUMENT
int mm_diag_set_quant_clock_buffer(void *buf) { return mm::set_quant_clock_buffer((unsigned long long *)buf) == hipSuccess ? MM_OK : MM_ERR_LAUNCH; }
// only in the instrumented variant (csrc/mx_instrument.h): the default library has neither this symbol nor the in-kernel stores
int mm_diag_set_clock_buffer(void *buf) {
    g_clock_buf = (unsigned long long *)buf;
    return MM_OK;
}
#endif

}  // extern "C"
