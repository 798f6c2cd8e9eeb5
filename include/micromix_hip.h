/*
 * micromix_hip.h -- C ABI of libmicromix_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the MicroMix `mixedgemm` extension's MX hot path.  Every
 * entry point takes plain device pointers, sizes and a HIP stream; no torch
 * types.  The caller (the Python `mixedgemm` module, or a C++/pybind binding a
 * reference maintainer writes) owns allocation, shape
 * derivation and stream/device selection.
 *
 * Reference interfaces replaced (paths relative to the MicroMix tree):
 *   mm_reorder_quantize  <- run_reorder_quantize_x   mgemm/src/reorder.cu:434-469
 *                           run_reorder_quantize_w   mgemm/src/reorder.cu:471-506
 *                           run_reorder_quantize_w4  mgemm/src/reorder.cu:508-543
 *                           (bindings: mgemm/src/bindings.cpp:104-151,155-202,206-253)
 *   mm_matmul            <- matmul_host / matmul_w4_host   mgemm/src/gemm.cu:26-78
 *                           (binding: mgemm/src/bindings.cpp:50-102)
 *   mm_rmsnorm_quantize  <- run_rmsnorm_bf16_mixed   mgemm/src/rmsnorm.cu:314-352 (binding bindings.cpp:257-303)
 *   mm_activate_quantize / mm_downproj_quantize <- mgemm/src/activate.cu:510-551 (bindings.cpp:307-387)
 *   mm_sf_bytes_x / _w   <- SF allocation sizes      mgemm/src/bindings.cpp:120-123,170-172
 *   mm_sf_offset         <- SF layout atom            mgemm/include/sm120_sf_layout.h:170-173
 *
 * All functions are asynchronous with respect to the host (kernels are queued
 * on `stream`) and return an mm_status code; they never exit() or abort().
 */
#ifndef MICROMIX_HIP_H
#define MICROMIX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *mm_stream_t; /* hipStream_t */

enum mm_status {
    MM_OK = 0,
    MM_ERR_BAD_SPLIT = 1,   /* KN+KS+KO != K, or not multiples of 128 (reference: "Value error in run_reorder_quantize_*") */
    MM_ERR_BAD_ARG = 2,     /* null pointer / negative size / K too large for int16 indices */
    MM_ERR_LAUNCH = 3,      /* HIP launch error; text via mm_last_error() */
    MM_ERR_UNSUPPORTED = 4, /* configuration not built */
    MM_ERR_NO_DEVICE = 5    /* no gfx950 device */
};

/* mode argument of mm_reorder_quantize */
enum mm_quant_mode {
    MM_QUANT_MIXED = 0, /* segments -> MXFP4 | MXFP6(E3M2) | MXFP8(E4M3)   (reorder_quantize_x / _w)  */
    MM_QUANT_W4 = 1     /* segments -> MXFP4 | MXFP4 | MXFP4                (reorder_quantize_w4)       */
};

/* wmode argument of mm_matmul: format of the B (weight) segments */
enum mm_weight_mode {
    MM_W_MATCH = 0, /* B = fp4 | fp6 | fp8  (matmul_host,    gemm.cu:26-51) */
    MM_W_FP4 = 1    /* B = fp4 | fp4 | fp4  (matmul_w4_host, gemm.cu:53-78) */
};

/* flags argument of mm_matmul */
enum mm_matmul_flags {
    MM_ROUND_PER_SEGMENT = 0, /* default: accumulator rounded through bf16 after each segment, as the
                                 reference's three chained kernels do (gemm.cu:75-77) */
    MM_ROUND_ONCE = 1,        /* single fp32 accumulator across segments, one bf16 rounding */
    MM_SPLIT_K_ALWAYS = 2,    /* mm_matmul_ws: split K whenever the shape allows it, not only where the cost model expects a
                                 gain (tests and tuning) */
    MM_OUT_F32 = 8,           /* mm_matmul / mm_matmul_ws: D is [M,N] FP32 and receives the fp32 accumulator itself, unrounded.  For the
                                 partial products of a K-sharded (row-parallel) tensor-parallel layer: the ranks' partials are summed in
                                 fp32 and rounded to bf16 once, so the result does not degrade with the number of ranks.  Needs
                                 MM_ROUND_ONCE and bias_bf16 == NULL (the bias is added after the reduction); mm_matmul_grouped and mm_qlinear_decode
                                 return MM_ERR_UNSUPPORTED for it. */
    MM_WS_TICKETS_ZEROED = 4  /* mm_matmul_ws / mm_matmul_workspace_bytes / mm_matmul_describe: the first MM_WS_TICKET_BYTES of the
                                 workspace are ZERO (the caller cleared them once, when it created the workspace; every launch
                                 leaves them zero again).  Enables the split-K whose reduction runs inside the GEMM launch (64-row
                                 tiles, launches with few tiles): its workgroups count their arrivals per tile there.  Without the
                                 flag the workspace may hold anything, and that path is not taken. */
};
#define MM_WS_TICKET_BYTES 4096

int mm_version(void); /* major * 10000 + minor * 100 + patch */
const char *mm_strerror(int status);
/* Text of the last HIP error seen by this thread ("" if none). */
const char *mm_last_error(void);

/* Scale-factor tensor geometry (one tensor per segment). */
size_t mm_sf_bytes_x(int M, int Kseg); /* (M/128+1)*128 * Kseg/32, bindings.cpp:120-123 */
size_t mm_sf_bytes_w(int N, int Kseg); /* ceil(N/128)*128 * Kseg/32, bindings.cpp:170-172 */
size_t mm_sf_offset(int row, int block, int Kseg);

/*
 * Fused column-reorder + per-32-group absmax + E8M0 scale + MXFP4/6/8 quantize + pack.
 *   src_bf16       [rows, K] bf16, row-major, contiguous
 *   reorder_index  [K] int16: output column j takes input column reorder_index[j]
 *   KN,KS,KO       widths of the three reordered segments; multiples of 128; KN+KS+KO == K
 *   oN [rows,KN/2]; oS [rows,3*KS/4] (mixed) or [rows,KS/2] (w4); oO [rows,KO] (mixed) or [rows,KO/2] (w4)
 *   sfN,sfS,sfO    UE8M0 bytes in the layout of mm_sf_offset; buffers of at least
 *                  mm_sf_bytes_x(rows,Kseg) (activations) / mm_sf_bytes_w(rows,Kseg) (weights) bytes.
 *                  Only the bytes of real rows are written (the reference leaves padding uninitialised).
 * Pointers of zero-width segments may be NULL.
 */
int mm_reorder_quantize(const void *src_bf16, int rows, int K, const int16_t *reorder_index, int KN, int KS, int KO,
                        int mode, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO,
                        mm_stream_t stream);

/*
 * Same kernel, gathering only a SUBSET of the input columns: `index` has KN+KS+KO (<= K_in) entries, each
 * < K_in, and the rows of src are K_in wide.  This is what a K-sharded (row-parallel) tensor-parallel rank
 * runs: it quantizes just its 128-aligned slices of the reordered segments (micromix_amd/tp.py).  No
 * counterpart in the reference, which has no tensor parallelism.
 */
int mm_reorder_quantize_gather(const void *src_bf16, int rows, int K_in, const int16_t *index, int KN, int KS, int KO,
                               int mode, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO,
                               mm_stream_t stream);

/*
 * Reorder-free quantizers (reference: mgemm/src/activate.cu:44-202, 208-500; bindings.cpp:307-387).  Natural column order,
 * scale = amax > 1e-6 ? 2^ceil(log2(amax/FMAX)) : 1.0, a single RNE rounding from fp32.  Every SF buffer holds
 * mm_sf_bytes_x(rows, Kseg) bytes (the reference sizes the weight variants that way too, bindings.cpp:348-350).
 *   mm_activate_quantize : v = silu(A) * B, A and B [rows, KN+KS+KO] bf16 -> fp4 | fp6 | fp8   (activate_quantize_x); silu in fp32
 *                          with the hardware exp2 / reciprocal (a few fp32 ulps, as the reference's CUDA expf)
 *   mm_downproj_quantize : v = W;  mode MM_QUANT_MIXED -> fp4 | fp6 | fp8 (downproj_quantize_w),
 *                                  mode MM_QUANT_W4    -> fp4 | fp4 | fp4 (downproj_quantize_w4)
 */
int mm_activate_quantize(const void *A_bf16, const void *B_bf16, int rows, int KN, int KS, int KO, uint8_t *oN, uint8_t *oS,
                         uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, mm_stream_t stream);
int mm_downproj_quantize(const void *W_bf16, int rows, int KN, int KS, int KO, int mode, uint8_t *oN, uint8_t *oS, uint8_t *oO,
                         uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, mm_stream_t stream);

/*
 * RMSNorm fused with reorder + quantize (reference: rmsnorm_bf16_mixed_kernel, mgemm/src/rmsnorm.cu:95-312; binding
 * rmsnorm_quantize_x, bindings.cpp:257-303).  v = bf16(x[idx] * w[idx] * rsqrt(mean(x^2) + eps)), then the mixed quantizer of
 * mm_reorder_quantize on v (zero block -> byte 126) -- with the reference's extra step (rmsnorm.cu:262-267): the scaled value
 * is rounded to an integer (half away from zero), clamped and rounded through bf16 before the element conversion.
 *   flags  MM_RMS_REFERENCE (0): as the reference;  MM_RMS_NO_INTEGER_ROUND: without that step
 *   X_bf16 [rows, K], W_bf16 [K] norm weight, reorder_index [K] int16; outputs as mm_reorder_quantize(MM_QUANT_MIXED),
 *   SF buffers mm_sf_bytes_x(rows, Kseg).  Any K % 128 == 0 up to 32768 (the reference compiles 3072, 3584, 4096, 5120 and its
 *   block reduction is only right for 4096).
 */
enum mm_rmsnorm_flags { MM_RMS_REFERENCE = 0, MM_RMS_NO_INTEGER_ROUND = 1 };
int mm_rmsnorm_quantize(const void *X_bf16, const void *W_bf16, float eps, int rows, int K, const int16_t *reorder_index, int KN,
                        int KS, int KO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS,
                        uint8_t *sfO, mm_stream_t stream);

/*
 * mm_add_rmsnorm_quantize (version >= 660): mm_rmsnorm_quantize with the residual add of a decoder layer in front of the norm.
 *   s[i] = bf16_rne(f32(x[i]) + f32(r[i]))   one IEEE fp32 add of the widened values, rounded to nearest even; subnormals kept;
 *                                            every NaN result (inf - inf, a NaN operand) is 0x7FC0 -- torch's bf16 `x + r`, bit for bit wherever that is a number
 * s is written to S_out_bf16 [rows, K] (the new residual stream) and normalised and quantized: the six outputs are byte for byte
 * mm_rmsnorm_quantize applied to s, same summation order, integer rounding and flags.  The add happens while the row is staged, so s
 * costs one write and no extra read.  Every row count runs the kernels that stage the row through registers (mm_rmsnorm_quantize
 * takes an LDS-DMA kernel for small row counts, which cannot add on the way).
 *   R_bf16 [rows, K]; S_out_bf16 must not overlap X_bf16 or R_bf16 (MM_ERR_BAD_ARG before any launch); X, R, S_out and W 16-byte
 *   aligned (MM_ERR_BAD_ARG).  Everything else -- statuses included -- as mm_rmsnorm_quantize; rows == 0 is MM_OK with nothing written.
 */
int mm_add_rmsnorm_quantize(const void *X_bf16, const void *R_bf16, void *S_out_bf16, const void *W_bf16, float eps, int rows, int K,
                            const int16_t *reorder_index, int KN, int KS, int KO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO,
                            uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, mm_stream_t stream);

/*
 * The decode launches with the same add in front of their norm (version >= 660): mm_rmsnorm_qlinear_decode /
 * mm_rmsnorm_gate_up_activate_decode on s = X + R, arguments as theirs plus R_bf16 and S_out_bf16 ([M, K]).  Every workgroup forms s for
 * itself (the add is deterministic) and exactly one workgroup of the grid stores it to S_out.  D (the six buffers) are bit-identical
 * to mm_add_rmsnorm_quantize followed by mm_matmul (mm_gate_up_activate).  Supported exactly where the plain forms are
 * (mm_rmsnorm_qlinear_decode_supported_w / mm_rmsnorm_gate_up_activate_decode_supported).  S_out must not overlap X or R -- every
 * workgroup re-reads both -- and R, S_out are 16-byte aligned like X: MM_ERR_BAD_ARG before any launch; M == 0 is MM_OK.
 */
int mm_add_rmsnorm_qlinear_decode(const void *X_bf16, const void *R_bf16, void *S_out_bf16, const void *norm_weight_bf16, float eps,
                                  const int16_t *reorder_index, const uint8_t *BN, const uint8_t *BS, const uint8_t *BO, const uint8_t *SFBN,
                                  const uint8_t *SFBS, const uint8_t *SFBO, int M, int N, int KN, int KS, int KO, int wmode, int flags,
                                  const void *bias_bf16, void *D_bf16, mm_stream_t stream);
int mm_add_rmsnorm_gate_up_activate_decode(const void *X_bf16, const void *R_bf16, void *S_out_bf16, const void *norm_weight_bf16, float eps,
                                           const int16_t *reorder_index, const uint8_t *BN, const uint8_t *BS, const uint8_t *BO,
                                           const uint8_t *SFBN, const uint8_t *SFBS, const uint8_t *SFBO, int M, int I, int KN, int KS, int KO,
                                           int DN, int DS, int DO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS,
                                           uint8_t *sfO, void *workspace, size_t workspace_bytes, mm_stream_t stream);

/*
 * Three-segment mixed-precision block-scaled GEMM:
 *   D[m,n] = bf16( sum over segments, blocks b:  2^(sfa[m,b]-127) * 2^(sfb[n,b]-127) * sum_{k in b} a[m,k]*b[n,k] ) (+ bias[n])
 *   A segments: AN [M,KN/2] fp4, AS [M,3KS/4] fp6(E3M2), AO [M,KO] fp8(E4M3)
 *   B segments: wmode MM_W_MATCH: same formats as A;  MM_W_FP4: all fp4 ([N,Kseg/2])
 *   bias_bf16   optional [N] bf16 (NULL for none), added after the final rounding and rounded
 *               again, i.e. exactly `y = matmul(...); y = y + bias` (qLinearLayer.py:68-71)
 *   D_bf16      [M,N] bf16 row-major; fully overwritten (no pre-zeroing needed)
 */
int mm_matmul(const uint8_t *AN, const uint8_t *BN, const uint8_t *AS, const uint8_t *BS, const uint8_t *AO,
              const uint8_t *BO, const uint8_t *SFAN, const uint8_t *SFBN, const uint8_t *SFAS, const uint8_t *SFBS,
              const uint8_t *SFAO, const uint8_t *SFBO, int M, int N, int KN, int KS, int KO, int wmode, int flags,
              const void *bias_bf16, void *D_bf16, mm_stream_t stream);

/*
 * mm_matmul with a caller-owned scratch buffer.  For shapes with few output tiles (medium M or small N; M > 32) the GEMM
 * splits K across workgroups, which needs room for fp32 partial sums; the library never allocates, so the caller passes
 *   workspace        device buffer of at least mm_matmul_workspace_bytes(...) bytes, 16-byte aligned, not shared with a
 *                    call that may run concurrently on another stream (NULL or too small: same results, without the split)
 * mm_matmul_workspace_bytes returns 0 when the shape would not be split.  Results are deterministic either way; they differ
 * from the unsplit kernel only in fp32 summation order (the bf16 rounding chain of MM_ROUND_PER_SEGMENT is kept).
 */
size_t mm_matmul_workspace_bytes(int M, int N, int KN, int KS, int KO, int wmode, int flags);
int mm_matmul_ws(const uint8_t *AN, const uint8_t *BN, const uint8_t *AS, const uint8_t *BS, const uint8_t *AO,
                 const uint8_t *BO, const uint8_t *SFAN, const uint8_t *SFBN, const uint8_t *SFAS, const uint8_t *SFBS,
                 const uint8_t *SFAO, const uint8_t *SFBO, int M, int N, int KN, int KS, int KO, int wmode, int flags,
                 const void *bias_bf16, void *D_bf16, void *workspace, size_t workspace_bytes, mm_stream_t stream);
/*
 * gate_proj + up_proj + silu(gate) * up + MX quantization for down_proj as ONE launch (M > 64).  Replaces the reference's
 *     gate = gate_proj(x); up = up_proj(x); h = act_fn(gate) * up; down_proj quantizes h        (model/qLlamaLayer.py:377-387)
 * and this library's own three-op form  mm_matmul (twice) -> mm_activate_quantize (mgemm/src/activate.cu:44-202,
 * bindings.cpp:307-334) with the bytes of the latter: gate and up are rounded to bf16 as mm_matmul rounds them, silu * up and the
 * quantization are those of mm_activate_quantize, so the outputs are bit-identical to that pair -- without the [M, 2 I] bf16
 * round trip through HBM.
 *   A*, SFA*         the quantized activations x, as for mm_matmul ([M, K], split KN | KS | KO)
 *   B*, SFB*         ONE packed fp4 weight of 2 I rows (MM_W_FP4 layout: [2I, KN/2], [2I, KS/2], [2I, KO/2] + scale tensors): rows
 *                    [256 j, 256 j + 128) are gate_proj's rows [128 j, 128 j + 128), rows [256 j + 128, 256 j + 256) up_proj's rows of
 *                    the same indices (both packed with x's reorder index; scale tensors interleave the same way, one 128-row tile =
 *                    (Kseg/128) * 512 bytes).  I must be a multiple of 128.
 *   DN, DS, DO       the consumer's (down_proj's) split of its K = I input features, natural column order as mm_activate_quantize
 *   o*, sf*          the consumer's activation operands: [M, DN/2], [M, 3 DS/4], [M, DO] and scale tensors of mm_sf_bytes_x(M, D*) bytes
 *   flags            MM_ROUND_PER_SEGMENT (default) or MM_ROUND_ONCE: the rounding of gate / up, as mm_matmul
 *   workspace        only for M <= 64 (mm_gate_up_activate_workspace_bytes(M, I) > 0): M * 2 I bf16 values of scratch, 16-byte aligned;
 *                    those sizes run the weight-streaming GEMM into it and the activation quantizer on it (same bytes, two launches)
 */
size_t mm_gate_up_activate_workspace_bytes(int M, int I);
int mm_gate_up_activate(const uint8_t *AN, const uint8_t *BN, const uint8_t *AS, const uint8_t *BS, const uint8_t *AO,
                        const uint8_t *BO, const uint8_t *SFAN, const uint8_t *SFBN, const uint8_t *SFAS, const uint8_t *SFBS,
                        const uint8_t *SFAO, const uint8_t *SFBO, int M, int I, int KN, int KS, int KO, int DN, int DS, int DO,
                        int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, void *workspace,
                        size_t workspace_bytes, mm_stream_t stream);
/* The same for decode-sized batches, from the bf16 activations: reorder + quantize + gate | up GEMM in one launch (mm_qlinear_decode on the
 * interleaved weight, M <= 8, mm_qlinear_decode_supported(M, 2 I, ...) != 0, else MM_ERR_UNSUPPORTED) into `workspace` (M * 2 I bf16
 * values, 16-byte aligned), then silu(gate) * up + the MX quantization for down_proj: two launches instead of the three of
 * mm_reorder_quantize -> mm_gate_up_activate, the same bytes.  flags as mm_gate_up_activate. */
int mm_gate_up_activate_decode(const void *X_bf16, const int16_t *reorder_index, const uint8_t *BN, const uint8_t *BS, const uint8_t *BO,
                               const uint8_t *SFBN, const uint8_t *SFBS, const uint8_t *SFBO, int M, int I, int KN, int KS, int KO, int DN,
                               int DS, int DO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO,
                               void *workspace, size_t workspace_bytes, mm_stream_t stream);
/* ... with the RMSNorm in front (post_attention_layernorm -> gate / up -> act_fn -> the quantization for down_proj; round 6, version >= 510):
 * mm_rmsnorm_quantize -> mm_gate_up_activate, the same bytes.  On wide layers (2 I / 64 >= the CUs, K <= 8192) and M <= 4 it is ONE
 * weight-streaming launch with the norm, the quantization of x, the GEMM, silu(gate) * up and the consumer's quantization inside
 * (`workspace` unused); otherwise two launches (`workspace` as mm_gate_up_activate_decode).  Since round 6 mm_gate_up_activate (M <= 32)
 * and mm_gate_up_activate_decode (M <= 4) run as one such launch too on layers that wide; down_proj is then a plain mm_matmul on o* / sf*.
 * The _supported queries (also for mm_gate_up_activate_decode): 0 cannot run; 1 runs; 2 runs as ONE launch and is expected to be the
 * fastest form of the MLP's first half (M <= 2; beyond that mm_rmsnorm_quantize / mm_reorder_quantize -> mm_gate_up_activate wins).
 * flags: MM_ROUND_* | MM_NORM_NO_INTEGER_ROUND. */
int mm_gate_up_activate_decode_supported(int M, int I, int KN, int KS, int KO);
int mm_rmsnorm_gate_up_activate_decode_supported(int M, int I, int KN, int KS, int KO);
int mm_rmsnorm_gate_up_activate_decode(const void *X_bf16, const void *norm_weight_bf16, float eps, const int16_t *reorder_index, const uint8_t *BN,
                                       const uint8_t *BS, const uint8_t *BO, const uint8_t *SFBN, const uint8_t *SFBS, const uint8_t *SFBO, int M,
                                       int I, int KN, int KS, int KO, int DN, int DS, int DO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO,
                                       uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, void *workspace, size_t workspace_bytes, mm_stream_t stream);
/* The other half of a decode-sized MLP: down_proj straight from the bf16 gate | up matrix GU [M, 2 I] (128 gate columns alternating with
 * the 128 up columns of the same indices: the layout mm_gate_up_activate's scratch and mm_qlinear_decode on an interleaved weight produce;
 * 16-byte aligned).  Every workgroup of the weight-streaming GEMM computes silu(gate) * up and quantizes it for its own use -- the
 * bytes of mm_activate_quantize (activate.cu:44-202) -- so the result equals mm_matmul on mm_activate_quantize's output, in ONE launch
 * instead of two.  (DN, DS, DO) = down_proj's split of the I intermediate features in natural column order; B / SFB = its packed weights
 * (mm_downproj_quantize); wmode / flags / bias as mm_matmul.  M <= 4: mm_down_activate_decode_supported() returns 0 if the shape cannot
 * run, 1 if it can, 2 if it is expected to beat the two-launch form. */
int mm_down_activate_decode_supported(int M, int N, int DN, int DS, int DO);
/* ... for the weight mode the launch will run in (MM_W_FP4 / MM_W_MATCH).  The five-argument form answers for matching-precision weights,
 * whose ring / reduction tail in LDS is the larger one (64 KB against 48 KB): what it accepts launches in either mode, but it turns away
 * long-K shapes that fit with fp4 weights (round 6; version >= 500) */
int mm_down_activate_decode_supported_w(int M, int N, int DN, int DS, int DO, int wmode);
int mm_down_activate_decode(const void *GU_bf16, const uint8_t *BN, const uint8_t *BS, const uint8_t *BO, const uint8_t *SFBN, const uint8_t *SFBS,
                            const uint8_t *SFBO, int M, int N, int DN, int DS, int DO, int wmode, int flags, const void *bias_bf16, void *D_bf16,
                            mm_stream_t stream);
/* which kernels mm_gate_up_activate launches for (M, I) (thread-local buffer, as mm_matmul_describe) */
const char *mm_gate_up_activate_describe(int M, int I);

/*
 * Re-arms a workspace for MM_WS_TICKETS_ZEROED: queues a one-workgroup kernel on `stream` that clears its first MM_WS_TICKET_BYTES
 * (a kernel node when the stream is being captured into a hipGraph; `workspace` must be 16-byte aligned).  Call it when the workspace is created, inside every graph capture that uses a
 * workspace of its own, and after a launch that did not complete (a fault or a reset mid-launch can leave a ticket counter of the
 * in-kernel split-K non-zero, and a later launch on that workspace would then never see its last arrival and never write that tile).
 */
int mm_matmul_ws_reset(void *workspace, size_t workspace_bytes, mm_stream_t stream);

/*
 * Grouped GEMM (MoE experts; reference caller: the per-expert loop of model/qMixtralLayer.py:507-519, one matmul per expert and
 * linear): `ngroups` independent products D_g = matmul(A_g, B_g) that share N, the (KN, KS, KO) split, the weight mode and the
 * flags but have their own operands, token counts and outputs.  Groups of at most 64 token rows share launches of the
 * weight-streaming kernels, larger groups launches of the tiled kernels, 8 groups per launch.  Results are bit-identical to
 * ngroups calls of mm_matmul (which never splits K).  `groups` is a HOST array (copied into the kernel arguments).
 */
typedef struct mm_quant_group {
    const void *src_bf16;           /* [rows, K] bf16: the token rows routed to this expert */
    const int16_t *reorder_index;   /* [K]: this expert's own index */
    uint8_t *oN, *oS, *oO, *sfN, *sfS, *sfO; /* outputs as mm_reorder_quantize */
    int rows;                        /* 0 = skip */
} mm_quant_group;
/* mm_reorder_quantize for `ngroups` independent row sets that share K and the split (the per-expert reorder_quantize_x calls of
 * qMixtralLayer.py:507-519), 8 groups per launch; `groups` is a HOST array.  Bit-identical to the separate calls. */
int mm_reorder_quantize_grouped(const mm_quant_group *groups, int ngroups, int K, int KN, int KS, int KO, int mode, mm_stream_t stream);

typedef struct mm_group {
    const uint8_t *AN, *AS, *AO, *SFAN, *SFAS, *SFAO; /* activations of this group: [M, KN/2], [M, 3KS/4], [M, KO] + scales */
    const uint8_t *BN, *BS, *BO, *SFBN, *SFBS, *SFBO; /* its packed weights */
    const void *bias_bf16;                             /* optional [N] */
    void *D;                                           /* [M, N] bf16 */
    int M;                                             /* token rows of this group (0 = skip) */
} mm_group;
int mm_matmul_grouped(const mm_group *groups, int ngroups, int N, int KN, int KS, int KO, int wmode, int flags, mm_stream_t stream);

/*
 * QLinearLayer.forward for decode-sized inputs in ONE launch (reference: qLinearLayer.py:58-74 = reorder_quantize_x + matmul
 * (+ bias)): every workgroup quantizes the M activation rows into LDS itself and then streams its weight rows.  Bit-identical to
 * mm_reorder_quantize(MM_QUANT_MIXED) followed by mm_matmul.  mm_qlinear_decode_supported() returns 0 when the shape cannot run
 * (needs 1 <= M <= 8 and the quantized rows in LDS; mm_qlinear_decode then returns MM_ERR_UNSUPPORTED), 1 when it can, 2 when it
 * can and is expected to be faster than the two calls (every workgroup repeats the quantization, so many rows x many
 * workgroup rounds lose).
 *   X_bf16 [M, KN+KS+KO] bf16, reorder_index [K] int16, B / SFB as mm_matmul, flags MM_ROUND_*, bias optional, D [M, N] bf16
 */
int mm_qlinear_decode_supported(int M, int N, int KN, int KS, int KO);
int mm_qlinear_decode_supported_w(int M, int N, int KN, int KS, int KO, int wmode);      /* as mm_down_activate_decode_supported_w */
int mm_qlinear_decode(const void *X_bf16, const int16_t *reorder_index, const uint8_t *BN, const uint8_t *BS, const uint8_t *BO,
                      const uint8_t *SFBN, const uint8_t *SFBS, const uint8_t *SFBO, int M, int N, int KN, int KS, int KO,
                      int wmode, int flags, const void *bias_bf16, void *D_bf16, mm_stream_t stream);

/*
 * The same with the RMSNorm that precedes q/k/v and gate/up in the reference's decoder layers inside the launch (reference:
 * rmsnorm_quantize_x, mgemm/src/rmsnorm.cu:95-352 / bindings.cpp:257-303, followed by matmul; model/qLlamaLayer.py input_layernorm ->
 * q/k/v, post_attention_layernorm -> gate/up): every workgroup computes the row's sum of squares in the reference's summation order,
 * v = bf16((x * w) * rvar), the reference's integer rounding, and quantizes.  Bit-identical to mm_rmsnorm_quantize followed by
 * mm_matmul.  Needs K <= 8192 besides the conditions of mm_qlinear_decode; X and norm_weight 16-byte aligned.
 *   flags: MM_ROUND_* | MM_NORM_NO_INTEGER_ROUND (= mm_rmsnorm_quantize's MM_RMS_NO_INTEGER_ROUND)
 */
#define MM_NORM_NO_INTEGER_ROUND 0x100
int mm_rmsnorm_qlinear_decode_supported(int M, int N, int KN, int KS, int KO);
int mm_rmsnorm_qlinear_decode_supported_w(int M, int N, int KN, int KS, int KO, int wmode);
int mm_rmsnorm_qlinear_decode(const void *X_bf16, const void *norm_weight_bf16, float eps, const int16_t *reorder_index, const uint8_t *BN,
                              const uint8_t *BS, const uint8_t *BO, const uint8_t *SFBN, const uint8_t *SFBS, const uint8_t *SFBO, int M, int N,
                              int KN, int KS, int KO, int wmode, int flags, const void *bias_bf16, void *D_bf16, mm_stream_t stream);

/*
 * Paged KV cache for decode (version >= 600).  The reference's vendored FlashInfer layout and parameter convention
 * (flashinfer/page.cuh:15,75-103, quantization.cuh:60-80), head_dim 128, any page size P >= 1, 64-bit offsets throughout:
 *   MM_KV_INT4  kv_data uint8 [max_pages, L, 2, Hkv, P, 64]: index 0 of the third dim is K, 1 is V; byte j of a row holds element 2j in
 *               its low nibble and 2j + 1 in its high nibble.  kv_param fp16 [max_pages, L, 2, Hkv, P, 2] = (scale, zero) per token and
 *               head; value = code * scale - zero.
 *   MM_KV_BF16  kv_data bf16 [max_pages, L, 2, Hkv, P, 128]; kv_param unused (NULL)
 *   MM_KV_FP8_E4M3  (detect it with mm_kv_dtype_supported(3); mm_version stays 660)  kv_data uint8 [max_pages, L, 2, Hkv, P, 128]: OCP
 *               e4m3fn codes, element j in byte j.  kv_param fp16 [max_pages, L, 2, Hkv, P, 2] = (scale, zero), the int4 layout, with
 *               scale = 2^e and zero = +0.0, so value = decode(code) * scale - zero is the one dequantization rule of both kinds.
 *               Row rule (one group per 128 values, K and V alike, finite inputs): amax = the largest magnitude of the row's bf16
 *               values; e = the smallest integer in [-14, 15] with amax <= 448 * 2^e -- from amax's bf16 exponent field E and
 *               mantissa M, e = clamp(E - 135 + (M > 96), -14, 15); an all-zero or denormal row gives -14.  Element rule:
 *               code = e4m3fn(RNE(clamp(x * 2^-e, -448, 448))); the scaling is exact, the clamp (which acts only where e was clamped
 *               at 15) comes first, -0.0 keeps its sign (0x80), and no code is 0x7F / 0xFF.  Every dequantized value is exactly a
 *               bf16 number.  Half the bytes of bf16 (plus 4 parameter bytes per 128-byte row), relative error <= 2^-4 per value
 *               that is normal in e4m3 at the row's scale.  Attention over it computes bit for bit what it computes over a bf16
 *               cache holding the dequantized values.
 * Code 2 is unassigned: MM_ERR_BAD_ARG.
 * Page table (int32, device): kv_indptr [B + 1] and kv_indices [nnz] list sequence b's pages in order; last_page_len [B] in 1..P; a
 * sequence without pages has length 0.  The table already counts the tokens being appended.  Page indices outside [0, max_pages) are
 * skipped (nothing read or written for their tokens).
 *
 * mm_kv_append: k, v bf16 [T, Hkv, 128]; append_indptr [B + 1] splits the T tokens among the sequences (arange(B + 1) for one decode
 *   token each); sequence b's tokens go to its last append_indptr[b + 1] - append_indptr[b] positions (page.cuh:180-188).  Int4: each
 *   (token, head) row of 128 values is quantized as quantize_int_group(x, 4, 128) (model/qLlamaLayer.py:13-23) in fp32 with fp16
 *   parameters, round-half-even throughout:
 *     s = fp16(max(max - min, 1e-5) / 15);  base = clamp(rint(-min / s), 0, 15);  code = clamp(rint(x / s) + base, 0, 15);
 *     zero = fp16(base * s)     (correctly rounded divides; fp16 conversions saturate to +-65504; finite inputs)
 *   A row that does not straddle zero keeps the reference's behaviour: base clamps to 0 and the top codes clip.  zero >= 0 always; a
 *   zero of value 0 is stored as +0.0 (0x0000), never -0.0, also where rint(-min / s) is -0.0.  Bf16: a copy.  Fp8: the rule above.
 *   Nothing outside the target slots is written.
 * mm_paged_decode: one query token per sequence, q bf16 [B, Hq, 128], Hq = g * Hkv with g <= 16; query head h attends kv head h / g
 *   (HF repeat_kv) over every cached token (no mask); softmax in fp32 with sm_scale (<= 0: 1 / sqrt(128)); o bf16 [B, Hq, 128], rounded
 *   once; a sequence of length 0 gives o = 0.  Split-KV: the tokens are cut into chunks chosen from (B, Hkv, max_seq_len) alone, so a
 *   captured graph stays valid while the sequences grow up to max_seq_len (longer sequences are still attended in full, by the last
 *   chunk).  With more than one chunk the partials go to `workspace` (mm_paged_decode_workspace_bytes, 16-byte aligned, not shared
 *   with a concurrent call) and a second launch merges them; with one chunk (workspace_bytes() == 0) one launch writes o.
 * Null pointers and bad sizes: MM_ERR_BAD_ARG; head_dim != 128 or g > 16: MM_ERR_UNSUPPORTED; both without device work.
 */
enum mm_kv_dtype { MM_KV_INT4 = 0, MM_KV_BF16 = 1, MM_KV_FP8_E4M3 = 3 };
int mm_kv_dtype_supported(int kv_dtype);   /* 1 for the codes above, 0 for every other value */
int mm_kv_append(void *kv_data, void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer, int num_kv_heads, int page_size,
                 int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_len, int batch,
                 const void *k_bf16, const void *v_bf16, const int32_t *append_indptr, int num_tokens, mm_stream_t stream);
size_t mm_paged_decode_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int max_seq_len);
int mm_paged_decode(const void *q_bf16, const void *kv_data, const void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer,
                    int num_kv_heads, int page_size, int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices,
                    const int32_t *last_page_len, int batch, int num_qo_heads, int max_seq_len, float sm_scale, void *workspace,
                    size_t workspace_bytes, void *o_bf16, mm_stream_t stream);

/*
 * Causal multi-token attention over the paged KV cache (version >= 610): prompt ingestion, chunked prefill, a new turn over a cached
 * conversation, speculative verification.  Cache layout, page table, head rules (head_dim 128, Hq = g * Hkv with g <= 16, query head h
 * reads kv head h / g) and sm_scale as mm_paged_decode.
 * mm_paged_prefill: q bf16 [T, Hq, 128]; qo_indptr [B + 1] (int32, device) splits the T query tokens among the sequences, the same
 *   array and convention as mm_kv_append's append_indptr (qo_indptr[B] = T).  The mask is causal and aligned bottom-right (FlashInfer
 *   prefill.cuh:192,207): sequence b holds len_b tokens (from the page table, which already counts the new ones) and
 *   n_b = qo_indptr[b + 1] - qo_indptr[b]; its j-th query token sits at position p = len_b - n_b + j and attends cache positions
 *   0..p.  A query with p < 0 (a table that does not count the tokens) gives o = 0, and so does a length-0 sequence.  Softmax in fp32;
 *   o bf16 [T, Hq, 128], rounded once.  With n_b = 1 for every b it computes what mm_paged_decode computes (within rounding).
 *   Int4 cache: p.V runs on bf16 MFMA operands, bf16(p * scale_v) times the codes, so |o - exact| stays within 2 bf16 ulps plus
 *   2^-8 max|V| of the attended tokens.
 *   The grid and the workspace depend only on (T, B, Hq, Hkv, max_seq_len), so one captured graph of mm_kv_append + mm_paged_prefill
 *   stays valid across later steps with the same T while the sequences stay within max_seq_len (longer ones are still attended in
 *   full).  With more than one kv chunk the partials go to `workspace` (mm_paged_prefill_workspace_bytes, 16-byte aligned, not shared
 *   with a concurrent call) and a second launch merges them; workspace_bytes() == 0 means one launch and no workspace.
 * Null pointers, bad sizes, Hq not a multiple of Hkv, negative T or max_seq_len, or a missing, small or misaligned workspace:
 * MM_ERR_BAD_ARG; head_dim != 128 or g > 16: MM_ERR_UNSUPPORTED; T = 0 or B = 0: MM_OK; all without device work.
 */
size_t mm_paged_prefill_workspace_bytes(int num_tokens, int batch, int num_qo_heads, int num_kv_heads, int max_seq_len);
int mm_paged_prefill(const void *q_bf16, const int32_t *qo_indptr, int num_tokens, const void *kv_data, const void *kv_param,
                     int kv_dtype, int max_pages, int num_layers, int layer, int num_kv_heads, int page_size, int head_dim,
                     const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_len, int batch,
                     int num_qo_heads, int max_seq_len, float sm_scale, void *workspace, size_t workspace_bytes,
                     void *o_bf16, mm_stream_t stream);

/*
 * Sliding-window attention over the paged KV cache (detect the four entries by their symbols; mm_version stays 660).  `window` = W >= 1
 * is HF's sliding_window: the query at position p attends positions max(0, p - W + 1) .. p, W tokens with itself -- in decode
 * p = len_b - 1, in prefill p = len_b - n_b + j (bottom-right, as above).  W = 0: no window, the same launches and the same bits as
 * mm_paged_decode / mm_paged_prefill; W < 0: MM_ERR_BAD_ARG.  Everything else -- arguments, sm_scale, head rules, every cache kind, a
 * length-0 sequence, negative positions, statuses -- as the un-windowed entry of the same name.
 *   Only the kv tiles that hold a window are visited (decode: from token max(0, len_b - W) on; prefill: per query tile, from the
 *   window start of its first token rounded down to 64), and the split-KV chunks are laid over that span, not over the sequence:
 *   over min(max_seq_len, W) tokens in decode and min(max_seq_len, W + 64 / g + 62) in prefill.  So the grid and the
 *   workspace depend on the old host values plus W (the *_window_workspace_bytes queries), one captured graph stays valid while the
 *   sequences grow -- past max_seq_len too, the cost staying that of W tokens -- and W >= max_seq_len gives the un-windowed split.
 *   The page-table entry of a token below every window is never read (prefill: read and its token masked), and a page index outside [0, max_pages) masks its
 *   tokens as everywhere else, so the pages that lie wholly below every window may be released and reused: put -1 in their entries and
 *   keep the entries, so that positions do not move (PagedKVCache(window=W) does this).
 */
size_t mm_paged_decode_window_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int max_seq_len, int window);
int mm_paged_decode_window(const void *q_bf16, const void *kv_data, const void *kv_param, int kv_dtype, int max_pages, int num_layers,
                           int layer, int num_kv_heads, int page_size, int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices,
                           const int32_t *last_page_len, int batch, int num_qo_heads, int max_seq_len, float sm_scale, void *workspace,
                           size_t workspace_bytes, void *o_bf16, mm_stream_t stream, int window);
size_t mm_paged_prefill_window_workspace_bytes(int num_tokens, int batch, int num_qo_heads, int num_kv_heads, int max_seq_len, int window);
int mm_paged_prefill_window(const void *q_bf16, const int32_t *qo_indptr, int num_tokens, const void *kv_data, const void *kv_param,
                            int kv_dtype, int max_pages, int num_layers, int layer, int num_kv_heads, int page_size, int head_dim,
                            const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_len, int batch,
                            int num_qo_heads, int max_seq_len, float sm_scale, void *workspace, size_t workspace_bytes,
                            void *o_bf16, mm_stream_t stream, int window);

/*
 * RoPE + paged KV append in one launch (version >= 620): takes q | k | v as the fused q/k/v projection leaves them, leaves the rotated
 * q ready for mm_paged_decode / mm_paged_prefill and the rotated K and the untouched V in the cache.  Cache layout, page table, head_dim
 * 128 as above; no limit on g = Hq / Hkv.
 * mm_rope_kv_append: q, k, v are three bf16 pointers that share one token stride, qkv_token_stride, in elements; within a token the
 *   heads are contiguous ([Hq * 128], [Hkv * 128], [Hkv * 128]).  A packed [T, (Hq + 2 Hkv) * 128] projection is passed as base,
 *   base + Hq * 128, base + (Hq + Hkv) * 128 with stride (Hq + 2 Hkv) * 128; three contiguous tensors with Hq = Hkv share a stride too.
 *   cos, sin bf16 [T, 128] with row stride cs_token_stride (elements): row i belongs to flat token i (HF's position_embeddings,
 *   flattened; rope scaling is the caller's).  RoPE is HF's apply_rotary_pos_emb in bf16 tensor arithmetic,
 *   x * cos + rotate_half(x) * sin, every op rounded to bf16 -- for element d of a head row, in fp32, round to nearest even:
 *     a = bf16(x[d] * cos[d]);  b = bf16((d < 64 ? -x[d + 64] : x[d - 64]) * sin[d]);  y[d] = bf16(a + b)       (finite inputs)
 *   The rotated q of every one of the T tokens goes to q_out bf16 [T, Hq, 128], contiguous, whether or not the token's cache slot is
 *   valid.  The rotated K and V are written exactly as mm_kv_append writes them: the same slot rule (append_indptr, a page table that
 *   already counts the tokens), the same int4 / fp8 rule or bf16 copy, the same guards, nothing outside the target slots.
 *   q_out must not overlap q, k, v, cos or sin (other workgroups may still be reading them).  No workspace, no host reads of device
 *   arrays: capture-safe like mm_kv_append.
 * Null pointers, negative sizes, Hq not a multiple of Hkv, a stride smaller than the row it holds (Hq * 128, 128) or odd, a q / k / v /
 * cos / sin / q_out pointer that is not 4-byte aligned, or tokens without a sequence (num_tokens > 0 with batch = 0): MM_ERR_BAD_ARG;
 * head_dim != 128: MM_ERR_UNSUPPORTED; num_tokens = 0: MM_OK; all without device work.
 */
int mm_rope_kv_append(void *kv_data, void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer, int num_kv_heads, int page_size,
                      int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_len, int batch,
                      const void *q_bf16, const void *k_bf16, const void *v_bf16, int64_t qkv_token_stride, int num_qo_heads,
                      const void *cos_bf16, const void *sin_bf16, int64_t cs_token_stride, const int32_t *append_indptr, int num_tokens,
                      void *q_out_bf16, mm_stream_t stream);

/*
 * Page copy of the paged KV cache (detect it by its symbol; mm_version stays 660): what a sequence needs before it writes into a partly
 * filled page that it shares with another sequence (copy-on-write; PagedKVCache.fork / extend).  Cache layout and kinds as above.
 * mm_kv_copy_pages: for pair i, for every (layer, K / V, kv head), token rows [0, r_i) of page src_pages[i] go to the same rows of page
 *   dst_pages[i]: the code bytes (64 / 128 / 256 per row for int4 / fp8 / bf16) and, for int4 and fp8, the fp16 (scale, zero) dword of
 *   each row.  r_i = rows[i] clamped to [0, P]; rows == NULL: r_i = P, whole pages.  Bytes only: nothing is dequantized or rounded
 *   again, and nothing outside those rows of those destination pages is written.
 *   A pair is skipped (nothing read or written) when either index lies outside [0, max_pages), when src == dst, or when r_i <= 0.
 *   Preconditions: the destination pages are pairwise distinct, and no destination page is a source of the same call (the pairs are
 *   copied concurrently).  src_pages, dst_pages and rows are device int32 arrays of num_pairs entries.  kv_data is 16-byte aligned and
 *   kv_param 4-byte aligned.  No workspace, no host reads of device arrays: capture-safe like mm_kv_append.
 * Null kv_data, null kv_param for int4 / fp8, misaligned kv_data / kv_param, null src_pages / dst_pages with num_pairs > 0, non-positive
 * geometry, negative num_pairs, an unassigned kv_dtype (2 included): MM_ERR_BAD_ARG; head_dim != 128, or a page of 2^31 or more 16-byte
 * vectors at the bf16 width (2 L Hkv P >= 2^27): MM_ERR_UNSUPPORTED; num_pairs == 0: MM_OK; all without device work.
 */
int mm_kv_copy_pages(void *kv_data, void *kv_param, int kv_dtype, int max_pages, int num_layers, int num_kv_heads, int page_size,
                     int head_dim, const int32_t *src_pages, const int32_t *dst_pages, const int32_t *rows /* or NULL */, int num_pairs,
                     mm_stream_t stream);

/*
 * Tree-masked attention over the paged KV cache and keeping a path (detect the two entries by their symbols; mm_version stays 660):
 * verifying a tree draft (Medusa, EAGLE, SpecInfer: candidate continuations that share ancestors) in one call, then keeping the accepted
 * root-to-leaf path.  Cache layout, kinds and page table as above.
 * mm_paged_prefill_tree: mm_paged_prefill (no window) with another mask among the tokens just appended.  tree_mask: uint64 [num_tokens]
 *   on the device, 8-byte aligned, read by the kernel only (a captured graph replays with other trees written into it).  With
 *   base_b = len_b - n_b, query token j of sequence b (row qo_indptr[b] + j, cache slot base_b + j) attends
 *     every cache position < base_b: the committed tokens, all of them;
 *     new slot base_b + i exactly when i <= j and bit i of tree_mask[qo_indptr[b] + j] is set.
 *   Bits above j are ignored; bit j itself is honoured as given (a node usually attends itself: set it).  For a node, set the bits of
 *   its ancestors among the new tokens and its own.  Words with bits 0 .. j set give the bits of mm_paged_prefill, not merely its budget.
 *   A sequence with n_b > 64 ignores its words and is attended causally, exactly as mm_paged_prefill does, so one call can mix a prompt
 *   chunk with tree drafts.  A row that attends nothing (base_b = 0 and no bit set, or p < 0 as above) gives o = 0.
 *   Everything else -- head rules, sm_scale, the three kinds, split-KV, statuses, the grid and the workspace, whose size is
 *   mm_paged_prefill_workspace_bytes of the same (T, B, Hq, Hkv, max_seq_len) -- as mm_paged_prefill; a null or misaligned tree_mask
 *   (with T > 0 and B > 0): MM_ERR_BAD_ARG.  RoPE needs nothing new: mm_rope_kv_append takes a cos / sin row per token, the row of
 *   position base_b + depth(node).
 * mm_kv_move_rows: for sequence b, for the moves m in [move_indptr[b], move_indptr[b + 1]), for every (layer, K / V, kv head), the token
 *   row at logical position src_pos[m] of b goes to logical position dst_pos[m] of b: the code bytes and, for int4 and fp8, the fp16
 *   (scale, zero) dword.  Bytes only.  Position pos is row pos % P of page kv_indices[kv_indptr[b] + pos / P].
 *   Within a sequence every source is read before any destination is written, so a destination may be another move's source, as
 *   always happens when a path is packed down.  At most 64 moves per sequence are performed; entries of a sequence past its 64th are
 *   skipped.  A move is skipped (nothing read or written) when src == dst, when a position is negative or past the pages the sequence
 *   lists, or when a page index lies outside [0, max_pages).
 *   Preconditions: the destination positions of a sequence are pairwise distinct, and the pages written are not listed by another
 *   sequence that has moves in the same call.  move_indptr [batch + 1], src_pos, dst_pos [num_moves]: device int32.  kv_data is 16-byte
 *   aligned and kv_param 4-byte aligned.  No workspace, no host reads of device arrays: capture-safe like mm_kv_append.
 * Null kv_data, null kv_param for int4 / fp8, misaligned kv_data / kv_param, non-positive geometry, negative batch or num_moves, an
 * unassigned kv_dtype (2 included), or (with work to do) a null kv_indptr / kv_indices / move_indptr / src_pos / dst_pos: MM_ERR_BAD_ARG;
 * head_dim != 128, more than 65535 layers or 32767 kv heads: MM_ERR_UNSUPPORTED; num_moves == 0 or batch == 0: MM_OK; all without
 * device work.
 */
int mm_paged_prefill_tree(const void *q_bf16, const int32_t *qo_indptr, int num_tokens, const void *kv_data, const void *kv_param,
                          int kv_dtype, int max_pages, int num_layers, int layer, int num_kv_heads, int page_size, int head_dim,
                          const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_len, int batch,
                          int num_qo_heads, int max_seq_len, float sm_scale, void *workspace, size_t workspace_bytes,
                          void *o_bf16, mm_stream_t stream, const uint64_t *tree_mask /* [num_tokens] */);
int mm_kv_move_rows(void *kv_data, void *kv_param, int kv_dtype, int max_pages, int num_layers, int num_kv_heads, int page_size,
                    int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices, int batch,
                    const int32_t *move_indptr /* [batch + 1] */, const int32_t *src_pos, const int32_t *dst_pos, int num_moves,
                    mm_stream_t stream);

/*
 * Greedy verification of tree and chain drafts on the device (detect the three entries by their symbols; mm_version stays 660): the
 * vocabulary argmax of the verified rows, the walk that picks the accepted path, and the move table mm_kv_move_rows takes.  None of
 * the three reads device memory on the host or allocates: capture-safe.
 * mm_argmax_rows: out_idx[r] = the index of the maximum of row r of logits (bf16, row r at logits + r * ld elements, ld >= vocab)
 *   under one total order: any NaN, of either sign, is greater than +inf; +0 == -0; among equal maxima the lowest index wins (so the
 *   first NaN of a row).  This is torch.argmax's order on the CPU.  The answer does not depend on how a row is divided or on the order
 *   in which workgroups finish.  logits needs 2-byte alignment only and ld may be odd (logits[:, :V] of a padded lm_head output): the
 *   kernel peels the elements in front of and behind the 16-byte vectors of a row's part itself.
 *   A row is split into parts of MM_ARGMAX_CHUNK columns, one workgroup each; with more than one part (vocab > MM_ARGMAX_CHUNK) every
 *   part writes its (key, index) to `workspace` (mm_argmax_rows_workspace_bytes(rows, vocab) bytes, 8-byte aligned, no initialisation
 *   needed: every word read was written by the same call) and a second small launch reduces them.  vocab <= MM_ARGMAX_CHUNK: one
 *   launch, no workspace (the size is 0).
 *   Limits: vocab <= MM_ARGMAX_MAX_VOCAB = 2^20, rows <= MM_ARGMAX_MAX_ROWS = 65535 (a grid dimension): beyond, MM_ERR_UNSUPPORTED.
 *   Null logits or out_idx with rows > 0, rows < 0, vocab < 1, ld < vocab, an odd logits address, an out_idx that is not 4-byte aligned,
 *   a workspace that is needed and null, too small or not 8-byte aligned: MM_ERR_BAD_ARG.  rows == 0: MM_OK.  All without device work.
 * mm_verify_greedy: for sequence b with n = qo_indptr[b + 1] - qo_indptr[b] new tokens (rows t = qo_indptr[b] + i, node i) and
 *   base = len_b - n (len_b from kv_indptr / last_page_len / page_size as in mm_paged_prefill_tree): draft_tok[t] is node i's token,
 *   target_tok[t] the token the target model picks after it (mm_argmax_rows of its logits, or any sampler's choice), root_tok[b] the
 *   token picked after the last committed one.  parent(i) is the highest set bit of tree_mask[t] below bit i, -1 without one (bits at
 *   i and above are ignored); with a null tree_mask, i - 1 (chains).
 *   The walk, for 1 <= n <= 64 and root_tok[b] >= 0: cur = -1, want = root_tok[b], k = 0; take the lowest i with parent(i) == cur and
 *   draft_tok == want; none: stop; else path[k++] = i, want = target_tok[row i], cur = i, again.
 *   result [batch, MM_VERIFY_STRIDE]: [0] = k, [1] = want (the bonus token; root_tok[b] when nothing matched or n == 0),
 *   [2 .. 2 + k) the path, the rest -1.  A sequence with n > 64 or root_tok[b] < 0 is no draft but a prompt chunk (which the attention
 *   kernels treat causally too) and keeps all: [0] = n, [1] = target_tok of its last row (-1 when n == 0), every path entry -1, no moves.
 *   move_src, move_dst [num_tokens], laid over qo_indptr, to be passed on as mm_kv_move_rows(..., move_indptr = qo_indptr, move_src,
 *   move_dst, num_moves = num_tokens): row qo_indptr[b] + i of a draft with i < k holds src = base + path[i], dst = base + i; every
 *   other row holds src = dst = -1.  Every element of result, move_src and move_dst is written by every call.
 *   qo_indptr entries are clamped to [0, num_tokens] as the attention kernels do.  No workspace.
 *   Null target_tok / draft_tok / move_src / move_dst with num_tokens > 0, null root_tok / qo_indptr / kv_indptr / last_page_len /
 *   result with batch > 0, a tree_mask that is not 8-byte aligned, negative num_tokens or batch, page_size < 1: MM_ERR_BAD_ARG;
 *   batch == 0: MM_OK; all without device work.
 */
#define MM_ARGMAX_CHUNK 8192          /* columns of a row that one workgroup reduces */
#define MM_ARGMAX_MAX_VOCAB (1 << 20)
#define MM_ARGMAX_MAX_ROWS 65535
#define MM_VERIFY_STRIDE 66           /* ints per sequence in mm_verify_greedy's result: k, the bonus token, 64 path entries */
size_t mm_argmax_rows_workspace_bytes(int rows, int vocab);
int mm_argmax_rows(const void *logits_bf16, int rows, int vocab, long long ld /* elements between rows, >= vocab */,
                   int32_t *out_idx /* [rows] */, void *workspace, size_t workspace_bytes, mm_stream_t stream);
int mm_verify_greedy(const int32_t *target_tok /* [T] */, const int32_t *draft_tok /* [T] */, const int32_t *root_tok /* [batch] */,
                     const uint64_t *tree_mask /* [T] or null: chains */, const int32_t *qo_indptr /* [batch + 1] */, int num_tokens,
                     const int32_t *kv_indptr, const int32_t *last_page_len, int page_size, int batch,
                     int32_t *result /* [batch, 66] */, int32_t *move_src /* [T] */, int32_t *move_dst /* [T] */, mm_stream_t stream);

/*
 * Sampling on the device (detect the two entries by their symbols; mm_version stays 660): out_idx[r] = a token drawn from row r of
 * bf16 logits under temperature, top-k, top-p and min-p, so that mm_sample_rows -> mm_verify_greedy closes a captured speculative
 * step as mm_argmax_rows -> mm_verify_greedy does for greedy decoding: sample the target's token at every node, keep the draft path
 * that matches, emit the target's sample as the bonus token -- distributed as the target model's, whatever the draft.  The library
 * draws no random numbers: u brings one uniform number per row.  u, temperature, top_k, top_p, min_p are DEVICE arrays of `rows`
 * entries (fp32; top_k int32), read by the kernels only, so one captured graph serves any mix of requests rewritten in place.  A null
 * temperature means 1.0, a null filter array means that filter is off; u is required.  Nothing is read on the host, nothing allocated.
 * The rule, for row r with logits l_i (i < vocab), u = u[r] (NaN -> 0, else clamped to [0, 1 - 2^-24]), T = temperature[r],
 * k = top_k[r], p = top_p[r], q = min_p[r]:
 *   1 Greedy cases.  m = the row maximum in mm_argmax_rows' order.  m NaN or +-inf, T <= 0 or T NaN: out_idx[r] is exactly what
 *     mm_argmax_rows returns for the row.  Every other row has a finite m and no NaN.
 *   2 Weights.  w_i = exp((l_i - m) / T), -inf -> 0; the maximum has w = 1.
 *   3 Classes.  Tokens of equal value form one class (+0 and -0 are one class, as in mm_argmax_rows' key); the classes are ordered by
 *     descending value; each filter keeps a non-empty prefix of that order.
 *   4 Filters.  top-k: the shortest prefix whose token count is >= k, for 1 <= k < vocab (any other k: off); Z_k is its mass.
 *     top-p: the shortest prefix whose mass is >= p * Z_k, for p < 1 (p <= 0: the top class only; p >= 1 or NaN: off).
 *     min-p: the classes with w >= q, for 0 < q <= 1 (any other q: off).
 *   5 Kept set.  The shortest of the three prefixes.  Whole classes are kept, so equal logits are treated equally: HF's
 *     TopKLogitsWarper exactly; for top-p a superset of HF's set by at most the rest of one tie class; min-p does not depend on where
 *     it stands in the chain.
 *   6 Draw.  Z = the kept mass; out_idx[r] = the first kept index i, in ascending index order, with sum_{kept j <= i} w_j > u * Z; if
 *     rounding leaves none, the last kept index with w > 0.
 *   How the kernels realise it: w = exp2((l - m) * (log2e / T)) in fp32 (V_EXP_F32), then W = trunc(w * 2^43) as a 64-bit integer, and
 *   every mass above is a sum of W's.  Integer sums are exact and do not depend on their order, so the result is a function of the
 *   inputs alone -- the same bits on every run and however a row is divided -- and "rounding leaves none" cannot occur.  A bf16 row holds
 *   at most 65 281 classes, named by mm_argmax_rows' 16-bit key: the filters are a radix select on it (two 256-bin histogram levels of
 *   counts and masses), without a sort.  tests/sample_oracle.py derives the bound on a prefix mass against the rule in exact arithmetic.
 *   logits, ld, the limits on vocab and rows and the split into parts of MM_ARGMAX_CHUNK columns: as mm_argmax_rows (2-byte alignment,
 *   any ld >= vocab).  workspace: mm_sample_rows_workspace_bytes(rows, vocab) bytes (0 for arguments mm_sample_rows refuses), 8-byte
 *   aligned, always needed, no initialisation needed: every word read was written by the same call.  It holds 3 KiB per part of every
 *   row (the histograms) and 2 KiB per row.  Launches: mm_argmax_rows' one or two, then 2 (no top_k and no top_p array) or 8.
 *   Null logits, u or out_idx with rows > 0, rows < 0, vocab < 1, ld < vocab, an odd logits address, any other array that is not 4-byte
 *   aligned, a workspace that is null, too small or not 8-byte aligned: MM_ERR_BAD_ARG.  vocab > MM_ARGMAX_MAX_VOCAB or
 *   rows > MM_ARGMAX_MAX_ROWS: MM_ERR_UNSUPPORTED.  rows == 0: MM_OK.  All without device work.
 */
size_t mm_sample_rows_workspace_bytes(int rows, int vocab);
int mm_sample_rows(const void *logits_bf16, int rows, int vocab, long long ld /* elements between rows, >= vocab */,
                   const float *u /* [rows] */, const float *temperature /* [rows] or null: 1.0 */,
                   const int32_t *top_k /* [rows] or null: off */, const float *top_p /* [rows] or null: off */,
                   const float *min_p /* [rows] or null: off */, int32_t *out_idx /* [rows] */, void *workspace, size_t workspace_bytes,
                   mm_stream_t stream);

/*
 * Shared-prefix decode over the paged KV cache (detect the two entries by their symbols; mm_version stays 660): mm_paged_decode for a
 * batch in which groups of sequences hold a leading run of pages in common (n samples of one prompt, beams, a system prompt;
 * PagedKVCache.fork).  The result is the same function as mm_paged_decode -- every sequence attends all of its own tokens -- within the
 * same error budget (the sums run in another order, so not the same bits).  The shared tokens are walked once per slab of
 * floor(16 / g) group members, whose queries fill the rows of one MFMA operand that g heads leave idle; every sequence's own tail is
 * walked on its own.  q, the cache, the page table, head rules, sm_scale and o as mm_paged_decode.
 *   group_indptr [batch + 1], group_members [batch], shared_len [batch]: int32 device arrays of fixed size, read by the kernels only,
 *   so one captured graph stays valid while the sharing changes between replays.  Group j is
 *   group_members[group_indptr[j] .. group_indptr[j + 1]); unused trailing groups are empty (group_indptr[j] = batch); group_members is
 *   a permutation of 0 .. batch - 1.  shared_len[b] is the number of leading tokens sequence b has on the same pages as the other
 *   members of its group: the same value for every member, at most every member's length, not necessarily a multiple of the page size
 *   (right after a fork the partly filled last page is shared too).  A sequence that shares nothing is a group of one with shared_len 0.
 *   The shared tokens are read through the page list of a slab's first member.
 *   When the arrays break these rules the results of the affected sequences are unspecified, and nothing is read or written outside
 *   the cache, the tables, the workspace and o: member indices outside [0, batch) are ignored, a walk never passes the length of the
 *   sequence whose page list it reads, and page numbers outside [0, max_pages) are skipped as everywhere else.
 *   max_shared_len bounds the shared counts and max_suffix_len the tails (length - shared count), each in [0, 2^29].  The two chunk
 *   counts and the workspace size depend on (batch, Hq, Hkv, max_shared_len, max_suffix_len) alone; the last chunk of either range runs
 *   to the real end, whatever the bound said.  The call always goes through `workspace` (mm_paged_decode_shared_workspace_bytes, never 0
 *   for arguments the call accepts with batch > 0; 16-byte aligned, not shared with a concurrent call): three launches, prefix, tails,
 *   merge.  No host read of a device array: capture-safe.
 *   No sliding window here: every member's window begins at a different place, which is a different problem.
 * Null pointers, bad sizes, Hq not a multiple of Hkv, a bound outside [0, 2^29], a missing, small or misaligned workspace:
 * MM_ERR_BAD_ARG; head_dim != 128 or g > 16: MM_ERR_UNSUPPORTED; batch = 0: MM_OK; all without device work.
 */
size_t mm_paged_decode_shared_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int max_shared_len, int max_suffix_len);
int mm_paged_decode_shared(const void *q_bf16, const void *kv_data, const void *kv_param, int kv_dtype, int max_pages, int num_layers,
                           int layer, int num_kv_heads, int page_size, int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices,
                           const int32_t *last_page_len, int batch, int num_qo_heads, const int32_t *group_indptr /* [batch + 1] */,
                           const int32_t *group_members /* [batch] */, const int32_t *shared_len /* [batch], per sequence */,
                           int max_shared_len, int max_suffix_len, float sm_scale, void *workspace, size_t workspace_bytes, void *o_bf16,
                           mm_stream_t stream);

/*
 * Sparse MoE block around mm_reorder_quantize_grouped / mm_matmul_grouped (version >= 630): top-k routing of the gate logits, the
 * dispatch plan, the row gather and the weighted combine (the reference's MixtralSparseMoeBlock.forward, qMixtralLayer.py:414-452,
 * without its per-expert host loop).  T tokens, E experts, n = T * top_k (token, k-slot) pairs, pair p = t * top_k + j.
 * Limits: 1 <= top_k <= 8, top_k <= E <= 64, n < 2^31, H a multiple of 8 (rows move as 16-byte vectors; bf16 row pointers 16-byte
 * aligned): otherwise MM_ERR_UNSUPPORTED.  Null or misaligned pointers, negative sizes: MM_ERR_BAD_ARG.  T = 0 (or no rows, H = 0):
 * MM_OK without device work.  All four run on `stream`, read nothing on the host, need no workspace and no zeroed state
 * (capture-safe), use no atomic that could decide an order: two launches on the same input give the same bytes.
 *
 * mm_moe_route: logits bf16 [T, E] -> topk_ids int32 [T, top_k], topk_w bf16 [T, top_k].  The top_k largest logits in descending
 *   order, equal logits (-0.0 = +0.0) in ascending expert index.  w_j = exp(l_j - m) / sum over the selected of exp(l_i - m) in fp32,
 *   m the largest logit, rounded to bf16 to nearest even: softmax -> topk -> renormalise -> cast, always renormalised.
 * mm_moe_plan: topk_ids -> expert_offsets int32 [E + 1], sorted_token int32 [n], slot_of int32 [T, top_k].  A stable counting sort
 *   of the pairs by expert: expert e owns the slots [expert_offsets[e], expert_offsets[e + 1]), within an expert the slots run by
 *   ascending pair (so by ascending token), sorted_token[s] is the token of slot s and slot_of[t, j] its inverse.  An id outside
 *   [0, E) is not counted and gets slot_of = -1; the slots from expert_offsets[E] on, which no pair owns then, get sorted_token = -1.
 * mm_moe_gather: x bf16 [T, H], sorted_token [num_rows] -> x_sorted bf16 [num_rows, H]: x_sorted[s] = x[sorted_token[s]]; a row
 *   whose sorted_token lies outside [0, T) is left untouched.
 * mm_moe_combine: y_sorted bf16 [n, H], topk_ids, topk_w, slot_of -> out bf16 [T, H].  Per token its top_k entries in ascending
 *   expert id (equal ids: ascending k-slot): c = bf16(y_sorted[slot] * w) (the fp32 product of two bf16 values is exact), acc =
 *   bf16(acc + c) from +0.0, every rounding to nearest even -- what zeros + index_add_ expert by expert gives.  Entries with
 *   slot_of outside [0, n) are skipped; a token with none gets zeros.  Every row of out is written.
 */
int mm_moe_route(const void *logits_bf16, int num_tokens, int num_experts, int top_k, int32_t *topk_ids, void *topk_w_bf16,
                 mm_stream_t stream);
int mm_moe_plan(const int32_t *topk_ids, int num_tokens, int num_experts, int top_k, int32_t *expert_offsets, int32_t *sorted_token,
                int32_t *slot_of, mm_stream_t stream);
int mm_moe_gather(const void *x_bf16, const int32_t *sorted_token, int num_tokens, int num_rows, int hidden, void *x_sorted_bf16,
                  mm_stream_t stream);
int mm_moe_combine(const void *y_sorted_bf16, const int32_t *topk_ids, const void *topk_w_bf16, const int32_t *slot_of, int num_tokens,
                   int top_k, int hidden, void *out_bf16, mm_stream_t stream);

/*
 * Device-sized grouped launches (version >= 640): the expert quantizer and the expert GEMM of a sparse MoE block with the row counts read
 * from expert_offsets ON THE DEVICE, so that the block needs no copy to the host and can be captured in a hipGraph.  Both entries take
 * no workspace, read no device data on the host, use no atomic to decide an order and give the same bytes on every launch; their
 * grids depend on host values only.  E experts, 1 <= E <= 64 (else MM_ERR_UNSUPPORTED); n = num_rows rows ("slots") in plan order;
 * expert e owns the slots [expert_offsets[e], expert_offsets[e + 1]) (mm_moe_plan's output).
 *
 * Data format -- one set of buffers per quantized operand for ALL experts:
 *   packed segments  [n, Kseg / 2 | 3 Kseg / 4 | Kseg] row-major; expert e's rows are rows expert_offsets[e] .. of it: the bytes of
 *                    the per-expert tensors of mm_reorder_quantize_grouped laid end to end.
 *   scale tensors    the layout above is tiled per 128 rows OF A GROUP, so every expert has its own run of 128-row tiles (a tile of a
 *                    segment is 128 * Kseg / 32 bytes).  Expert e's run starts at tile
 *                        expert_offsets[e] / 128 + e            (integer division)
 *                    and is ceil(M_e / 128) tiles long.  A pure function of expert_offsets[e]: no scan.  The runs are disjoint for any
 *                    non-decreasing offsets, because floor(lo / 128) + ceil(M / 128) <= floor(hi / 128) + 1, and they lie inside
 *                    n / 128 + E tiles: mm_moe_sf_bytes(n, E, Kseg) bytes is the allocation.  Inside its run an expert's scale bytes are
 *                    those of its own [M_e, Kseg] scale tensor (mm_sf_offset from the run's first byte).
 *   expert table     mm_moe_expert[E] in DEVICE memory (8-byte aligned), built once: the expert's reorder index (mm_moe_quantize reads
 *                    only this), its packed weights and scales and an optional bias (mm_moe_matmul reads these).  One table per layer
 *                    (w1, w3, w2).  The pointers must stay valid while launches that read the table run.
 *
 * mm_moe_quantize: for every slot s that an expert owns, quantizes row row_of_slot[s] of src (bf16 [src_rows, K]; row s itself when
 *   row_of_slot is NULL) with that expert's reorder index, as mm_reorder_quantize does, into packed row s and the scale bytes of row
 *   s - expert_offsets[e] of the expert's run.  With row_of_slot = mm_moe_plan's sorted_token this is mm_moe_gather folded in.  A slot
 *   from expert_offsets[E] on, offsets that are not a plan's (decreasing, negative, past n), or a row index outside [0, src_rows) leave
 *   that slot's outputs untouched; nothing is read or written out of bounds.  src and the packed outputs 16-byte aligned, scale tensors
 *   4-byte aligned.  mode: MM_QUANT_MIXED or MM_QUANT_W4.
 * mm_moe_activate_quantize (version >= 650): the activation of the expert MLP computed while the quantizer stages the row.  a, b bf16
 *   [n, K] with rows in slot order (the experts' two up-projections).  For every slot s that an expert owns, in mm_moe_quantize's sense,
 *       h[s, c] = bf16( float(bf16( silu(a[s, c]) )) * float(b[s, c]) ),     silu(x) = x * rcp(1 + exp2(-x log2 e)) in fp32,
 *   both roundings to nearest even -- torch's bf16 `silu(a) * b`, which rounds twice, except where the hardware exp2 / rcp (about one
 *   fp32 ulp each) move silu across a bf16 rounding boundary: fewer than 1 element in 1 000 differs from the correctly rounded result,
 *   none by more than 3 bf16 ulps (1 ulp when b = 1).  Row h[s, :] is then quantized exactly as mm_moe_quantize(h, NULL, ..,
 *   MM_QUANT_MIXED) would: the same six buffers, byte for byte, which mm_moe_matmul consumes.  h_out_bf16, when not NULL, also receives
 *   the bf16 row, unreordered ([n, K]; it must not overlap a or b).  A slot no expert owns, offsets that are not a plan's or a slot from
 *   expert_offsets[E] on leave every output of that slot untouched, h_out included; the scale tile written is at most s / 128 + E - 1.
 *   a, b, h_out and the packed outputs 16-byte aligned, scale tensors 4-byte aligned.  One launch, no workspace.
 * mm_moe_matmul: D[slots of e] = the product mm_matmul_grouped computes for group e, on the same kernel family -- bit for bit when
 *   K <= 512, for an expert of more than 64 rows, and whenever the two streaming launches split K over the same number of waves (4 when
 *   ceil(N / 32) * groups >= CUs and the tier is above 16 rows, else 8; here tier and groups come from max_rows and min(E, n, 8), there
 *   from the largest group and the number of groups of at most 64 rows in each launch); otherwise the fp32 partial sums of an expert of
 *   at most 64 rows are added in another order.  The result depends on (max_rows, the expert's rows) alone.  A / SFA the buffers
 *   mm_moe_quantize (MM_QUANT_MIXED) filled, weights and bias from the table, D bf16 [n, N].  max_rows is a host bound on any expert's rows that the
 *   caller vouches for (a MoE block passes T: a token meets an expert at most once).  Experts of 1 .. 64 rows run in one launch of the
 *   weight-streaming kernels (at the tier of min(max_rows, 64)), experts of more than 64 rows, when max_rows > 64, in one launch of the
 *   tiled kernels whose grid is the host bound (n / bm + min(E, n)) * ceil(N / bn) on the sum of their tiles; an expert finds itself in
 *   one launch and leaves the other at once.  An expert with more than max_rows rows is skipped whole: its D rows stay untouched.
 *   KN + KS + KO == 0 writes zeros to the owned rows.  MM_OUT_F32 and shapes whose scale images do not fit the streaming kernels' LDS at some
 *   tier up to min(max_rows, 64)'s (mm_moe_matmul_supported() == 0; the caller then takes mm_matmul_grouped): MM_ERR_UNSUPPORTED.
 * mm_moe_gate_up_activate (detect it by the symbol; mm_version stays 660): both up-projections, the activation and the quantizer of the
 *   down-projection in ONE launch of the tiled kernels.  A / SFA the buffers mm_moe_quantize (MM_QUANT_MIXED) filled with w1's split
 *   (KN, KS, KO).  gate_up_table: per expert the fp4-packed weight of N = 2 I rows whose gate half is w1 and whose up half is w3, both
 *   with their rows in the order of the expert's w2 reorder index (row j = row idx2[j]) and then interleaved per 128 rows as
 *   mm_gate_up_activate takes them; no bias.  (DN, DS, DO) is w2's split of the I features.  For every slot s that an expert with
 *   1 .. max_rows rows owns,
 *       h[s, j] = bf16( float(bf16( silu(a[s, idx2[j]]) )) * float(b[s, idx2[j]]) )
 *   with a, b the bf16 rows that the tiled kernels without split-K give the expert for w1 and w3 (mm_moe_matmul's own rows for an
 *   expert of more than 64 rows; below that mm_moe_matmul streams the weights and may add its fp32 partial sums in another order),
 *   quantized into packed row s and the expert's run of scale tiles: for owned rows byte for byte the six buffers that
 *   mm_moe_activate_quantize(a, b, ..) with w2's table fills.  The scale bytes of rows past M_e inside the expert's own tiles are
 *   unspecified (whole 512-byte atoms are written); everything outside the experts' rows and runs keeps its bytes; an expert above
 *   max_rows, or one whose offsets are negative, decreasing or past n, is skipped whole.  The grid is the host bound
 *   (n / bm + min(E, n)) * (2 I / 256): 128-row tiles while that fits one round of workgroups, else 256-row tiles
 *   (mm_moe_gate_up_activate_describe).  flags: MM_ROUND_ONCE or 0.  I and DN, DS, DO multiples of 128; the packed outputs and the
 *   scale tensors 16-byte aligned.  mm_moe_gate_up_activate_supported: 0 for max_rows < 1, a bad split, or weights that are not fp4.
 * Null or misaligned pointers, negative sizes: MM_ERR_BAD_ARG; a bad split: MM_ERR_BAD_SPLIT; n = 0: MM_OK; all without device work.
 */
typedef struct mm_moe_expert {
    const int16_t *reorder_index;                 /* [K] */
    const uint8_t *BN, *BS, *BO;                  /* packed weights [N, .] */
    const uint8_t *SFBN, *SFBS, *SFBO;            /* their scales */
    const void *bias_bf16;                        /* [N] or NULL */
} mm_moe_expert;
size_t mm_moe_sf_bytes(int num_rows, int num_experts, int Kseg);
int mm_moe_quantize(const void *src_bf16, const int32_t *row_of_slot, const int32_t *expert_offsets, const mm_moe_expert *expert_table,
                    int num_experts, int num_rows, int src_rows, int K, int KN, int KS, int KO, int mode, uint8_t *oN, uint8_t *oS,
                    uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, mm_stream_t stream);
int mm_moe_activate_quantize(const void *a_bf16, const void *b_bf16, const int32_t *expert_offsets, const mm_moe_expert *expert_table,
                             int num_experts, int num_rows, int K, int KN, int KS, int KO, uint8_t *oN, uint8_t *oS, uint8_t *oO,
                             uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, void *h_out_bf16, mm_stream_t stream);
int mm_moe_matmul_supported(int max_rows, int N, int KN, int KS, int KO, int wmode);
int mm_moe_matmul(const uint8_t *AN, const uint8_t *AS, const uint8_t *AO, const uint8_t *SFAN, const uint8_t *SFAS, const uint8_t *SFAO,
                  const int32_t *expert_offsets, const mm_moe_expert *expert_table, int num_experts, int num_rows, int max_rows, int N,
                  int KN, int KS, int KO, int wmode, int flags, void *D_bf16, mm_stream_t stream);
int mm_moe_gate_up_activate_supported(int max_rows, int I, int KN, int KS, int KO, int DN, int DS, int DO, int wmode);
const char *mm_moe_gate_up_activate_describe(int num_experts, int num_rows, int I);
int mm_moe_gate_up_activate(const uint8_t *AN, const uint8_t *AS, const uint8_t *AO, const uint8_t *SFAN, const uint8_t *SFAS, const uint8_t *SFAO,
                            const int32_t *expert_offsets, const mm_moe_expert *gate_up_table, int num_experts, int num_rows, int max_rows, int I,
                            int KN, int KS, int KO, int DN, int DS, int DO, int flags, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN,
                            uint8_t *sfS, uint8_t *sfO, mm_stream_t stream);

/* Which kernel(s) and how many workgroups mm_matmul / mm_matmul_ws launch for this problem on the CURRENT device (the same
 * decision code as the launcher; workspace_bytes = 0 means "no workspace", i.e. never split-K).  Returns a string in a
 * thread-local buffer, valid until the calling thread's next call.  Used by bench.py to name the kernel it timed. */
const char *mm_matmul_describe(int M, int N, int KN, int KS, int KO, int wmode, int flags, size_t workspace_bytes);

/* bindings.cpp:700 `m.def("test_function", ...)`: the reference module's liveness probe; returns the same constant string. */
const char *mm_test_function(void);

/*
 * Measurement hook -- UNSTABLE, not part of the drop-in interface (no reference counterpart; bench.py and tools/ use it; it changes
 * no result).  THREAD-LOCAL: it affects only launches made by the calling thread.
 *
 * mm_diag_set_kernel_events: while a pair of hipEvent_t is registered, every tiled-GEMM launch (M > 64, and the M > 32 shapes that
 *   run on tiles; mm_gate_up_activate's fused launch) and every quantizer launch (mm_reorder_quantize, mm_rmsnorm_quantize,
 *   mm_activate_quantize, mm_downproj_quantize) of this thread attaches them to its own dispatch (hipExtLaunchKernel start/stop events), so hipEventElapsedTime
 *   gives the kernel's duration as rocprofv3 reports it, without the launch gap that events recorded around the call include.
 *   NULL, NULL disables.  Host-side only: the kernels are the same with and without it.
 *
 * The in-kernel clock stamps (mm_diag_set_clock_buffer) and the MM_DBG ablation switches exist only in the instrumented
 * developer variant of the library (-DMM_INSTRUMENT, csrc/mx_instrument.h, tools/build_variant.sh); the default library neither
 * exports that symbol nor contains the stores.  The hardware microbenchmarks and probes (mm_diag_mfma, mm_diag_hw_convert,
 * mm_diag_mfma_rate, mm_diag_l2_bw, mm_diag_stream_once) live in libmicromix_diag.so, declared in include/micromix_diag.h.
 */
int mm_diag_set_kernel_events(void *start_event, void *stop_event);
#ifdef MM_INSTRUMENT
/* device buffer of 4 x 8 bytes per workgroup: {main-loop s_memtime delta, main-loop s_memrealtime delta, start tick,
 * end-of-epilogue tick delta} of every workgroup of the large-M GEMM (in-kernel clock = ratio x 100 MHz); NULL disables.
 * The ping-pong kernel also writes its head -- {shader cycles from the start stamp to wave 0's first DMA request, ... to its first
 * MFMA} -- to row 2048 + workgroup when it has at most 2048 workgroups: give it a buffer of at least 4096 rows. */
int mm_diag_set_clock_buffer(void *buf);
/* device buffer of 4 x 8 bytes per workgroup of reorder_quantize_kernel: {start, row staged, first group stored, end} ticks */
int mm_diag_set_quant_clock_buffer(void *buf);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MICROMIX_HIP_H */
