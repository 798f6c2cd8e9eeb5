/*
 * micromix_qknorm.h -- Qwen3's QK-norm inside the three RoPE entries for 128-wide heads: mm_rope_kv_append (micromix_hip.h),
 * mm_rope_prefill (micromix_rope.h) and mm_rope_append_decode (micromix_decode_step.h), each with a per-head RMSNorm of q and of k
 * between the projection and the rotation (HF's Qwen3Attention.q_norm / k_norm: one bf16 weight of 128 each, shared by all heads).
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The status
 * codes are micromix_hip.h's.  micromix_amd/paged.py (the qk_norm= argument of rope_kv_append, rope_kv_append_dense, rope_qk,
 * rope_append_decode) and PagedKVCache (append_rope, prefill_fresh, decode_step) are the Python side; csrc/mx_qknorm.h holds the one
 * copy of the rule, the kernels are the parents' with NORM = true.
 *
 * The rule: HF's Qwen3RMSNorm followed by HF's bf16 RoPE.  For one 128-element bf16 row x of q or k, weight w (bf16 [128]) and eps:
 *   1  p[l] = x[2l]^2 + x[2l+1]^2 in fp32, l = 0 .. 63 (the squares are exact there: one rounding).
 *   2  S = the sum of the 64 p[l] in one fixed binary tree: partners whose index differs in bit 0 are added first, then bit 1, 2, 3,
 *      5, 4, in that order.  All three kernels realise this tree, so they agree bit for bit on every input.
 *   3  r = 1 / sqrt(S * 2^-7 + eps), the square root and the divide correctly rounded.
 *   4  n[d] = bf16_rne(fp32(x[d]) * r);  y[d] = bf16_rne(fp32(w[d]) * fp32(n[d])).
 *   5  y takes the place of x in the parent's RoPE element rule.  V, the slot rule and the int4 / fp8 / bf16 rules are the parent's.
 * Where fp32 addition is exact in any order -- HF's x.float().pow(2).mean(-1) sums in an order of its own -- the result is HF's bit
 * for bit; elsewhere S may differ from HF's in its last bits, as any two orders of 64 fp32 additions do, which rarely reaches a bf16
 * output (DESIGN 7ae counts it).  Finite inputs.
 *
 * Each entry takes its parent's arguments with q_norm_weight_bf16, k_norm_weight_bf16 (bf16 [128] each, 16-byte aligned, both required)
 * and norm_eps (finite, > 0; Qwen3: 1e-6) before the stream, and gives its parent's results for the normed q and k: the same outputs,
 * the same cache bytes, the same edges, capture-safe in the same way.  mm_rope_append_decode_qknorm's workspace is its parent's:
 * mm_rope_append_decode_workspace_bytes.
 *
 * Statuses, all without device work: the parent's, in the parent's order (so MM_ERR_UNSUPPORTED for a head_dim other than 128), and
 * MM_ERR_BAD_ARG for a norm_eps that is not finite and > 0, reported with the parent's other numbers (before a call with nothing to do
 * returns MM_OK), and for a null or not-16-byte-aligned weight, reported with the parent's pointers (only when there is work).
 *
 * Out of scope: norming only one of q and k, a weight per head, and 64-wide rows.
 */
#ifndef MICROMIX_QKNORM_H
#define MICROMIX_QKNORM_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int mm_rope_kv_append_qknorm(void *kv_data, void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer, int num_kv_heads,
                             int page_size, int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_len,
                             int batch, const void *q_bf16, const void *k_bf16, const void *v_bf16, int64_t qkv_token_stride,
                             int num_qo_heads, const void *cos_bf16, const void *sin_bf16, int64_t cs_token_stride,
                             const int32_t *append_indptr, int num_tokens, void *q_out_bf16, const void *q_norm_weight_bf16,
                             const void *k_norm_weight_bf16, float norm_eps, mm_stream_t stream);

int mm_rope_prefill_qknorm(void *kv_data /* or NULL: no cache */, void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer,
                           int num_kv_heads, int page_size, int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices,
                           const int32_t *last_page_len, int batch, const void *q_bf16, const void *k_bf16, const void *v_bf16,
                           int64_t qkv_token_stride, int num_qo_heads, const void *cos_bf16, const void *sin_bf16, int64_t cs_token_stride,
                           const int32_t *append_indptr, int num_tokens, void *q_out_bf16, void *k_out_bf16 /* or NULL */,
                           void *v_out_bf16 /* or NULL */, const void *q_norm_weight_bf16, const void *k_norm_weight_bf16, float norm_eps,
                           mm_stream_t stream);

int mm_rope_append_decode_qknorm(void *kv_data, void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer, int num_kv_heads,
                                 int page_size, int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices,
                                 const int32_t *last_page_len, int batch, const void *q_bf16, const void *k_bf16, const void *v_bf16,
                                 int64_t qkv_token_stride, int num_qo_heads, const void *cos_bf16, const void *sin_bf16,
                                 int64_t cs_token_stride, int max_seq_len, float sm_scale, void *workspace, size_t workspace_bytes,
                                 void *q_out_bf16, void *o_bf16, const void *q_norm_weight_bf16, const void *k_norm_weight_bf16,
                                 float norm_eps, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
