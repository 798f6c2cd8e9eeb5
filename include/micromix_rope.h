/*
 * micromix_rope.h -- RoPE and the paged KV append in the shape of a prompt: mm_rope_kv_append (micromix_hip.h) for many tokens at a
 * time, with the outputs that let a fresh prompt run on mm_dense_attention (micromix_attention.h) with or without a cache.
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The status
 * codes are micromix_hip.h's.  micromix_amd/paged.py (rope_qk, rope_kv_append_dense) is the Python side; csrc/rope_prefill.hip is the kernel.
 *
 * mm_rope_prefill.  q, k, v, cos, sin, the strides, num_qo_heads, append_indptr and num_tokens = T are mm_rope_kv_append's: three bf16
 * pointers that share the token stride qkv_token_stride (elements), heads contiguous within a token; cos, sin bf16 [T, 128] with row
 * stride cs_token_stride, row i for flat token i, both halves of a row read (a table need not repeat its halves).
 *   q_out     bf16 [T, Hq, 128] contiguous, required: HF's bf16 apply_rotary_pos_emb of q, bit for bit, for every token -- the element
 *             rule stated under mm_rope_kv_append:  a = bf16(x[d] * cos[d]);  b = bf16((d < 64 ? -x[d + 64] : x[d - 64]) * sin[d]);
 *             y[d] = bf16(a + b), in fp32, round to nearest even, finite inputs.
 *   Cache     kv_data != NULL: the cache (kv_data .. batch, as mm_rope_kv_append takes them) receives exactly the bytes mm_rope_kv_append
 *             writes for the same arguments: rope(k) and v by the same slot rule (append_indptr, a page table that already counts the
 *             tokens), the same int4 / fp8 rule or bf16 copy, the same guards, nothing outside the target slots.  A token without a
 *             valid slot writes nothing there and still gets its q_out, k_out and v_out.
 *             kv_data == NULL: no cache.  kv_param .. batch and append_indptr are not looked at (append_indptr may be NULL); only
 *             num_kv_heads and head_dim count.  This form is plain RoPE of q and k.
 *   k_out     bf16 [T, Hkv, 128] contiguous, or NULL (not written): for every token and kv head the bf16 value a reader of the slot gets
 *   v_out     back, of rope(k) and of v:
 *               bf16 kind, or no cache   the value itself: rope(k), and v as given
 *               fp8                      code * 2^e, which is exactly a bf16 number
 *               int4                     bf16_rne(fp32(code) * fp32(scale) - fp32(zero)) with the row's stored fp16 (scale, zero): the
 *                                        product is exact in fp32, the subtraction one fp32 rounding, then one bf16 rounding -- the bf16
 *                                        tensor the reference's quantize_int_group hands its attention
 *             A caller with a bf16 cache or none passes v_out = NULL and attends v in place.
 *   Capture   no workspace, no host read of a device array, a grid of ceil(T / MM_ROPE_PREFILL_TOKENS) workgroups: capture-safe; a captured
 *             graph replays with another split of the same T.
 *   Tiles     a workgroup owns MM_ROPE_PREFILL_TOKENS consecutive tokens; published for tests that want to stand on the edges.
 *
 * Limits: head_dim 128; any g = Hq / Hkv >= 1; q, k, v, cos, sin, q_out, k_out, v_out and kv_data 16-byte aligned, kv_param and the
 * int32 arrays 4-byte aligned; both strides a multiple of 8 elements and at least the row they hold (Hq * 128; 128).  The outputs must
 * not overlap the inputs or each other.  Offsets are 64-bit throughout.
 *
 * Statuses, all without device work.  MM_ERR_BAD_ARG: num_tokens < 0, num_qo_heads < 1, num_kv_heads < 1, num_qo_heads no multiple of
 * num_kv_heads, a stride that is no multiple of 8 or smaller than its row; with a cache, whatever mm_rope_kv_append refuses in the cache's
 * geometry (an unassigned kv_dtype, non-positive sizes, a layer outside the cache); with num_tokens > 0: a null or misaligned q, k, v,
 * cos, sin or q_out, a misaligned k_out or v_out, and with a cache batch == 0 (tokens that belong to no sequence), a null kv_param for
 * int4 / fp8, a null page-table array or append_indptr, a misaligned kv_data, kv_param or append_indptr.
 * MM_ERR_UNSUPPORTED: head_dim != 128.  num_tokens == 0 (with arguments the lines above do not refuse): MM_OK.
 */
#ifndef MICROMIX_ROPE_H
#define MICROMIX_ROPE_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MM_ROPE_PREFILL_TOKENS 8

int mm_rope_prefill(void *kv_data /* or NULL: no cache */, void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer,
                    int num_kv_heads, int page_size, int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices,
                    const int32_t *last_page_len, int batch, const void *q_bf16, const void *k_bf16, const void *v_bf16,
                    int64_t qkv_token_stride, int num_qo_heads, const void *cos_bf16, const void *sin_bf16, int64_t cs_token_stride,
                    const int32_t *append_indptr, int num_tokens, void *q_out_bf16, void *k_out_bf16 /* or NULL */,
                    void *v_out_bf16 /* or NULL */, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
