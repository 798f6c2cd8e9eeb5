/*
 * micromix_attention.h -- dense causal GQA attention over contiguous bf16 q, k, v: the attention of a forward pass WITHOUT a KV cache
 * (the reference's default mode, scaled_dot_product_attention(q, k, v, is_causal=True) on what came out of the projections), the
 * fourth kind beside decode, paged prefill and tree (micromix_hip.h), which all read a paged cache.
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The status
 * codes are micromix_hip.h's.  micromix_amd/paged.py (dense_attention) is the Python side; csrc/dense_attention.hip is the kernel.
 *
 * mm_dense_attention.  q, k, v are bf16; token t, head h, element e of q lies at q[t * q_stride + h * 128 + e], and k, v likewise with
 * their strides and num_kv_heads heads: the strides are ELEMENTS BETWEEN TWO TOKENS, so q, k and v may be three views of one packed
 * [total_tokens, (Hq + 2 Hkv) * 128] projection, read in place.  o is bf16 [total_tokens, Hq, 128], contiguous.
 *   Sequences  seq_indptr (device, int32 [batch + 1]) splits the tokens: sequence b owns tokens seq_indptr[b] .. seq_indptr[b + 1] of all
 *              four arrays.  Entries are clamped to [0, total_tokens]; a sequence of length <= 0 writes nothing, and tokens that no
 *              sequence owns are not written.
 *   Mask       token i of a sequence attends tokens 0 .. i of that sequence (square causal); nothing of another sequence is read.
 *   Heads      query head h reads kv head h / (Hq / Hkv) (HF repeat_kv).
 *   Arithmetic scores q.k in fp32 from the bf16 values, softmax in fp32 with sm_scale (<= 0: 1 / sqrt(128)), the probabilities rounded to
 *              bf16 ahead of p.V (as the paged kernels do), fp32 accumulation, o rounded to bf16 once.
 *   Capture    seq_indptr is read on the device only and nothing is allocated: the grid is (total_tokens / MM_DENSE_ATTN_BQ + batch) * Hq
 *              workgroups, from host values alone, so a captured graph replays with another split of the same total_tokens.  No
 *              workspace: square causal attention over whole sequences needs no split along kv.
 *   Tiles      a workgroup owns MM_DENSE_ATTN_BQ query tokens of one (sequence, query head) and walks the kv tokens MM_DENSE_ATTN_BK at a
 *              time; the two are published for tests and tools that want to stand on the edges.
 *
 * Limits: head_dim 128; any g = Hq / Hkv >= 1 (the g workgroups of a kv head run next to each other and share K/V through L2; g is
 * not bounded); each stride a multiple of 8 elements, at least its heads * 128 and at most MM_DENSE_ATTN_MAX_STRIDE; q, k, v, o 16-byte
 * aligned; (total_tokens / MM_DENSE_ATTN_BQ + batch) * Hq < 2^31.  Offsets are 64-bit throughout: total_tokens * stride may pass 2^31.
 *
 * Statuses, all without device work.  MM_ERR_BAD_ARG: total_tokens < 0, batch < 0, num_q_heads < 1, num_kv_heads < 1; with work to do
 * (total_tokens > 0 and batch > 0): a null q, k, v, o or seq_indptr, a base not 16-byte aligned, seq_indptr not 4-byte aligned, a
 * stride that is no multiple of 8 or smaller than its heads * 128.  MM_ERR_UNSUPPORTED, for arguments the lines above do not refuse:
 * head_dim != 128, num_q_heads no multiple of num_kv_heads, a stride above MM_DENSE_ATTN_MAX_STRIDE, a grid of 2^31 workgroups or more.
 * total_tokens == 0 or batch == 0: MM_OK.
 */
#ifndef MICROMIX_ATTENTION_H
#define MICROMIX_ATTENTION_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MM_DENSE_ATTN_BQ 128
#define MM_DENSE_ATTN_BK 64
#define MM_DENSE_ATTN_MAX_STRIDE (1 << 22)

int mm_dense_attention(const void *q, const void *k, const void *v, long long q_stride, long long k_stride, long long v_stride,
                       const int32_t *seq_indptr /* device, [batch + 1] */, int batch, int total_tokens, int num_q_heads, int num_kv_heads,
                       int head_dim, float sm_scale, void *o /* bf16 [total_tokens, Hq, 128] contiguous */, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
