/*
 * micromix_attention_hd64.h -- the cache-less route of a forward pass for 64-wide heads (Llama-3.2-1B, Qwen2.5-0.5B): RoPE of q and k and
 * dense causal GQA attention over contiguous bf16 q, k, v, what mm_rope_prefill without a cache (micromix_rope.h), mm_dense_attention
 * (micromix_attention.h) and mm_dense_attention_window (micromix_attention_window.h) are for 128-wide heads.  Those entries keep
 * answering MM_ERR_UNSUPPORTED for head_dim 64: the dimension arrives as the two entries below, with kernels of their own.
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The status
 * codes are micromix_hip.h's.  micromix_amd/paged.py (dense_attention, dense_attention_window and rope_qk given [T, H, 64] tensors) is the
 * Python side; csrc/dense_attention_hd64.hip holds both kernels.
 *
 * Out of scope here: the paged cache.  Its append and decode for 64-wide rows are micromix_kv_hd64.h's; its prefill / tree / window
 * kernels, mm_dense_attention_prefix and mm_kv_gather_dense stay 128-only.
 *
 * mm_dense_attention_hd64.  q, k, v are bf16; token t, head h, element e of q lies at q[t * q_stride + h * 64 + e], and k, v likewise with
 * their strides and num_kv_heads heads: the strides are ELEMENTS BETWEEN TWO TOKENS, so q, k and v may be three views of one packed
 * [total_tokens, (Hq + 2 Hkv) * 64] projection, read in place.  o is bf16 [total_tokens, Hq, 64], contiguous.
 *   Sequences  seq_indptr (device, int32 [batch + 1]) splits the tokens: sequence b owns tokens seq_indptr[b] .. seq_indptr[b + 1] of all
 *              four arrays.  Entries are clamped to [0, total_tokens]; a sequence of length <= 0 writes nothing, and tokens that no
 *              sequence owns are not written.
 *   Mask       window == 0: token i of a sequence attends tokens 0 .. i of that sequence (square causal).  window >= 1: HF's
 *              sliding_window, tokens max(0, i - window + 1) .. i.  Nothing of another sequence is read; with a window, nothing below the
 *              kv tile that holds the lower edge of the query tile's first row either.
 *   Same bits  window >= total_tokens launches the un-windowed kernel and gives its bits; below that, a sequence no longer than window
 *              comes out bit-equal to window == 0.
 *   Heads      query head h reads kv head h / (Hq / Hkv) (HF repeat_kv); g = Hq / Hkv is not bounded.
 *   Arithmetic scores q.k in fp32 from the bf16 values, softmax in fp32 with sm_scale (<= 0: 1 / sqrt(64)), the probabilities rounded to
 *              bf16 ahead of p.V, fp32 accumulation, o rounded to bf16 once.
 *   Capture    seq_indptr is read on the device only and nothing is allocated: the grid is
 *              (total_tokens / MM_DENSE_ATTN_HD64_BQ + batch) * Hq workgroups, from host values alone, so a captured graph replays with
 *              another split of the same total_tokens.  No workspace.
 *   Tiles      a workgroup owns MM_DENSE_ATTN_HD64_BQ query tokens of one (sequence, query head) and walks the kv tokens
 *              MM_DENSE_ATTN_HD64_BK at a time; published for tests and tools that want to stand on the edges.
 *
 * Limits: each stride a multiple of 8 elements, at least its heads * 64 and at most MM_DENSE_ATTN_HD64_MAX_STRIDE; q, k, v, o 16-byte
 * aligned; (total_tokens / MM_DENSE_ATTN_HD64_BQ + batch) * Hq < 2^31.  Offsets are 64-bit throughout.
 *
 * Statuses, all without device work.  MM_ERR_BAD_ARG: total_tokens < 0, batch < 0, num_q_heads < 1, num_kv_heads < 1, window < 0; with
 * work to do (total_tokens > 0 and batch > 0): a null q, k, v, o or seq_indptr, a base not 16-byte aligned, seq_indptr not 4-byte
 * aligned, a stride that is no multiple of 8 or smaller than its heads * 64.  MM_ERR_UNSUPPORTED, for arguments the lines above do not
 * refuse: num_q_heads no multiple of num_kv_heads, a stride above MM_DENSE_ATTN_HD64_MAX_STRIDE, a grid of 2^31 workgroups or more.
 * total_tokens == 0 or batch == 0: MM_OK.
 *
 * mm_rope_qk_hd64.  Plain RoPE of q and k, the cache-less form of mm_rope_prefill (kv_data == NULL) for 64-wide heads.  q and k are bf16
 * pointers that share the token stride qkv_token_stride (elements), heads contiguous within a token; cos, sin bf16 [T, 64] with row
 * stride cs_token_stride, row i for token i, both halves of a row read.  q_out is bf16 [T, Hq, 64] and k_out bf16 [T, Hkv, 64], both
 * contiguous and both required: HF's bf16 apply_rotary_pos_emb, bit for bit, by the element rule of micromix_rope.h with the partner
 * at d +- 32:  a = bf16(x[d] * cos[d]);  b = bf16((d < 32 ? -x[d + 32] : x[d - 32]) * sin[d]);  y[d] = bf16(a + b), in fp32, round to
 * nearest even, finite inputs.  No workspace, no device array read by the host, a grid of ceil(T / MM_ROPE_HD64_TOKENS) workgroups:
 * capture-safe.  A workgroup owns MM_ROPE_HD64_TOKENS consecutive tokens.  The outputs must not overlap the inputs or each other.
 *
 * Limits and statuses, all without device work, mm_rope_prefill's restated with 64.  MM_ERR_BAD_ARG: num_tokens < 0, num_qo_heads < 1,
 * num_kv_heads < 1, num_qo_heads no multiple of num_kv_heads, a stride that is no multiple of 8 or smaller than its row (Hq * 64; 64);
 * with num_tokens > 0: a null or not 16-byte aligned q, k, cos, sin, q_out or k_out.  num_tokens == 0 (with arguments the lines above
 * do not refuse): MM_OK.
 */
#ifndef MICROMIX_ATTENTION_HD64_H
#define MICROMIX_ATTENTION_HD64_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MM_DENSE_ATTN_HD64_BQ 128
#define MM_DENSE_ATTN_HD64_BK 64
#define MM_DENSE_ATTN_HD64_MAX_STRIDE (1 << 22)
#define MM_ROPE_HD64_TOKENS 16

int mm_dense_attention_hd64(const void *q, const void *k, const void *v, long long q_stride, long long k_stride, long long v_stride,
                            const int32_t *seq_indptr /* device, [batch + 1] */, int batch, int total_tokens, int num_q_heads,
                            int num_kv_heads, int window /* 0: none */, float sm_scale,
                            void *o /* bf16 [total_tokens, Hq, 64] contiguous */, mm_stream_t stream);

int mm_rope_qk_hd64(const void *q_bf16, const void *k_bf16, int64_t qkv_token_stride, int num_qo_heads, int num_kv_heads,
                    const void *cos_bf16, const void *sin_bf16, int64_t cs_token_stride, int num_tokens, void *q_out_bf16,
                    void *k_out_bf16, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
