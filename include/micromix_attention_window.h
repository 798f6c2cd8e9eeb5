/*
 * micromix_attention_window.h -- the sliding-window form of mm_dense_attention (micromix_attention.h): dense causal GQA attention over
 * contiguous bf16 q, k, v in which a token attends the last `window` tokens of its sequence only, HF's sliding_window (Mistral, Qwen2
 * layers with sliding_window), as mm_paged_prefill_window has it over a paged cache.
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The status
 * codes are micromix_hip.h's.  micromix_amd/paged.py (dense_attention_window) is the Python side; csrc/dense_attention.hip holds the
 * kernel, the window instantiation of mm_dense_attention's.
 *
 * mm_dense_attention_window.  Every argument up to `stream` is mm_dense_attention's, in its order and with its meaning: layouts, strides,
 * seq_indptr, heads, arithmetic, capture (the same grid from host values alone, no workspace: with window >= 1 every row attends
 * itself, so no row is empty), tiles and limits are stated there.
 *   Mask      token i of a sequence attends tokens max(0, i - window + 1) .. i of that sequence.
 *   Same bits window >= total_tokens launches mm_dense_attention's own kernel.  Below that, a sequence no longer than window comes out
 *             bit-equal to mm_dense_attention's: its masks never bind and its walk starts at its first token.
 *   Walk      a workgroup (MM_DENSE_ATTN_BQ query tokens from token i0 of a sequence) walks the kv tiles from tile
 *             max(0, i0 - window + 1) / MM_DENSE_ATTN_BK up to its diagonal: a query tile past the window visits about
 *             (window + MM_DENSE_ATTN_BQ) / MM_DENSE_ATTN_BK tiles however long the sequence is.
 *   Reads     only tokens of the row's own sequence, from the first tile of that walk on.  A token below a row's window inside a visited
 *             tile enters with a masked score and p = 0: finite values there leave the row's bits unchanged, non-finite values there
 *             may reach it (p.V is 0 * v), as a non-finite row above a row's diagonal inside its kv tile may in mm_dense_attention.
 *             Nothing of another sequence is ever read, and nothing below the first tile of the walk.
 *
 * Statuses, all without device work: mm_dense_attention's, unchanged and in its order, and window < 1: MM_ERR_BAD_ARG, checked with its
 * first argument checks (ahead of MM_ERR_UNSUPPORTED and of the MM_OK of total_tokens == 0 or batch == 0).
 */
#ifndef MICROMIX_ATTENTION_WINDOW_H
#define MICROMIX_ATTENTION_WINDOW_H
#include "micromix_attention.h"
#ifdef __cplusplus
extern "C" {
#endif

int mm_dense_attention_window(const void *q, const void *k, const void *v, long long q_stride, long long k_stride, long long v_stride,
                              const int32_t *seq_indptr /* device, [batch + 1] */, int batch, int total_tokens, int num_q_heads,
                              int num_kv_heads, int head_dim, float sm_scale, void *o /* bf16 [total_tokens, Hq, 128] contiguous */,
                              mm_stream_t stream, int window);

#ifdef __cplusplus
}
#endif
#endif
