/*
 * micromix_kv_prefill_hd64.h -- causal multi-token attention over the paged KV cache for 64-wide heads: what mm_paged_prefill
 * (micromix_hip.h) is for 128-wide heads, over the cache of micromix_kv_hd64.h.  A chunk of a chunked prompt, a new turn over a cached
 * conversation, the verification of a chain draft.  The kernel is its own (csrc/kv_prefill_hd64.hip).
 *
 * Exported from libmicromix_hip.so and detected by symbol; mm_version() does not change.  The status codes are micromix_hip.h's.
 * mixedgemm.paged_prefill given a cache whose rows are 64 wide and PagedKVCache(head_dim=64).attend_new are the Python side.
 *
 * mm_paged_prefill_hd64.  q bf16 [T, Hq, 64] -> o bf16 [T, Hq, 64], rounded once, over layer `layer` of the cache (layout and page
 * table: micromix_kv_hd64.h; MM_KV_BF16 and MM_KV_FP8_E4M3, any page_size >= 1).
 *   Tokens     qo_indptr [batch + 1] (int32, device; the append_indptr of mm_rope_kv_append_hd64) splits the T queries among the
 *              sequences.  The page table already counts the new tokens.  The mask is causal, aligned bottom-right: the j-th of
 *              sequence b's n_b tokens sits at position len_b - n_b + j and attends positions 0 .. that one.  A query at a negative
 *              position (a table that does not count the new tokens) gives zeros, and so does a sequence of length 0.
 *   Heads      Hq = g * Hkv with g <= 16; query head h reads kv head h / g (HF repeat_kv).
 *   Arithmetic scores q.k on the matrix unit from the bf16 values (fp8: from decode(code) * 2^e, exact in bf16), fp32 accumulation;
 *              online softmax in fp32 in the log2 domain with sm_scale (<= 0: 1 / sqrt(64)); p rounded to bf16 for p.V on the matrix
 *              unit, fp32 accumulation, the sum of p taken in fp32 before that rounding.  Over an fp8 cache the result equals, bit for
 *              bit, that over a bf16 cache holding the dequantized values.
 *   Lengths    a sequence longer than max_seq_len is still attended in full: the last chunk runs to the sequence's end.  A token on a
 *              page outside [0, max_pages) is not attended.
 *   Plan       from host values only -- T, batch, Hq, Hkv, max_seq_len --, so a captured graph of append + attention stays valid over
 *              later steps with the same T.  mm_paged_prefill_hd64_plan publishes it.  rows: the (token, head) rows of a workgroup,
 *              MM_KV_PREFILL_HD64_ROWS_FEW = 64 when T * g <= 64 * batch (speculative widths: a sequence's tokens and heads fill at
 *              most half a large tile on average), else MM_KV_PREFILL_HD64_ROWS = 128.  tile_tokens = rows / g (floor) query tokens
 *              of one sequence per tile; tiles = T / tile_tokens + batch, which bounds sum ceil(n_b / tile_tokens) -- sequence b owns
 *              tiles [qo_indptr[b] / tile_tokens + b, ...), found on the device, surplus tiles exit.  chunks and chunk_len:
 *              mm_paged_prefill's rule, chunks = min(ceil(1024 / (tiles * Hkv)), ceil(max_seq_len / 256)), at least 1; chunk_len =
 *              ceil(max_seq_len / chunks) rounded up to a multiple of MM_KV_PREFILL_HD64_TILE = 64; chunks = ceil(max_seq_len /
 *              chunk_len) again (1 for max_seq_len == 0).  Chunk c is positions [c * chunk_len, (c + 1) * chunk_len), the last to the end.
 *   Workspace  mm_paged_prefill_hd64_workspace_bytes: 0 for one chunk -- a single launch then writes o --, else tiles * Hkv * chunks *
 *              rows * 66 floats of (o[64], m, l) partials that a second, small launch merges.  It needs no initialisation, holds no
 *              tickets, and must be 16-byte aligned.  0 also for arguments mm_paged_prefill_hd64 refuses.
 *   Capture    nothing is read on the host and nothing allocated: capture-safe.
 * Statuses, all without device work.  MM_ERR_BAD_ARG: a kv_dtype that is no mm_kv_dtype, max_pages, num_layers, num_kv_heads,
 * page_size < 1, layer outside [0, num_layers), num_kv_heads > 65535, batch < 0 or > 65535, num_qo_heads < 1 or no multiple of
 * num_kv_heads, max_seq_len < 0, num_tokens < 0.  MM_ERR_UNSUPPORTED: MM_KV_INT4, g > 16.  num_tokens == 0 or batch == 0: MM_OK.  Then
 * MM_ERR_BAD_ARG: a null q, qo_indptr, o, kv_data, kv_param (fp8) or page-table array; q, o or kv_data not 16-byte aligned; kv_param
 * or an int32 array not 4-byte aligned; a workspace that is needed and null, smaller than mm_paged_prefill_hd64_workspace_bytes or not
 * 16-byte aligned.
 *
 * Out of scope: the sliding-window and tree-mask forms (mm_paged_prefill_window, mm_paged_prefill_tree) for 64-wide rows.
 */
#ifndef MICROMIX_KV_PREFILL_HD64_H
#define MICROMIX_KV_PREFILL_HD64_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MM_KV_PREFILL_HD64_ROWS 128
#define MM_KV_PREFILL_HD64_ROWS_FEW 64
#define MM_KV_PREFILL_HD64_TILE 64

size_t mm_paged_prefill_hd64_workspace_bytes(int num_tokens, int batch, int num_qo_heads, int num_kv_heads, int max_seq_len);

/* the plan mm_paged_prefill_hd64 uses for these host values; MM_ERR_BAD_ARG for num_tokens < 0, batch, num_kv_heads, num_qo_heads < 1,
   num_qo_heads no multiple of num_kv_heads, max_seq_len < 0 or a null pointer; MM_ERR_UNSUPPORTED for g > 16 */
int mm_paged_prefill_hd64_plan(int num_tokens, int batch, int num_qo_heads, int num_kv_heads, int max_seq_len, int *rows,
                               int *tile_tokens, int *tiles, int *chunks, int *chunk_len);

int mm_paged_prefill_hd64(const void *q_bf16, const int32_t *qo_indptr, int num_tokens, const void *kv_data, const void *kv_param,
                          int kv_dtype, int max_pages, int num_layers, int layer, int num_kv_heads, int page_size,
                          const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_len, int batch, int num_qo_heads,
                          int max_seq_len, float sm_scale, void *workspace, size_t workspace_bytes, void *o_bf16, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
