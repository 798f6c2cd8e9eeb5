/*
 * micromix_kv_hd64.h -- the paged KV cache for 64-wide heads (Llama-3.2-1B, Qwen2.5-0.5B): RoPE + append and split-KV decode attention,
 * what mm_rope_kv_append / mm_rope_prefill / mm_kv_append and mm_paged_decode (micromix_hip.h, micromix_rope.h) are for 128-wide heads.
 * Those entries keep answering MM_ERR_UNSUPPORTED for head_dim 64: the dimension arrives as the entries below, with kernels of their
 * own (csrc/kv_hd64.hip).  With micromix_attention_hd64.h a 64-wide model goes from prompt to decoded tokens on library calls only.
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The status
 * codes are micromix_hip.h's.  micromix_amd/paged.py (kv_append, rope_kv_append, rope_kv_append_dense, paged_decode given a cache whose
 * rows are 64 wide) and PagedKVCache(head_dim=64) are the Python side.
 *
 * Cache layout: the 128 layout of micromix_hip.h with rows of 64.
 *   MM_KV_BF16      kv_data bf16  [max_pages, L, 2, Hkv, P, 64]; kv_param is not read (NULL).
 *   MM_KV_FP8_E4M3  kv_data uint8 [max_pages, L, 2, Hkv, P, 64], OCP e4m3fn codes, element j in byte j; kv_param fp16
 *                   [max_pages, L, 2, Hkv, P, 2] = (2^e, +0.0).  The rule is the 128 cache's applied to a 64-value row: e is the smallest
 *                   integer in [-14, 15] with amax <= 448 * 2^e; the row is clamped to +-448 * 2^e first (only e = 15 can clamp), then
 *                   converted round-to-nearest-even; value = decode(code) * 2^e.  Finite inputs.
 *   MM_KV_INT4      MM_ERR_UNSUPPORTED: the reference's rule is one (scale, zero) group per 128 values, and a 64-value row has no such
 *                   group; a half group would be a format of this library's own invention.
 *   Page table      as in micromix_hip.h: kv_indptr [batch + 1], kv_indices, last_page_len [batch], int32 on the device; sequence b holds
 *                   pages kv_indices[kv_indptr[b] .. kv_indptr[b + 1]) and (pages - 1) * P + clamp(last_page_len[b], 0, P) tokens.  Any
 *                   page_size P >= 1.  Row offsets are 64-bit.
 *
 * mm_rope_kv_append_hd64.  RoPE of q and k, and the append of (rotated k, v) into layer `layer`, in one launch: mm_rope_kv_append,
 * mm_rope_prefill and -- without cos / sin -- mm_kv_append for 64-wide rows.  q, k, v are bf16 pointers that share the token stride
 * qkv_token_stride (elements), heads contiguous within a token; cos, sin bf16 [T, 64] with row stride cs_token_stride, row i for token i.
 *   RoPE     HF's bf16 apply_rotary_pos_emb by the element rule of micromix_rope.h with the partner at d +- 32:
 *            a = bf16(x[d] * cos[d]);  b = bf16((d < 32 ? -x[d + 32] : x[d - 32]) * sin[d]);  y[d] = bf16(a + b), in fp32, round to nearest
 *            even: the bits of mm_rope_qk_hd64.
 *   Slots    the page table already counts the new tokens; append_indptr [batch + 1] splits the T tokens among the sequences and each
 *            sequence's go to its last positions.  A table that does not count the appended tokens writes nothing for them; a page
 *            outside [0, max_pages) writes nothing; append_indptr is not validated beyond that (it has to be non-decreasing from 0 to T).
 *   Outputs  q_out bf16 [T, Hq, 64] contiguous: the rotated q.  k_out, v_out bf16 [T, Hkv, 64] contiguous, each optional (NULL): what a
 *            reader of each token's slot gets back -- bf16: rope(k) and v; fp8: decode(code) * 2^e, exact in bf16 -- written for every
 *            token, whether or not its slot was.  They feed mm_dense_attention_hd64 for a fresh prompt.
 *   Copy     cos == sin == NULL: no rotation, the plain append.  q and q_out may then be NULL as well (both or neither); when given, q
 *            is copied to q_out.  One of cos, sin NULL and the other not is MM_ERR_BAD_ARG.
 *   Capture  no workspace, no device array read by the host, a grid of ceil(T / MM_KV_HD64_APPEND_TOKENS) workgroups: capture-safe.
 *            The outputs must not overlap the inputs or each other.
 * Limits and statuses, all without device work, mm_rope_prefill's restated with 64.  MM_ERR_BAD_ARG: a kv_dtype that is no mm_kv_dtype,
 * max_pages, num_layers, num_kv_heads, page_size < 1, layer outside [0, num_layers), num_kv_heads > 65535, batch < 0 or > 65535,
 * num_tokens < 0, num_qo_heads < 1, num_qo_heads no multiple of num_kv_heads, a stride that is no multiple of 8 or smaller than its row
 * (max(Hq, Hkv) * 64 for q | k | v; 64 for cos / sin, when given).  MM_ERR_UNSUPPORTED: MM_KV_INT4.  num_tokens == 0: MM_OK.  Then
 * MM_ERR_BAD_ARG: batch == 0 (tokens that belong to no sequence), a null kv_data, kv_param (fp8), page-table array, append_indptr, k or
 * v; a null q or q_out with cos / sin given; q given without q_out or the reverse; q, k, v, cos, sin, q_out, k_out, v_out or kv_data not
 * 16-byte aligned; kv_param or an int32 array not 4-byte aligned.
 *
 * mm_paged_decode_hd64.  Single-token GQA attention over layer `layer`: q bf16 [batch, Hq, 64] -> o bf16 [batch, Hq, 64], rounded once.
 *   Heads      Hq = g * Hkv with g <= 16; query head h reads kv head h / g (HF repeat_kv).
 *   Arithmetic scores q.k in fp32 from the bf16 values (fp8: from the codes, the row's power-of-two scale applied to the fp32 score, which
 *              moves no rounding), online softmax in fp32 in the log2 domain with sm_scale (<= 0: 1 / sqrt(64)), p.V in fp32 without
 *              rounding p, fp32 accumulation.  Over an fp8 cache the result equals, bit for bit, that over a bf16 cache holding the
 *              dequantized values.
 *   Lengths    a sequence of length 0 gives zeros.  A sequence longer than max_seq_len is still attended in full: the last chunk runs to
 *              the sequence's end.  A token on a page outside [0, max_pages) is not attended.
 *   Split      from host values only -- batch, num_kv_heads, max_seq_len -- so a captured graph stays valid while the sequences grow up
 *              to max_seq_len.  mm_paged_decode_hd64_split publishes it: chunks = min(ceil(512 / (batch * Hkv)), ceil(max_seq_len /
 *              256)), at least 1; chunk_len = ceil(max_seq_len / chunks) rounded up to a multiple of MM_KV_HD64_DECODE_TILE *
 *              MM_KV_HD64_DECODE_WAVES = 256; chunks = ceil(max_seq_len / chunk_len) again (1 for max_seq_len == 0).  Chunk c of a
 *              sequence is its tokens [c * chunk_len, (c + 1) * chunk_len), the last chunk to the end.  One workgroup of
 *              MM_KV_HD64_DECODE_WAVES waves serves a (sequence, kv head, chunk) and all g heads; a wave walks tiles of
 *              MM_KV_HD64_DECODE_TILE tokens.
 *   Workspace  mm_paged_decode_hd64_workspace_bytes: 0 for one chunk -- a single launch then writes o --, else batch * Hq * chunks * 66
 *              floats of partials that a second, small launch merges.  It needs no initialisation, holds no tickets, and must be 16-byte
 *              aligned.  0 also for arguments mm_paged_decode_hd64 refuses.
 *   Capture    nothing is read on the host and nothing allocated: capture-safe.
 * Statuses, all without device work.  MM_ERR_BAD_ARG: the geometry cases of mm_rope_kv_append_hd64, num_qo_heads < 1 or no multiple of
 * num_kv_heads, max_seq_len < 0.  MM_ERR_UNSUPPORTED: MM_KV_INT4, g > 16.  batch == 0: MM_OK.  Then MM_ERR_BAD_ARG: a null q, o, kv_data,
 * kv_param (fp8) or page-table array; q, o or kv_data not 16-byte aligned; kv_param or an int32 array not 4-byte aligned; a workspace
 * that is needed and null, smaller than mm_paged_decode_hd64_workspace_bytes or not 16-byte aligned.
 *
 * Out of scope: int4 for 64-wide rows; the sliding-window, shared-prefix and tree forms (the causal multi-token form is
 * micromix_kv_prefill_hd64.h's); mm_dense_attention_prefix / mm_kv_gather_dense, mm_kv_copy_pages and mm_kv_move_rows for 64-wide rows.
 */
#ifndef MICROMIX_KV_HD64_H
#define MICROMIX_KV_HD64_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MM_KV_HD64_APPEND_TOKENS 16
#define MM_KV_HD64_DECODE_TILE 64
#define MM_KV_HD64_DECODE_WAVES 4

int mm_rope_kv_append_hd64(void *kv_data, void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer, int num_kv_heads,
                           int page_size, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_len, int batch,
                           const void *q_bf16, const void *k_bf16, const void *v_bf16, int64_t qkv_token_stride, int num_qo_heads,
                           const void *cos_bf16, const void *sin_bf16, int64_t cs_token_stride, const int32_t *append_indptr,
                           int num_tokens, void *q_out_bf16, void *k_out_bf16, void *v_out_bf16, mm_stream_t stream);

size_t mm_paged_decode_hd64_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int max_seq_len);

/* the split mm_paged_decode_hd64 uses for these host values; MM_ERR_BAD_ARG for batch, num_kv_heads < 1, max_seq_len < 0 or a null pointer */
int mm_paged_decode_hd64_split(int batch, int num_kv_heads, int max_seq_len, int *chunks, int *chunk_len);

int mm_paged_decode_hd64(const void *q_bf16, const void *kv_data, const void *kv_param, int kv_dtype, int max_pages, int num_layers,
                         int layer, int num_kv_heads, int page_size, const int32_t *kv_indptr, const int32_t *kv_indices,
                         const int32_t *last_page_len, int batch, int num_qo_heads, int max_seq_len, float sm_scale, void *workspace,
                         size_t workspace_bytes, void *o_bf16, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
