/*
 * micromix_decode_step.h -- one decode step over the 128-wide paged KV cache in one launch: RoPE of q and k, the append of the step's
 * token and single-token attention over the sequence that now holds it.  It is mm_rope_kv_append (one token per sequence) followed by
 * mm_paged_decode (micromix_hip.h) without the launch boundary between them; both entries stay as they are.
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The status
 * codes are micromix_hip.h's.  micromix_amd/paged.py (rope_append_decode) and PagedKVCache.decode_step are the Python side; the kernel
 * is csrc/decode_step.hip.
 *
 * mm_rope_append_decode.
 *   Tokens     exactly one new token per sequence, token b for sequence b: mm_rope_kv_append's append_indptr = 0, 1, .., batch.  The page
 *              table already counts the token, so it goes to position len_b - 1.
 *   Inputs     q, k, v are bf16 pointers that share the token stride qkv_token_stride (elements): views of the packed q | k | v
 *              projection, read in place, heads contiguous within a token.  cos, sin bf16 [batch, 128] with row stride cs_token_stride,
 *              row b for sequence b.  As in mm_rope_kv_append.
 *   Cache      the layout, the kinds (MM_KV_INT4, MM_KV_FP8_E4M3, MM_KV_BF16) and the page table of micromix_hip.h; head_dim must be 128;
 *              Hq = g * Hkv with g <= 16; any page_size >= 1.
 *   Results    After the call kv_data / kv_param hold, byte for byte, what mm_rope_kv_append leaves; o bf16 [batch, Hq, 128] is, bit for
 *              bit, what mm_paged_decode returns after that append for the same max_seq_len and sm_scale (<= 0: 1 / sqrt(128)); q_out
 *              bf16 [batch, Hq, 128], optional (NULL), receives the rotated q, bit-equal to mm_rope_kv_append's.  The slot rule, the
 *              guards, the int4 / fp8 rules, the RoPE and the attention arithmetic are those entries' own code.
 *   Edges      the chain's: a sequence of length 0 writes nothing and gives zeros (its q is still rotated into q_out); a page outside
 *              [0, max_pages) is neither written nor attended; a sequence longer than max_seq_len is attended in full by the last chunk.
 *   Split      mm_paged_decode's, from the same host values; mm_rope_append_decode_workspace_bytes equals
 *              mm_paged_decode_workspace_bytes for every argument.  With more than one chunk a second, small launch merges the partials
 *              (mm_paged_decode's merge), so the call is one launch or two where the chain is two or three.
 *   Capture    capture-safe: nothing is read on the host, the workspace needs no initialisation and holds no tickets, and no workgroup
 *              waits on another.  o, q_out and the workspace must not overlap the inputs, the cache or each other.
 * Statuses, all without device work: the union of the two entries'.  MM_ERR_BAD_ARG: a kv_dtype that is no mm_kv_dtype, max_pages,
 * num_layers, num_kv_heads, page_size, head_dim < 1, layer outside [0, num_layers), num_kv_heads > 65535, batch < 0 or > 65535.
 * MM_ERR_UNSUPPORTED: head_dim other than 128.  MM_ERR_BAD_ARG: num_qo_heads < 1 or no multiple of num_kv_heads, max_seq_len < 0,
 * qkv_token_stride < num_qo_heads * 128, cs_token_stride < 128, an odd stride.  MM_ERR_UNSUPPORTED: g > 16.  batch == 0: MM_OK.  Then
 * MM_ERR_BAD_ARG: a null kv_data, kv_param (int4, fp8), page-table array, q, k, v, cos, sin or o; q, k, v, cos, sin, o or q_out not
 * 4-byte aligned; a workspace that is needed and null, smaller than mm_rope_append_decode_workspace_bytes or not 16-byte aligned.
 *
 * Out of scope: the sliding-window, shared-prefix and tree forms of the attention, more than one new token per sequence, and 64-wide
 * rows; those steps stay mm_rope_kv_append / mm_rope_prefill followed by their attention entry.
 */
#ifndef MICROMIX_DECODE_STEP_H
#define MICROMIX_DECODE_STEP_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

size_t mm_rope_append_decode_workspace_bytes(int batch, int num_qo_heads, int num_kv_heads, int max_seq_len);

int mm_rope_append_decode(void *kv_data, void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer, int num_kv_heads,
                          int page_size, int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_len,
                          int batch, const void *q_bf16, const void *k_bf16, const void *v_bf16, int64_t qkv_token_stride,
                          int num_qo_heads, const void *cos_bf16, const void *sin_bf16, int64_t cs_token_stride, int max_seq_len,
                          float sm_scale, void *workspace, size_t workspace_bytes, void *q_out_bf16, void *o_bf16, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
