/*
 * micromix_attention_prefix.h -- the rectangular form of mm_dense_attention (micromix_attention.h): dense causal GQA attention of new
 * query tokens over contiguous bf16 K and V that also hold the tokens in front of them -- the second and later chunks of a chunked
 * prefill, a new turn over a cached conversation, a prompt behind a shared prefix -- with the mask aligned bottom-right as
 * mm_paged_prefill has it, and the work split along kv so that a short query block over a long prefix fills the device.
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The status
 * codes are micromix_hip.h's.  micromix_amd/paged.py (dense_attention_prefix) is the Python side; csrc/dense_attention.hip holds the
 * kernel, the third instantiation of mm_dense_attention's, and the merge.  mm_kv_gather_dense (micromix_kvgather.h) makes K and V
 * from a paged cache.
 *
 * mm_dense_attention_prefix.  q, k, v, the strides, the heads, head_dim, sm_scale, o, the arithmetic, the tiles and the limits are
 * mm_dense_attention's.  q and o hold total_q_tokens tokens, k and v total_kv_tokens.
 *   Sequences  qo_indptr and kv_indptr (device, int32 [batch + 1] each) split the two: sequence b owns query tokens qo_indptr[b] ..
 *              qo_indptr[b + 1] (nq of them) and kv tokens kv_indptr[b] .. kv_indptr[b + 1] (nk).  Entries are clamped to
 *              [0, total_q_tokens] and [0, total_kv_tokens]; query tokens that no sequence owns are not written.
 *   Mask       query i of sequence b attends keys 0 .. nk - nq + i of that sequence; a query for which that range is empty (nk < nq)
 *              writes zeros.  Nothing of another sequence is read, and no kv row past the last one a query tile attends.
 *   Split      mm_dense_attention_prefix_plan gives nc chunks of `chunk` kv tokens (a multiple of MM_DENSE_ATTN_BK), from
 *              total_q_tokens, batch, num_q_heads and max_kv_len alone: enough chunks for MM_DENSE_PREFIX_TARGET workgroups, the
 *              workgroups an MI355X holds at once, at most one per 256 tokens of max_kv_len.  max_kv_len bounds every nk, as max_seq_len bounds
 *              mm_paged_prefill's lengths; kv tokens at or past nc * chunk would not be attended.  Workgroup (query tile, head, c) walks
 *              the kv tiles of tokens [c * chunk, (c + 1) * chunk) below its diagonal and leaves unnormalised fp32 partial rows and
 *              (m, l) in the workspace; a second launch merges them and rounds to bf16 once.  No atomics.
 *   nc == 1    the kernel writes o itself and takes no workspace; with nq == nk for every sequence the bits are mm_dense_attention's.
 *   Workspace  mm_dense_attention_prefix_workspace_bytes(total_q_tokens, batch, num_q_heads, max_kv_len) bytes, 16-byte aligned,
 *              uninitialised; 0 when nc == 1.
 *   Capture    both tables are read on the device only: the grid is (total_q_tokens / MM_DENSE_ATTN_BQ + batch) * num_q_heads * nc
 *              workgroups (and that many / nc for the merge), from host values alone, so a captured graph replays while the
 *              sequences grow within max_kv_len and total_kv_tokens.
 *
 * Limits: mm_dense_attention's, and the grid above < 2^31.
 *
 * Statuses, all without device work: mm_dense_attention's, in its order, with total_q_tokens in the place of total_tokens and both
 * tables in the place of seq_indptr; total_kv_tokens < 0 or max_kv_len < 0: MM_ERR_BAD_ARG, with its first argument checks; with work
 * to do (total_q_tokens > 0 and batch > 0) and nc > 1, a workspace that is null, not 16-byte aligned or smaller than
 * mm_dense_attention_prefix_workspace_bytes: MM_ERR_BAD_ARG, after every other check.  total_q_tokens == 0 or batch == 0: MM_OK.
 * The two queries refuse nothing.  mm_dense_attention_prefix_plan writes nc and chunk (either pointer may be null) and returns nc; for
 * counts the entry refuses (a negative one, num_q_heads < 1) and for nothing to do it gives nc = 1, chunk = MM_DENSE_ATTN_BK, and the
 * bytes are 0.
 */
#ifndef MICROMIX_ATTENTION_PREFIX_H
#define MICROMIX_ATTENTION_PREFIX_H
#include "micromix_attention.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MM_DENSE_PREFIX_TARGET 512

int mm_dense_attention_prefix_plan(int total_q_tokens, int batch, int num_q_heads, int max_kv_len, int *num_chunks, int *chunk_tokens);

size_t mm_dense_attention_prefix_workspace_bytes(int total_q_tokens, int batch, int num_q_heads, int max_kv_len);

int mm_dense_attention_prefix(const void *q, const void *k, const void *v, long long q_stride, long long k_stride, long long v_stride,
                              const int32_t *qo_indptr /* device, [batch + 1] */, const int32_t *kv_indptr /* device, [batch + 1] */,
                              int batch, int total_q_tokens, int total_kv_tokens, int num_q_heads, int num_kv_heads, int head_dim,
                              int max_kv_len, float sm_scale, void *workspace, size_t workspace_bytes,
                              void *o /* bf16 [total_q_tokens, Hq, 128] contiguous */, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
