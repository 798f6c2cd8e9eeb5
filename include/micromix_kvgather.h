/*
 * micromix_kvgather.h -- one layer of a paged KV cache as contiguous bf16 K and V: the operands mm_dense_attention_prefix
 * (micromix_attention_prefix.h) takes when the sequences already hold tokens.
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The status
 * codes are micromix_hip.h's.  micromix_amd/paged.py (kv_gather_dense) is the Python side; csrc/kv_gather.hip is the kernel.
 *
 * mm_kv_gather_dense.  The cache arguments kv_data .. batch are those of every cache op of micromix_hip.h (mm_kv_append), in their
 * order and with their meaning; the cache is int4, fp8 (e4m3) or bf16.  k_out and v_out are bf16: token row t, head h, element e lies at
 * k_out[t * k_stride + h * 128 + e], rows 0 .. total_kv_tokens - 1, the strides in ELEMENTS BETWEEN TWO TOKENS; v_out likewise.
 *   Rows      out_indptr (device, int32 [batch + 1]) places the sequences: token p of sequence b, p < its length by the page table, goes
 *             to row out_indptr[b] + p.  Entries are clamped to [0, total_kv_tokens].  A row outside every sequence's range is not
 *             written; neither is a row past the sequence's length, a row at or past out_indptr[b + 1], or a token on a page index
 *             outside the cache (a released -1 entry included).
 *   Values    what a reader of the slot gets back, the rule mm_rope_prefill states for k_out / v_out: bf16 the stored bits, fp8
 *             code * 2^e (exact), int4 bf16(code * scale - zero) computed in fp32 from the fp16 parameters as stored.  One copy of the
 *             rule serves both kernels (csrc/mx_paged_kv.h).
 *   Capture   the page table and out_indptr are read on the device only and nothing is allocated: the grid is
 *             ceil(total_kv_tokens / MM_KV_GATHER_TOKENS) workgroups of min(2 * num_kv_heads, 16) waves, from host values alone, so a
 *             captured graph replays while the sequences grow within total_kv_tokens.
 *
 * Limits: head_dim 128; each stride a multiple of 8 elements and at least num_kv_heads * 128; kv_data, k_out, v_out 16-byte aligned.
 * Offsets are 64-bit throughout.
 *
 * Statuses, all without device work.  The cache geometry first, as mm_kv_append refuses it (MM_ERR_BAD_ARG; head_dim != 128:
 * MM_ERR_UNSUPPORTED).  MM_ERR_BAD_ARG: total_kv_tokens < 0; a stride that is no multiple of 8 or smaller than num_kv_heads * 128; with
 * work to do (total_kv_tokens > 0 and batch > 0): a null cache pointer, k_out, v_out or out_indptr, kv_data, k_out or v_out not 16-byte
 * aligned, kv_param or an int32 table not 4-byte aligned.  total_kv_tokens == 0 or batch == 0: MM_OK.
 */
#ifndef MICROMIX_KVGATHER_H
#define MICROMIX_KVGATHER_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MM_KV_GATHER_TOKENS 8

int mm_kv_gather_dense(void *kv_data, void *kv_param, int kv_dtype, int max_pages, int num_layers, int layer, int num_kv_heads, int page_size,
                       int head_dim, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_len, int batch,
                       const int32_t *out_indptr /* device, [batch + 1] */, int total_kv_tokens, void *k_out, void *v_out, long long k_stride,
                       long long v_stride, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
