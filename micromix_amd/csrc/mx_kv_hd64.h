// Host side of the paged KV cache for 64-wide heads (kv_hd64.hip, include/micromix_kv_hd64.h): what capi.hip calls.  kv.kind is
// KV_BF16 or KV_FP8; the rows of kv.data are 64 values wide.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mx_kernels.h"

namespace mm {

// split-KV chunks of the decode, from host values only (kv_chunks' rule, chunks of whole 64-token tiles for four waves)
void kv_decode_hd64_split(int B, int Hkv, int max_seq_len, int *nc, int *chunk);
size_t kv_decode_hd64_workspace_bytes(int B, int Hq, int Hkv, int max_seq_len);
hipError_t launch_paged_decode_hd64(const PagedKV &kv, const void *q, int Hq, int max_seq_len, float sm_scale, void *ws, void *o,
                                    hipStream_t stream);
// cos == sin == nullptr: no rotation; q == q_out == nullptr: no q rows; k_out / v_out each optional
hipError_t launch_rope_kv_append_hd64(const PagedKV &kv, const void *q, const void *k, const void *v, int64_t qkv_stride, int Hq,
                                      const void *cos, const void *sin, int64_t cs_stride, const int *append_indptr, int T, void *q_out,
                                      void *k_out, void *v_out, hipStream_t stream);

// causal multi-token attention (kv_prefill_hd64.hip, include/micromix_kv_prefill_hd64.h).  The plan, from host values only: the rows of
// a workgroup (128 or 64), its query tokens bq = rows / g, the tile count T / bq + B and DESIGN 7c's chunks of whole 64-token tiles
void kv_prefill_hd64_plan(int T, int B, int Hq, int Hkv, int max_seq_len, int *rows, int *bq, int *tiles, int *nc, int *chunk);
size_t kv_prefill_hd64_workspace_bytes(int T, int B, int Hq, int Hkv, int max_seq_len);
hipError_t launch_paged_prefill_hd64(const PagedKV &kv, const void *q, const int *qo_indptr, int T, int Hq, int max_seq_len,
                                     float sm_scale, void *ws, void *o, hipStream_t stream);

}  // namespace mm
