// Host side of mm_paged_decode_shared (include/micromix_hip.h; the kernels: kv_cache.hip): the argument rules, the two splits and the
// workspace size.  Plain C++ without a HIP call, so a stand-alone program can run it under the host sanitizers over the edge values
// (tools/kv_shared_host_check.cpp).  Everything here depends on the host arguments alone: a captured graph stays valid while the
// sharing changes between replays.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/micromix_hip.h"

namespace mm {

void kv_chunks(long long work, int target_workgroups, int max_seq_len, int round_to, int *nc, int *chunk);   // kv_cache.hip

constexpr int KV_SHARED_MAX_BOUND = 1 << 29;      // of max_shared_len and max_suffix_len: kv_chunks adds a bound and a chunk in an int
constexpr int KV_SHARED_ROUND = 128;              // a chunk gives each of the four waves whole 32-token tiles (kv_decode_split's rule)

// the sizes the kernels can take; MM_OK, or the status mm_paged_decode_shared returns before it looks at a pointer
inline int kv_shared_sizes_status(int B, int Hq, int Hkv, int max_shared_len, int max_suffix_len) {
    if (B < 0 || B > 65535 || Hkv <= 0 || Hkv > 65535 || Hq <= 0 || Hq % Hkv) return MM_ERR_BAD_ARG;
    if (max_shared_len < 0 || max_suffix_len < 0 || max_shared_len > KV_SHARED_MAX_BOUND || max_suffix_len > KV_SHARED_MAX_BOUND)
        return MM_ERR_BAD_ARG;
    return Hq / Hkv > 16 ? MM_ERR_UNSUPPORTED : MM_OK;
}

struct KvSharedSplit {
    int ncA, chunkA;           // prefix walk [0, shared): ncA chunks of chunkA tokens
    int ncB, chunkB;           // tail walk [shared, len): ncB chunks of chunkB tokens
};

// Sizes that passed kv_shared_sizes_status, B >= 1.  The prefix's work items are the slabs -- at least ceil(B / per) of them per kv head,
// per = 16 / g members to a slab, and exactly that many when one group holds the batch, the case the split is made for; with more
// groups there are more slabs and more workgroups than the target, never fewer.  The tails are one item per (sequence, kv head).
inline KvSharedSplit kv_shared_split(int B, int Hq, int Hkv, int max_shared_len, int max_suffix_len) {
    const int per = 16 / (Hq / Hkv);
    KvSharedSplit s;
    kv_chunks((long long)((B + per - 1) / per) * Hkv, 512, max_shared_len, KV_SHARED_ROUND, &s.ncA, &s.chunkA);
    kv_chunks((long long)B * Hkv, 512, max_suffix_len, KV_SHARED_ROUND, &s.ncB, &s.chunkB);
    return s;
}

// partials of every (sequence, query head): ncA + ncB chunks of (o[128], m, l) fp32; 0 for sizes the call refuses (or B = 0)
inline size_t kv_shared_workspace_bytes(int B, int Hq, int Hkv, int max_shared_len, int max_suffix_len) {
    if (B <= 0 || kv_shared_sizes_status(B, Hq, Hkv, max_shared_len, max_suffix_len) != MM_OK) return 0;
    const KvSharedSplit s = kv_shared_split(B, Hq, Hkv, max_shared_len, max_suffix_len);
    unsigned long long n = (unsigned long long)B * (unsigned long long)Hq;          // < 2^16 * 2^31
    if (__builtin_mul_overflow(n, (unsigned long long)(s.ncA + s.ncB), &n)) return 0;
    if (__builtin_mul_overflow(n, (unsigned long long)((128 + 2) * sizeof(float)), &n)) return 0;
    return n > SIZE_MAX ? 0 : (size_t)n;
}

// the workspace a call was given: present, large enough, 16-byte aligned
inline int kv_shared_workspace_status(const void *workspace, size_t workspace_bytes, size_t need) {
    return need && workspace && workspace_bytes >= need && !((uintptr_t)workspace & 15) ? MM_OK : MM_ERR_BAD_ARG;
}

}  // namespace mm
