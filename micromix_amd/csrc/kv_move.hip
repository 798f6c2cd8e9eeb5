// Row moves inside the paged KV cache (mm_kv_move_rows, include/micromix_hip.h): within one sequence, the token row at logical position
// src goes to logical position dst, for every (layer, K / V, kv head), bytes only -- what keeps the accepted root-to-leaf path of a tree
// draft: its rows sit in scattered slots among the draft's and become the next contiguous positions (PagedKVCache.accept).
//
// The contract is read-all-then-write-all within a sequence: a destination may be another move's source (path [1, 2, 5] -> slots 0, 1, 2
// overwrites slot 1 and 2 while they are still wanted).  So one workgroup owns ALL moves of one (sequence, layer, K / V, head) -- at most
// MOVE_MAX = 64, 16 KiB of bf16 rows -- holds them in registers (lane k % 256 the k-th 16-byte vector of the move list: 1, 2 or 4 vectors
// a lane for int4 / fp8 / bf16), passes one barrier and only then stores.  Different (layer, K / V, head) never touch the same bytes, and
// different sequences do not either (the sole-owner rule of the pages a sequence writes), so nothing is ordered between workgroups.
// A move is dropped, source unread and destination unwritten, when src == dst, when a position is negative or past the pages the
// sequence lists, or when a page index lies outside [0, max_pages).  Workgroups of sequences without moves exit at once.
#include "mx_paged_kv.h"

namespace mm {

using namespace kv;

constexpr int MOVE_THREADS = 256, MOVE_MAX = 64;      // lanes per workgroup; moves performed per sequence

// the row (in rows of one token-head) that position pos of the sequence with page list `pages` (np entries) has; -1: no such row
__device__ inline int64_t move_row(const PagedKV &kv, const int *pages, int np, int pos, int layer, int which, int h) {
    if (pos < 0 || pos / kv.P >= np) return -1;
    const int page = pages[pos / kv.P];
    if (page < 0 || page >= kv.max_pages) return -1;
    return ((((int64_t)page * kv.L + layer) * 2 + which) * kv.Hkv + h) * kv.P + pos % kv.P;
}

template <int KIND>
__global__ __launch_bounds__(MOVE_THREADS) void kv_move_rows_kernel(const PagedKV kv, const int *__restrict__ move_indptr,
                                                                   const int *__restrict__ src_pos, const int *__restrict__ dst_pos,
                                                                   int num_moves) {
    constexpr int VPR = KIND == KV_INT4 ? 4 : KIND == KV_FP8 ? 8 : 16;      // 16-byte vectors per row: 64, 128 or 256 bytes of codes
    constexpr int VECS = MOVE_MAX * VPR / MOVE_THREADS;                     // per lane: 1, 2 or 4
    const int b = blockIdx.z, layer = blockIdx.y, which = blockIdx.x / kv.Hkv, h = blockIdx.x % kv.Hkv;
    const int m0 = min(max(move_indptr[b], 0), num_moves), m1 = min(max(move_indptr[b + 1], 0), num_moves);
    const int nm = min(m1 - m0, MOVE_MAX);
    if (nm <= 0) return;
    const int first = kv.indptr[b], np = kv.indptr[b + 1] - first;
    const int *pages = kv.indices + first;

    v4u x[VECS];
    int64_t dst[VECS];                                                      // the vector's index in kv.data; -1: not moved
#pragma unroll
    for (int u = 0; u < VECS; ++u) {
        const int k = threadIdx.x + u * MOVE_THREADS, m = k / VPR;
        dst[u] = -1;
        x[u] = v4u{0, 0, 0, 0};
        if (m < nm) {
            const int s = src_pos[m0 + m], d = dst_pos[m0 + m];
            const int64_t sr = move_row(kv, pages, np, s, layer, which, h), dr = move_row(kv, pages, np, d, layer, which, h);
            if (s != d && sr >= 0 && dr >= 0) {
                x[u] = ((const v4u *)kv.data)[sr * VPR + k % VPR];
                dst[u] = dr * VPR + k % VPR;
            }
        }
    }
    uint32_t par = 0;
    int64_t pdst = -1;
    if (KIND != KV_BF16 && (int)threadIdx.x < nm) {                         // lane m: the (scale, zero) dword of move m
        const int s = src_pos[m0 + threadIdx.x], d = dst_pos[m0 + threadIdx.x];
        const int64_t sr = move_row(kv, pages, np, s, layer, which, h), dr = move_row(kv, pages, np, d, layer, which, h);
        if (s != d && sr >= 0 && dr >= 0) {
            par = ((const uint32_t *)kv.param)[sr];
            pdst = dr;
        }
    }
    // the contract rests on this: the loaded values are in their registers (an empty asm that takes them as operands makes the compiler
    // wait for them) before the barrier, so every source of this (sequence, layer, K / V, head) is read before the first store below
#pragma unroll
    for (int u = 0; u < VECS; ++u) asm volatile("" ::"v"(x[u]));
    asm volatile("" ::"v"(par));
    __syncthreads();
#pragma unroll
    for (int u = 0; u < VECS; ++u)
        if (dst[u] >= 0) ((v4u *)kv.data)[dst[u]] = x[u];
    if (KIND != KV_BF16 && pdst >= 0) ((uint32_t *)kv.param)[pdst] = par;
}

// grid (K / V x head, layer, sequence): mm_kv_move_rows checks that the three fit
hipError_t launch_kv_move_rows(const PagedKV &kv, const int *move_indptr, const int *src_pos, const int *dst_pos, int num_moves,
                               hipStream_t stream) {
    const dim3 grid(2 * kv.Hkv, kv.L, kv.B);
    if (kv.kind == KV_INT4) kv_move_rows_kernel<KV_INT4><<<grid, MOVE_THREADS, 0, stream>>>(kv, move_indptr, src_pos, dst_pos, num_moves);
    else if (kv.kind == KV_FP8) kv_move_rows_kernel<KV_FP8><<<grid, MOVE_THREADS, 0, stream>>>(kv, move_indptr, src_pos, dst_pos, num_moves);
    else kv_move_rows_kernel<KV_BF16><<<grid, MOVE_THREADS, 0, stream>>>(kv, move_indptr, src_pos, dst_pos, num_moves);
    return hipGetLastError();
}

}  // namespace mm
