// Page copy of the paged KV cache (mm_kv_copy_pages, include/micromix_hip.h): the first r token rows of every (layer, K / V, kv head) of
// a source page go to the same rows of a destination page, bytes only -- what a sequence needs before it writes into a partly filled
// page it shares with another (PagedKVCache.extend, copy-on-write).
//
// kv_row (mx_paged_kv.h) numbers the rows (page, layer, K / V, head, slot) with the page outermost, so a page is 2 L v_offset(kv)
// consecutive rows from kv_row(page, layer 0, K, head 0, slot 0) on, and the k-th 16-byte vector of one page corresponds to the k-th of
// another: row k / VPR of the page, slot (k / VPR) % P, which is copied when the slot lies below r.  The parameter dword of row j of
// the page likewise.  Nothing but that modulo is computed per lane; the page bases are uniform over the workgroup.
//
// Grid (slices, pairs): a workgroup of 256 lanes owns 2 * 256 consecutive vectors of its pair's page, 8 KiB, both loads issued before
// the first store.  One bf16 page at Llama-3-8B shapes (L 32, Hkv 8, P 16: 2 MiB) is 256 workgroups, one per CU; an fp8 page 128, an
// int4 page 64.  The slice count depends on the geometry alone (r is read on the device), so lanes above r idle without touching memory.
// The first rows-per-page lanes of a pair also move the parameter dwords: there are at least twice as many lanes as rows.
#include "mx_paged_kv.h"

namespace mm {

using namespace kv;

constexpr int COPY_THREADS = 256, COPY_VECS = 2;      // per workgroup: 256 lanes x 2 vectors of 16 bytes

template <int KIND>
__global__ __launch_bounds__(COPY_THREADS) void kv_copy_pages_kernel(const PagedKV kv, const int *__restrict__ src_pages,
                                                                    const int *__restrict__ dst_pages, const int *__restrict__ rows) {
    constexpr int VPR = KIND == KV_INT4 ? 4 : KIND == KV_FP8 ? 8 : 16;      // 16-byte vectors per row: 64, 128 or 256 bytes of codes
    const int pair = blockIdx.y;
    const int src = src_pages[pair], dst = dst_pages[pair];
    const int r = rows ? min(rows[pair], kv.P) : kv.P;
    if (src < 0 || src >= kv.max_pages || dst < 0 || dst >= kv.max_pages || src == dst || r <= 0) return;
    const int64_t page_rows = 2 * kv.L * v_offset(kv);                      // kv.layer is 0: kv_row gives the page's first row
    const int64_t src_row = kv_row(kv, src, 0, 0, 0), dst_row = kv_row(kv, dst, 0, 0, 0);
    const v4u *s = (const v4u *)kv.data + src_row * VPR;
    v4u *d = (v4u *)kv.data + dst_row * VPR;
    const int64_t first = (int64_t)blockIdx.x * (COPY_THREADS * COPY_VECS) + threadIdx.x;
    v4u x[COPY_VECS];
    bool live[COPY_VECS];
#pragma unroll
    for (int u = 0; u < COPY_VECS; ++u) {
        const int64_t k = first + u * COPY_THREADS;
        live[u] = k < page_rows * VPR && (r == kv.P || (int)((uint32_t)(k / VPR) % (uint32_t)kv.P) < r);
        if (live[u]) x[u] = s[k];
    }
#pragma unroll
    for (int u = 0; u < COPY_VECS; ++u)
        if (live[u]) d[first + u * COPY_THREADS] = x[u];
    if (KIND != KV_BF16) {
        const int64_t j = (int64_t)blockIdx.x * COPY_THREADS + threadIdx.x;     // the page's rows, one dword (scale, zero) each
        if (j < page_rows && (int)((uint32_t)j % (uint32_t)kv.P) < r)
            ((uint32_t *)kv.param)[dst_row + j] = ((const uint32_t *)kv.param)[src_row + j];
    }
}

// a page holds fewer than 2^31 vectors (mm_kv_copy_pages checks), so the slices fit grid.x; the pairs go in launches of 65535 (grid.y)
hipError_t launch_kv_copy_pages(const PagedKV &kv, const int *src_pages, const int *dst_pages, const int *rows, int num_pairs,
                                hipStream_t stream) {
    const int vpr = kv.kind == KV_INT4 ? 4 : kv.kind == KV_FP8 ? 8 : 16;
    const int64_t vecs = (int64_t)2 * kv.L * kv.Hkv * kv.P * vpr, per_wg = COPY_THREADS * COPY_VECS;
    const unsigned slices = (unsigned)((vecs + per_wg - 1) / per_wg);
    for (int p0 = 0; p0 < num_pairs; p0 += 65535) {
        const dim3 grid(slices, num_pairs - p0 < 65535 ? num_pairs - p0 : 65535);
        const int *r = rows ? rows + p0 : nullptr;
        if (kv.kind == KV_INT4) kv_copy_pages_kernel<KV_INT4><<<grid, COPY_THREADS, 0, stream>>>(kv, src_pages + p0, dst_pages + p0, r);
        else if (kv.kind == KV_FP8) kv_copy_pages_kernel<KV_FP8><<<grid, COPY_THREADS, 0, stream>>>(kv, src_pages + p0, dst_pages + p0, r);
        else kv_copy_pages_kernel<KV_BF16><<<grid, COPY_THREADS, 0, stream>>>(kv, src_pages + p0, dst_pages + p0, r);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mm
