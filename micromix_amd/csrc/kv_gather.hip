// One layer of a paged KV cache as contiguous bf16 K and V (include/micromix_kvgather.h, mm_kv_gather_dense, which states the function):
// the operands of the rectangular dense attention (dense_attention.hip, mm_dense_attention_prefix) when the sequences already hold tokens.
// The kernel holds no rule of its own: the page-table walk (seq_len, kv_row, row_of) and the value a reader of a slot gets back
// (fp8_seen, int4_seen: what store_row8 reports for the rows it writes) are mx_paged_kv.h's.
//
// Design, the shape rope_prefill.hip uses for rows.  A workgroup owns TPW = MM_KV_GATHER_TOKENS = 8 consecutive OUTPUT rows and is G
// waves wide, G = min(2 Hkv, 16).
//   Rows     Eight adjacent lanes own a 128-element head row: lane j of the eight holds elements 8 j .. 8 j + 7 and 64 + 8 j .. 64 + 8 j + 7.
//            It loads them as the cache stores them -- bf16 two 16-byte loads, fp8 two 8-byte loads, int4 two dwords, and the row's
//            4-byte (scale, zero) -- and stores two 16-byte halves.  No cross-lane exchange, no LDS.
//   Waves    A wave is 8 row groups, one per output row of the workgroup; the 2 Hkv rows of a token -- Hkv of K, then Hkv of V -- are
//            dealt to the G waves round robin, so which tensor a row goes to is uniform over a wave.
//   Slots    Every lane looks its own output row up ahead of the wave's first row: the sequence (binary search over out_indptr), its
//            length, the page.  The eight dependent chains of a wave run side by side; the row of (K / V, head) follows from the token's
//            K row of head 0 by an offset (row_of).  A row that belongs to no token leaves with its whole group.
//   Capture  The grid is ceil(total_kv_tokens / 8) workgroups: nothing of the tables is known on the host.
//   Offsets  64-bit throughout.
// Compiler report: DESIGN 7y; no scratch, no LDS.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "../../include/micromix_kvgather.h"
#include "mx_kernels.h"
#include "mx_paged_kv.h"

namespace {

using namespace mm::kv;

constexpr int TPW = MM_KV_GATHER_TOKENS, MAX_WAVES = 16;
static_assert(TPW == 8, "a wave is one 8-lane row group per output row of the workgroup");

template <int KIND>
__global__ __launch_bounds__(64 * MAX_WAVES) void kv_gather_kernel(const mm::KVGather a) {
    const int j = threadIdx.x & 7, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * TPW + ((threadIdx.x >> 3) & (TPW - 1));
    if (i >= a.T) return;                                     // whole row groups leave: no lane needs another
    // ---- the token of output row i: sequence b = the largest one with start(b) <= i, position p in it
    int lo = 0, hi = a.kv.B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (min(max(a.out_indptr[mid], 0), a.T) <= i) lo = mid; else hi = mid;
    }
    const int64_t p = i - min(max(a.out_indptr[lo], 0), a.T);
    if (p < 0 || i >= min(max(a.out_indptr[lo + 1], 0), a.T) || p >= seq_len(a.kv, lo)) return;
    const int page = a.kv.indices[a.kv.indptr[lo] + (int)p / a.kv.P];
    if (page < 0 || page >= a.kv.max_pages) return;           // a released entry: nothing to hand on
    const int64_t row0 = kv_row(a.kv, page, 0, 0, (int)p % a.kv.P);

    for (int r = wave; r < 2 * a.kv.Hkv; r += a.G) {
        const int which = r >= a.kv.Hkv, h = r - which * a.kv.Hkv;
        const int64_t row = row_of(a.kv, row0, which, h);
        v4u x[2];                                             // lo | hi halves of the row, bf16 bits
        if (KIND == KV_BF16) {
            const v4u *src = (const v4u *)a.kv.data + row * (HD / 8);
            x[0] = src[j], x[1] = src[HD / 16 + j];
        } else if (KIND == KV_FP8) {
            const v2u *src = (const v2u *)a.kv.data + row * (HD / 8);
            const v2u c0 = src[j], c1 = src[HD / 16 + j];
            const float scale = scale_of(((const uint32_t *)a.kv.param)[row]);
            const v2u s0 = fp8_seen(c0.x, scale), s1 = fp8_seen(c0.y, scale), s2 = fp8_seen(c1.x, scale), s3 = fp8_seen(c1.y, scale);
            x[0] = v4u{s0.x, s0.y, s1.x, s1.y};
            x[1] = v4u{s2.x, s2.y, s3.x, s3.y};
        } else {
            const uint32_t *src = (const uint32_t *)a.kv.data + row * (HD / 8);
            const uint32_t code[2] = {src[j], src[HD / 16 + j]}, w = ((const uint32_t *)a.kv.param)[row];
            const float sf = scale_of(w), zf = zero_of(w);
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int m = 0; m < 4; ++m) {                 // byte m: element 2 m of the eight in the low nibble
                    const uint32_t byte = (code[half] >> (8 * m)) & 0xffu;
                    x[half][m] = int4_seen((float)(byte & 15u), (float)(byte >> 4), sf, zf);
                }
        }
        v4u *dst = (v4u *)((which ? a.v_out + i * a.sv : a.k_out + i * a.sk) + (int64_t)h * HD);
        dst[j] = x[0];
        dst[HD / 16 + j] = x[1];
    }
}

}  // namespace

namespace mm {

hipError_t launch_kv_gather(KVGather a, hipStream_t stream) {
    a.G = 2 * a.kv.Hkv < MAX_WAVES ? 2 * a.kv.Hkv : MAX_WAVES;
    const unsigned grid = (unsigned)(((int64_t)a.T + TPW - 1) / TPW);
    if (a.kv.kind == KV_INT4) kv_gather_kernel<KV_INT4><<<grid, 64 * a.G, 0, stream>>>(a);
    else if (a.kv.kind == KV_FP8) kv_gather_kernel<KV_FP8><<<grid, 64 * a.G, 0, stream>>>(a);
    else kv_gather_kernel<KV_BF16><<<grid, 64 * a.G, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace mm
