// One decode step over the 128-wide paged cache in one launch (include/micromix_decode_step.h, mm_rope_append_decode): what
// mm_rope_kv_append with one token per sequence followed by mm_paged_decode computes -- the same cache bytes, the same o, bit for bit.
//
// The split of the work is paged_decode's (kv_cache.hip): one workgroup of 4 waves per (sequence, kv head, chunk) walks the chunk's
// 32-token tiles for all g query heads; the walk is the shared tile loop, kv_decode_tiles.inc as WALK_STEP, and the chunk merge is
// kv_cache.hip's.  What this kernel adds in front of the walk:
//   q      every wave rotates its own A operand: lane (c, kq) of the MFMA layout holds dims 32 kq .. 32 kq + 31 of head c, whose
//          rotate_half partners are the 32 dims of block kq ^ 2 of the same row.  Both blocks, and the same block of the token's cos / sin
//          row, come straight from global memory into registers (4 x 64 bytes per lane, L2 hits after the first wave), 32 x rope_one
//          (mx_rope.h) per lane: no LDS, no exchange between lanes, waves or workgroups.  The waves repeat each other's work -- g x 128
//          elements four times -- instead of meeting at a barrier.  With q_out, wave 0 of chunk 0 stores what it holds.
//   k, v   position len - 1 lies in exactly one chunk.  The workgroup of that chunk writes the row: wave 0 rotates k (rope_pair) and
//          stores it, wave 1 stores v, both by store_row (mx_paged_kv.h) at the row append_row_at gives -- the code of
//          rope_kv_append_kernel, so the bytes are its bytes.  Then the workgroup passes __syncthreads(), which is a release fence at
//          workgroup scope (s_waitcnt vmcnt(0): the stores have reached L2, and the write-through vector L1 of the CU holds no older
//          copy of their lines -- a store updates or invalidates the line it hits), the barrier, and an acquire fence.  All four waves of
//          a workgroup run on one CU and load through that one L1, so the walk's ordinary loads find the row.  The walk therefore
//          decodes the stored codes and parameters: the arithmetic that meets the new row is the chain's.
//          No other workgroup reads the row: the other chunks of the sequence end before it (t1), and the masked over-read of the tile
//          loop -- row 0 of the cache for a token that is not `ok` -- stays behind its selects, as in paged_decode.
// Nothing waits on another workgroup: no flag, no ticket, no spinning.  The owner pays one load, one store and a barrier before its first
// tile; every other workgroup starts its walk as soon as its q is rotated.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "mx_kernels.h"
#include "mx_kv_decode.h"
#include "mx_paged_kv.h"
#include "mx_qknorm.h"
#include "mx_rope.h"

namespace {

using namespace mm::kv;
using mm::PagedKV;

// 16 bytes that are only known to lie on a dword: q | k | v and cos | sin are views into the caller's projection
typedef unsigned v4u_dw __attribute__((ext_vector_type(4), aligned(4)));
typedef float v4f_dw __attribute__((ext_vector_type(4), aligned(4)));

struct StepArgs {
    DecodeArgs d;                      // d.q is unused: the walk takes q from registers
    const uint16_t *q, *k, *v, *cos, *sin;
    uint16_t *q_out;                   // optional
    int64_t qkv_stride, cs_stride;     // elements per token
};

struct StepNormArgs : StepArgs {
    const uint16_t *q_weight, *k_weight;   // bf16 [128] each
    float eps;
};

// NORM (mm_rope_append_decode_qknorm): q and k pass mx_qknorm.h's rule before their rotation.  q: a lane norms the block it holds and
// the block of its rotate_half partners (qknorm_blocks: the row's sum needs one exchange, with lane ^ 16), with the two blocks of the
// weight loaded next to its cos / sin block; the four waves repeat the norm as they repeat the rotation.  k: wave 0 of the owning
// workgroup, in rope_pair's layout (qknorm_pair).  No LDS and no barrier beyond the one below.
template <int KIND, int GP, bool NORM>
__global__ __launch_bounds__(256) void rope_append_decode_kernel(const std::conditional_t<NORM, StepNormArgs, StepArgs> st) {
    constexpr int WALK = WALK_STEP;
    const DecodeArgs &a = st.d;
    const SharedArgs sh = {};
    v4u step_q[4];
    {
        const int b = blockIdx.z, kvh = blockIdx.y, chunk = blockIdx.x, wave = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, kq = l >> 4;
        const int64_t in = (int64_t)b * st.qkv_stride;
        // ---- q: dims 32 kq + 8 s + j of head c, step s = step_q[s]
#pragma unroll
        for (int s = 0; s < 4; ++s) step_q[s] = v4u{0, 0, 0, 0};
        if (c < a.g) {
            const int hq = kvh * a.g + c;
            const uint16_t *row = st.q + in + (int64_t)hq * HD;
            const v4u_dw *x = (const v4u_dw *)(row + 32 * kq), *r = (const v4u_dw *)(row + 32 * (kq ^ 2));
            const v4u_dw *cs = (const v4u_dw *)(st.cos + (int64_t)b * st.cs_stride + 32 * kq);
            const v4u_dw *sn = (const v4u_dw *)(st.sin + (int64_t)b * st.cs_stride + 32 * kq);
            const uint32_t flip = kq < 2 ? 0x80008000u : 0u;                   // rotate_half: -x[d + 64] below 64, x[d - 64] above
            if constexpr (NORM) {
                const v4u_dw *gx = (const v4u_dw *)(st.q_weight + 32 * kq), *gp = (const v4u_dw *)(st.q_weight + 32 * (kq ^ 2));
                v4u xn[4], pn[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) xn[s] = x[s], pn[s] = r[s];
                const float rscale = qknorm_blocks_rscale(xn, pn, st.eps);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const v4u wx = gx[s], wp = gp[s];
#pragma unroll
                    for (int j = 0; j < 4; ++j) xn[s][j] = qkn_scale(xn[s][j], rscale, wx[j]), pn[s][j] = qkn_scale(pn[s][j], rscale, wp[j]);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const v4u cc = cs[s], ss = sn[s];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t xv = xn[s][j], p = pn[s][j] ^ flip;
                        step_q[s][j] = rope_one(xv & 0xffffu, p & 0xffffu, cc[j] & 0xffffu, ss[j] & 0xffffu) |
                                       (rope_one(xv >> 16, p >> 16, cc[j] >> 16, ss[j] >> 16) << 16);
                    }
                }
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const v4u xs = x[s], rs = r[s], cc = cs[s], ss = sn[s];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t p = rs[j] ^ flip;
                        step_q[s][j] = rope_one(xs[j] & 0xffffu, p & 0xffffu, cc[j] & 0xffffu, ss[j] & 0xffffu) |
                                       (rope_one(xs[j] >> 16, p >> 16, cc[j] >> 16, ss[j] >> 16) << 16);
                    }
                }
            }
            if (st.q_out && chunk == 0 && wave == 0) {
                // stored as floats: an integer store may alias the page table for all the compiler knows (rope_append.hip)
                v4f_dw *dst = (v4f_dw *)(st.q_out + ((int64_t)b * a.Hq + hq) * HD + 32 * kq);
#pragma unroll
                for (int s = 0; s < 4; ++s) dst[s] = __builtin_bit_cast(v4f, step_q[s]);
            }
        }
        // ---- the new row, in the workgroup whose chunk [t0, t1) holds position len - 1 (the chunk rule of the walk below)
        const int len = seq_len(a.kv, b), t0 = chunk * a.chunk;
        const int t1 = chunk == a.nc - 1 ? len : min(len, t0 + a.chunk);
        if (len - 1 >= t0 && len - 1 < t1) {
            if (wave < 2) {                                                    // wave 0: K, wave 1: V, as rope_kv_append_kernel
                uint32_t two = ((const uint32_t *)((wave ? st.v : st.k) + in + (int64_t)kvh * HD))[l];
                if (wave == 0) {
                    const uint32_t cs = ((const uint32_t *)(st.cos + (int64_t)b * st.cs_stride))[l];
                    const uint32_t sn = ((const uint32_t *)(st.sin + (int64_t)b * st.cs_stride))[l];
                    if constexpr (NORM) two = qknorm_pair(two, ((const uint32_t *)st.k_weight)[l], st.eps);
                    two = rope_pair(two, cs, sn, l);
                }
                const int64_t row = append_row_at(a.kv, b, len - 1, len, wave, kvh);
                if (row >= 0) store_row<KIND>(a.kv, row, l, two);
            }
            __syncthreads();                                                   // release, barrier, acquire at workgroup scope: see above
        }
    }
#include "kv_decode_tiles.inc"
}

template <int KIND, bool NORM>
hipError_t launch_step_g(const std::conditional_t<NORM, StepNormArgs, StepArgs> &st, hipStream_t stream) {
    const dim3 grid(st.d.nc, st.d.kv.Hkv, st.d.kv.B);
    if (st.d.g <= 4) rope_append_decode_kernel<KIND, 4, NORM><<<grid, 256, 0, stream>>>(st);
    else if (st.d.g <= 8) rope_append_decode_kernel<KIND, 8, NORM><<<grid, 256, 0, stream>>>(st);
    else rope_append_decode_kernel<KIND, 16, NORM><<<grid, 256, 0, stream>>>(st);
    return hipGetLastError();
}

template <bool NORM>
hipError_t launch_step_kind(const std::conditional_t<NORM, StepNormArgs, StepArgs> &st, hipStream_t stream) {
    if (st.d.kv.kind == KV_INT4) return launch_step_g<KV_INT4, NORM>(st, stream);
    if (st.d.kv.kind == KV_FP8) return launch_step_g<KV_FP8, NORM>(st, stream);
    return launch_step_g<KV_BF16, NORM>(st, stream);
}

}  // namespace

namespace mm {

hipError_t launch_rope_append_decode(const PagedKV &kv, const void *q, const void *k, const void *v, int64_t qkv_stride, int Hq, const void *cos,
                                     const void *sin, int64_t cs_stride, int max_seq_len, float sm_scale, void *ws, void *q_out, void *o,
                                     hipStream_t stream, const void *q_weight, const void *k_weight, float eps) {
    StepNormArgs st;                                                           // q_weight != nullptr: the QK-norm form, both weights given
    st.d.kv = kv;
    st.d.q = nullptr;
    st.d.ws = (float *)ws;
    st.d.o = (uint16_t *)o;
    st.d.Hq = Hq;
    st.d.g = Hq / kv.Hkv;
    kv_decode_split(kv.B, kv.Hkv, max_seq_len, 0, &st.d.nc, &st.d.chunk);      // mm_paged_decode's plan
    st.d.scale_log2 = kv_scale_log2(sm_scale);
    st.d.window = 0;
    st.q = (const uint16_t *)q;
    st.k = (const uint16_t *)k;
    st.v = (const uint16_t *)v;
    st.cos = (const uint16_t *)cos;
    st.sin = (const uint16_t *)sin;
    st.q_out = (uint16_t *)q_out;
    st.qkv_stride = qkv_stride;
    st.cs_stride = cs_stride;
    st.q_weight = (const uint16_t *)q_weight;
    st.k_weight = (const uint16_t *)k_weight;
    st.eps = eps;
    const hipError_t e = q_weight ? launch_step_kind<true>(st, stream) : launch_step_kind<false>(st, stream);
    if (e != hipSuccess || st.d.nc == 1) return e;
    return launch_paged_decode_merge(st.d, stream);
}

}  // namespace mm
