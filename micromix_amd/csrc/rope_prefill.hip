// RoPE + paged KV append in the prefill shape (include/micromix_rope.h, mm_rope_prefill, which states the function): what
// rope_append.hip does for decode -- one token per workgroup, a dword per lane -- for a prompt's worth of tokens, and with the outputs a
// dense attention over the prompt needs: the rotated q, and K / V as a reader of the cache slot gets them back (k_out, v_out).  The
// cache is optional: without one this is plain RoPE.
// The kernel holds no rule of its own: the element rule of RoPE is mx_rope.h's (rope_one, shared with rope_append.hip), the slot rule
// and the int4 / fp8 / bf16 rules are mx_paged_kv.h's (append_row, store_row8: the element rules store_row is made of).
//
// Design.  A workgroup owns TPW = MM_ROPE_PREFILL_TOKENS = 8 consecutive tokens and is G waves wide, 1 <= G <= 16.
//   Rows     Eight lanes own a 128-element head row: lane j of the eight holds elements 8 j .. 8 j + 7 and 64 + 8 j .. 64 + 8 j + 7, two
//            16-byte loads and two 16-byte stores, and both partners of every RoPE pair are its own: no cross-lane exchange, no LDS.
//   Waves    A wave is 8 row groups, one per token of the workgroup, and all eight work on the same row number at a time: the R rows
//            of a token -- Hq of q, then Hkv of K, then Hkv of V -- are dealt to the G waves round robin (wave w: rows w, w + G, ..), so
//            whether a row is rotated, and where it goes, is uniform over a wave.  G = ceil(R / 4): four rows per group (Llama-3-8B,
//            R = 48: 12 waves, 768 lanes, 512 workgroups at T = 4096), enough lanes that the loads of the whole prompt are in flight
//            together; past G = 16 a group takes more rows.
//   Tables   A group loads its token's cos / sin chunks once, both halves (a table need not repeat its halves), 16 registers, and
//            keeps them over its rows.
//   Slots    Only the waves that hold a K or V row look a slot up, each lane for its own token, ahead of the wave's first row: the
//            eight dependent chains of a wave (binary search over append_indptr, page count, last page, page index) run side by side
//            instead of one per workgroup behind scalar loads, and the waves that rotate q do not wait for them.  The row of (K / V,
//            head) follows from the token's K row of head 0 by an offset (row_of).
//   Quantize The row's min / max (int4) or amax (fp8) is a three-step DPP exchange among the eight lanes.  An int4 lane stores two
//            dwords of codes, an fp8 lane two 8-byte halves, a bf16 lane two 16-byte halves; lane 0 of the eight stores the 4-byte
//            (scale, zero).  No byte-wide stores.  The value a reader gets back is formed from the codes in registers.
//   Offsets  64-bit throughout.
// Registers (hipcc 7, -O3, gfx950): see DESIGN 7w for the compiler's report; no scratch, no LDS.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/micromix_rope.h"
#include "mx_kernels.h"
#include "mx_paged_kv.h"
#include "mx_qknorm.h"
#include "mx_rope.h"

namespace {

using namespace mm::kv;

constexpr int TPW = MM_ROPE_PREFILL_TOKENS, MAX_WAVES = 16;
static_assert(TPW == 8, "a wave is one 8-lane row group per token of the workgroup");

struct RopePrefillArgs {
    mm::PagedKV kv;                    // all zero without a cache
    const int *append_indptr;
    const uint16_t *q, *k, *v, *cos, *sin;
    uint16_t *q_out, *k_out, *v_out;
    int64_t qkv_stride, cs_stride;     // elements per token
    int T, Hq, Hkv, R, G;              // R rows of a token are visited: Hq + Hkv, + Hkv when V goes anywhere
    int cache;
};

// rotates a row in place: lo = elements 8 j .. 8 j + 7, hi = 64 + 8 j .. 64 + 8 j + 7, cs / sn the same chunks of the token's table row
__device__ inline void rope_row(v4u &lo, v4u &hi, const v4u (&cs)[2], const v4u (&sn)[2]) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const uint32_t xl = lo[m], xh = hi[m], nh = xh ^ 0x80008000u;      // rotate_half: -x[d + 64] below 64, x[d - 64] above
        lo[m] = rope_one(xl & 0xffffu, nh & 0xffffu, cs[0][m] & 0xffffu, sn[0][m] & 0xffffu) |
                (rope_one(xl >> 16, nh >> 16, cs[0][m] >> 16, sn[0][m] >> 16) << 16);
        hi[m] = rope_one(xh & 0xffffu, xl & 0xffffu, cs[1][m] & 0xffffu, sn[1][m] & 0xffffu) |
                (rope_one(xh >> 16, xl >> 16, cs[1][m] >> 16, sn[1][m] >> 16) << 16);
    }
}

struct RopePrefillNormArgs : RopePrefillArgs {
    const uint16_t *q_weight, *k_weight;       // bf16 [128] each
    float eps;
};

// NORM: q and k rows pass mx_qknorm.h's rule (qknorm_row8) before the rotation.  A group loads its two chunks of the q weight next to
// its cos / sin chunks and keeps them over its q rows; a wave's rows ascend, q before K, so the chunks of the k weight replace them
// once, at the wave's first K row.
template <int KIND, bool NORM>
__global__ __launch_bounds__(64 * MAX_WAVES) void rope_prefill_kernel(const std::conditional_t<NORM, RopePrefillNormArgs, RopePrefillArgs> a) {
    const int j = threadIdx.x & 7, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * TPW + ((threadIdx.x >> 3) & (TPW - 1));
    if (i >= a.T) return;                                     // whole row groups leave: the eight lanes of a group stay together
    const int rot_rows = a.Hq + a.Hkv;
    // the slot, where this wave will store a K or V row: its last row is one
    int64_t row0 = -1;
    if (a.cache && wave + (a.R - 1 - wave) / a.G * a.G >= a.Hq) row0 = append_row(a.kv, a.append_indptr, (int)i, 0, 0);
    v4u cs[2] = {}, sn[2] = {};
    if (wave < rot_rows) {
        const v4u *c = (const v4u *)(a.cos + i * a.cs_stride), *s = (const v4u *)(a.sin + i * a.cs_stride);
        cs[0] = c[j], cs[1] = c[HD / 16 + j], sn[0] = s[j], sn[1] = s[HD / 16 + j];
    }
    [[maybe_unused]] v4u w[2] = {};
    [[maybe_unused]] bool w_is_k = wave >= a.Hq;
    if constexpr (NORM) {
        if (wave < rot_rows) {
            const v4u *g = (const v4u *)(w_is_k ? a.k_weight : a.q_weight);
            w[0] = g[j], w[1] = g[HD / 16 + j];
        }
    }
    for (int r = wave; r < a.R; r += a.G) {
        const bool isq = r < a.Hq, isk = !isq && r < rot_rows;
        const int h = isq ? r : isk ? r - a.Hq : r - rot_rows;
        const v4u *src = (const v4u *)((isq ? a.q : isk ? a.k : a.v) + i * a.qkv_stride + (int64_t)h * HD);
        v4u lo = src[j], hi = src[HD / 16 + j];
        if constexpr (NORM) {
            if (isk && !w_is_k) {
                const v4u *g = (const v4u *)a.k_weight;
                w[0] = g[j], w[1] = g[HD / 16 + j], w_is_k = true;
            }
            if (r < rot_rows) qknorm_row8(lo, hi, w, a.eps);
        }
        if (r < rot_rows) rope_row(lo, hi, cs, sn);
        v4u *dst;
        if (isq) {                                            // q: every token, whatever its cache slot
            dst = (v4u *)(a.q_out + (i * a.Hq + h) * HD);
        } else {
            store_row8<KIND>(a.kv, row0 >= 0 ? row_of(a.kv, row0, isk ? 0 : 1, h) : -1, j, lo, hi);
            uint16_t *out = isk ? a.k_out : a.v_out;
            if (!out) continue;
            dst = (v4u *)(out + (i * a.Hkv + h) * HD);
        }
        dst[j] = lo;
        dst[HD / 16 + j] = hi;
    }
}

}  // namespace

namespace mm {

hipError_t launch_rope_prefill(const PagedKV *kv, const void *q, const void *k, const void *v, int64_t qkv_stride, int Hq, int Hkv,
                               const void *cos, const void *sin, int64_t cs_stride, const int *append_indptr, int T, void *q_out, void *k_out,
                               void *v_out, hipStream_t stream, const void *q_weight, const void *k_weight, float eps) {
    RopePrefillNormArgs a{};                                  // q_weight != nullptr: the QK-norm form, both weights given
    if (kv) a.kv = *kv;
    a.cache = kv != nullptr;
    a.append_indptr = append_indptr;
    a.q = (const uint16_t *)q;
    a.k = (const uint16_t *)k;
    a.v = (const uint16_t *)v;
    a.cos = (const uint16_t *)cos;
    a.sin = (const uint16_t *)sin;
    a.q_out = (uint16_t *)q_out;
    a.k_out = (uint16_t *)k_out;
    a.v_out = (uint16_t *)v_out;
    a.qkv_stride = qkv_stride;
    a.cs_stride = cs_stride;
    a.T = T;
    a.Hq = Hq;
    a.Hkv = Hkv;
    a.R = Hq + ((kv || k_out || v_out) ? Hkv : 0) + ((kv || v_out) ? Hkv : 0);     // rows that go nowhere are not read
    a.G = (a.R + 3) / 4 < MAX_WAVES ? (a.R + 3) / 4 : MAX_WAVES;
    const unsigned grid = (unsigned)(((int64_t)T + TPW - 1) / TPW);
    const int kind = kv ? kv->kind : KV_BF16;                 // without a cache K and V are handed on as they are: the bf16 kind's values
    a.q_weight = (const uint16_t *)q_weight;
    a.k_weight = (const uint16_t *)k_weight;
    a.eps = eps;
    const RopePrefillArgs &plain = a;
    if (q_weight) {
        if (kind == KV_INT4) rope_prefill_kernel<KV_INT4, true><<<grid, 64 * a.G, 0, stream>>>(a);
        else if (kind == KV_FP8) rope_prefill_kernel<KV_FP8, true><<<grid, 64 * a.G, 0, stream>>>(a);
        else rope_prefill_kernel<KV_BF16, true><<<grid, 64 * a.G, 0, stream>>>(a);
    } else if (kind == KV_INT4) rope_prefill_kernel<KV_INT4, false><<<grid, 64 * a.G, 0, stream>>>(plain);
    else if (kind == KV_FP8) rope_prefill_kernel<KV_FP8, false><<<grid, 64 * a.G, 0, stream>>>(plain);
    else rope_prefill_kernel<KV_BF16, false><<<grid, 64 * a.G, 0, stream>>>(plain);
    return hipGetLastError();
}

}  // namespace mm
