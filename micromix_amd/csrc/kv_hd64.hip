// The paged KV cache for 64-wide heads (include/micromix_kv_hd64.h states the functions): RoPE + append (mm_rope_kv_append_hd64) and GQA
// split-KV decode attention (mm_paged_decode_hd64) over kv_data [max_pages, L, 2, Hkv, P, 64], bf16 or e4m3 codes with an fp16 (2^e, 0)
// pair per row.  The page walk and the element rules of the fp8 kind are mx_paged_kv.h's (they do not depend on the row width); the
// kernels are this file's own.
//
// Decode.  One workgroup (4 waves) per (sequence, kv head, chunk) serves all g = Hq / Hkv heads; a wave walks 64-token tiles of the chunk,
// tile n of wave w being tokens t0 + 64 (w + 4 n) ...  A bf16 tile is 8 KB of K and 8 KB of V.
//   depth    a wave holds TWO tiles in registers (Tile a, b): the K and V loads of tile n + 1 are issued before the scores, softmax and
//            p.V of tile n, so the memory latency of a tile lies under the arithmetic of the one before, and what the arithmetic waits
//            for is s_waitcnt vmcnt(N) with N the loads of the next tile, not 0.  The page-table entry of a token is read one tile
//            further ahead still (lane l reads the entry of token l of tile n + 2 while tile n + 1's loads are issued), so no K or V load
//            waits on an index load.  The loop is unrolled by two so that the two register sets swap roles without moves.
//            -DMM_KV_HD64_NO_DEPTH (tools/time_kv_hd64.py's ablation, never the product build) issues tile n + 1 after tile n's p.V.
//   rows     lane l turns its entry into the K row of its token (64-bit, -1: past the chunk or off the cache) and the wave passes the 64
//            rows through LDS: the score lanes read 4 of them, the p.V lanes 8
//   scores   v_mfma_f32_16x16x32_bf16, A = q (16 head rows, g used; lane (c, kq) holds dims 16 kq + 8 s + j of head c in step s), B = the
//            K row of token 16 G + c, the same 16 dims: two MFMAs per 16 tokens, eight per tile.  fp8: the codes widened by
//            v_cvt_scalef32_pk_bf16_fp8 at scale 1.0 (exact), and the row's 2^e applied to the fp32 score
//   softmax  online, log2 domain: the running max is kept scaled, p = exp2(fma(score, sm_scale * log2 e, -max)), one fma per score; only
//            the tile max crosses lanes (16 token lanes, four rows per lane); l stays a per-lane partial until the end
//   p.V      VALU, fp32: lane (dg, tg) = (l & 7, l >> 3) owns dims 8 dg .. 8 dg + 7 of tokens 8 i + tg, acc[h][8] += p[h] * v, p (times the V
//            row's 2^e for fp8) through LDS as [token][head]; p is never rounded to bf16
//   merge    the waves through LDS; one chunk: the workgroup writes o; otherwise (m, l, o) partials that a small second launch combines
// Append.  mm_rope_qk_hd64's shape extended to write the cache: a workgroup owns 16 tokens, four lanes a 64-element row, lane j holding
// elements 8 j .. 8 j + 7 and their RoPE partners 32 + 8 j .. 32 + 8 j + 7; wave w takes the rows w, w + G, .. of q | k | v.  Every lane
// finds its token's slot on its own, the 16 lookups of a workgroup side by side.  fp8: the row's amax is two quad_perm DPP steps
// among the four lanes; codes leave as 8-byte stores, bf16 as 16-byte stores, the (2^e, 0) pair as one dword.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/micromix_kv_hd64.h"
#include "mx_kv_hd64.h"
#include "mx_paged_kv.h"
#include "mx_rope.h"

namespace {

using namespace mm::kv;
using mm::PagedKV;

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int D = 64;                                   // head_dim
constexpr int WAVES = MM_KV_HD64_DECODE_WAVES, TILE = MM_KV_HD64_DECODE_TILE;
static_assert(WAVES == 4 && TILE == 64, "a wave's 64 lanes are the 64 tokens of a tile; the LDS below is sized for four waves");

template <int KIND> constexpr int row_bytes() { return KIND == KV_BF16 ? 2 * D : D; }

struct Decode64 {
    PagedKV kv;
    const uint16_t *q;
    float *ws;                 // partials: o [B, Hkv, nc, g, 64], then (m, l) [B, Hkv, nc, g, 2]
    uint16_t *o;
    int Hq, g, nc, chunk;
    float scale_log2;          // sm_scale * log2(e)
};

// what a wave holds of one tile: the K operand of its score lanes, the V rows of its p.V lanes, fp8 their rows' params, and which exist
template <int KIND>
struct Tile {
    v4u k[4][KIND == KV_BF16 ? 2 : 1];                  // token 16 G + c, dims 16 kq .. 16 kq + 15
    v4u vb[KIND == KV_BF16 ? 8 : 1];                    // bf16: token 8 i + tg, dims 8 dg .. 8 dg + 7
    v2u vc[KIND == KV_FP8 ? 8 : 1];                     // fp8: the same as codes
    uint32_t pk[KIND == KV_FP8 ? 4 : 1], pv[KIND == KV_FP8 ? 4 : 1];
    uint32_t okk, okv;                                  // bit G / bit i: the token exists
};

// lane l's token of the tile that starts at tb: its page-table entry, -1 past the chunk (no read)
__device__ inline int page_entry(const PagedKV &kv, const int *pages, int64_t tb, int t1, int l) {
    const int64_t t = tb + l;
    return t < t1 ? pages[(int)t / kv.P] : -1;
}

// issues the loads of the tile that starts at tb; `page` is page_entry() of it.  rows: this wave's 64 LDS entries
template <int KIND>
__device__ inline void issue_tile(const PagedKV &kv, int64_t *rows, int page, int tb, int kvh, int l, Tile<KIND> &t) {
    const int c = l & 15, kq = l >> 4, dg = l & 7, tg = l >> 3;
    rows[l] = page >= 0 && page < kv.max_pages ? kv_row(kv, page, 0, kvh, (tb + l) % kv.P) : -1;   // page >= 0: tb + l is a token
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's own exchange (LDS operations of a wave run in order)
    const int64_t voff = v_offset(kv);
    t.okk = t.okv = 0;
#pragma unroll
    for (int G = 0; G < 4; ++G) {
        int64_t r = rows[16 * G + c];
        t.okk |= (r >= 0 ? 1u : 0u) << G;
        r = r >= 0 ? r : 0;                              // row 0 is always there to address; what it holds is never used
        const v4u *src = (const v4u *)(kv.data + r * row_bytes<KIND>()) + (KIND == KV_BF16 ? 2 : 1) * kq;
        t.k[G][0] = src[0];
        if constexpr (KIND == KV_BF16) t.k[G][1] = src[1];
        if constexpr (KIND == KV_FP8) {
            t.pk[G] = ((const uint32_t *)kv.param)[r];
            t.pv[G] = ((const uint32_t *)kv.param)[r + voff];
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int64_t r = rows[8 * i + tg];
        t.okv |= (r >= 0 ? 1u : 0u) << i;
        r = (r >= 0 ? r : 0) + voff;
        if constexpr (KIND == KV_BF16) t.vb[i] = ((const v4u *)(kv.data + r * row_bytes<KIND>()))[dg];
        else t.vc[i] = ((const v2u *)(kv.data + r * row_bytes<KIND>()))[dg];
    }
    asm volatile("" ::: "memory");                       // the next tile writes `rows` after these reads
}

// scores, online softmax and p.V of one loaded tile
template <int KIND, int GP>
__device__ inline void consume_tile(const Tile<KIND> &t, const v8bf (&qa)[2], float scale_log2, float (&m)[4], float (&lsum)[4],
                                    float (&acc)[GP][8], float (*sp)[16], float *salpha, int l) {
    const int c = l & 15, kq = l >> 4, tg = l >> 3;
    float sc[4][4], sv[4];
#pragma unroll
    for (int G = 0; G < 4; ++G) {
        const bool ok = (t.okk >> G) & 1u;
        v4f d = {0.0f, 0.0f, 0.0f, 0.0f};
        float sk = 1.0f;
        if constexpr (KIND == KV_BF16) {
            d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[0], __builtin_bit_cast(v8bf, t.k[G][0]), d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[1], __builtin_bit_cast(v8bf, t.k[G][1]), d, 0, 0, 0);
            sv[G] = 1.0f;                                // p is 0 for a token that does not exist
        } else {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const v2u lo = fp8x4_to_bf16(t.k[G][0][2 * s]), hi = fp8x4_to_bf16(t.k[G][0][2 * s + 1]);
                d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[s], __builtin_bit_cast(v8bf, (v4u{lo.x, lo.y, hi.x, hi.y})), d, 0, 0, 0);
            }
            sk = scale_of(t.pk[G]);
            sv[G] = ok ? scale_of(t.pv[G]) : 0.0f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[G][r] = ok ? sk * d[r] : -INFINITY;
    }
    float pw[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float mt = fmaxf(fmaxf(sc[0][r], sc[1][r]), fmaxf(sc[2][r], sc[3][r]));
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) mt = fmaxf(mt, __shfl_xor(mt, o));
        const float mn = fmaxf(m[r], mt * scale_log2);   // scale_log2 > 0: the max of the scaled scores
        const float base = mn == -INFINITY ? 0.0f : mn;  // a tile whose tokens all lie off the cache, before any other
        const float alpha = exp2f(m[r] - base);
        float ps = 0.0f;
#pragma unroll
        for (int G = 0; G < 4; ++G) {
            const float p = exp2f(fmaf(sc[G][r], scale_log2, -base));
            ps += p;
            pw[G][r] = p * sv[G];
        }
        m[r] = mn;
        lsum[r] = lsum[r] * alpha + ps;
        if (c == 0) salpha[4 * kq + r] = alpha;
    }
#pragma unroll
    for (int G = 0; G < 4; ++G) *(v4f *)&sp[16 * G + c][4 * kq] = v4f{pw[G][0], pw[G][1], pw[G][2], pw[G][3]};
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int h = 0; h < GP; h += 4) {
        const v4f al = *(const v4f *)&salpha[h];
#pragma unroll
        for (int hh = 0; hh < 4; ++hh)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[h + hh][e] *= al[hh];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool ok = (t.okv >> i) & 1u;
        float vv[8];
        if constexpr (KIND == KV_BF16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t w = ok ? t.vb[i][j] : 0u;
                vv[2 * j] = bf16f(w & 0xffffu);
                vv[2 * j + 1] = bf16f(w >> 16);
            }
        } else {
            fp8x4_to_f32(ok ? t.vc[i].x : 0u, vv);
            fp8x4_to_f32(ok ? t.vc[i].y : 0u, vv + 4);
        }
#pragma unroll
        for (int h = 0; h < GP; h += 4) {
            const v4f p = *(const v4f *)&sp[8 * i + tg][h];
#pragma unroll
            for (int hh = 0; hh < 4; ++hh)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[h + hh][e] = fmaf(p[hh], vv[e], acc[h + hh][e]);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads of this tile's exchange done before the next tile writes it
}

template <int KIND, int GP>
__global__ __launch_bounds__(64 * WAVES) void paged_decode_hd64_kernel(const Decode64 a) {
    __shared__ __attribute__((aligned(16))) float s_p[WAVES][TILE][16];             // (p * V scale) of the tile, [token][head]
    __shared__ __attribute__((aligned(16))) float s_alpha[WAVES][16];
    __shared__ int64_t s_row[WAVES][TILE];             // K row of each token of the tile being loaded (-1: none)
    __shared__ float s_o[WAVES][GP][D];
    __shared__ float s_ml[WAVES][GP][2];

    const int chunk = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, kq = l >> 4, dg = l & 7, tg = l >> 3;
    const PagedKV &kv = a.kv;
    const int g = a.g;
    const int len = seq_len(kv, b);
    const int t0 = chunk * a.chunk;
    const int t1 = chunk == a.nc - 1 ? len : min(len, t0 + a.chunk);   // the last chunk runs to the end, whatever max_seq_len said
    const int *pages = kv.indices + kv.indptr[b];

    v8bf qa[2];
    {
        const v4u *qrow = (const v4u *)(a.q + ((int64_t)b * a.Hq + (int64_t)kvh * g + (c < g ? c : 0)) * D + 16 * kq);
        qa[0] = __builtin_bit_cast(v8bf, c < g ? qrow[0] : v4u{0, 0, 0, 0});
        qa[1] = __builtin_bit_cast(v8bf, c < g ? qrow[1] : v4u{0, 0, 0, 0});
    }
    float m[4], lsum[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; lsum[r] = 0.0f; }
    float acc[GP][8];
#pragma unroll
    for (int h = 0; h < GP; ++h)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[h][e] = 0.0f;

    constexpr int STEP = TILE * WAVES;
    int tb = t0 + TILE * wave;
    if (tb < t1) {
        Tile<KIND> tile_a, tile_b;
        const int first = page_entry(kv, pages, tb, t1, l);
        int ahead_a = page_entry(kv, pages, (int64_t)tb + STEP, t1, l), ahead_b = -1;   // the entries of the next tile and of the one after
        issue_tile<KIND>(kv, s_row[wave], first, tb, kvh, l, tile_a);
        // one step: the tile in `cur` is loaded (or on its way), tb is its first token; `near` holds the next tile's entry and `far`
        // receives that of the tile after it.  Two variables that swap like the tiles: a load into the one just read would need a copy,
        // and the copy a wait for every load in flight
        auto step = [&](Tile<KIND> &cur, Tile<KIND> &nxt, const int &near, int &far) {
            // Unconditional: past the chunk's last tile `near` is -1 in every lane and the loads read row 0, unused.  A branch here
            // would merge a path with 17 younger loads and one with none, and every wait below would be counted for the latter
#ifndef MM_KV_HD64_NO_DEPTH
            far = page_entry(kv, pages, (int64_t)tb + 2 * STEP, t1, l);   // the index load first: waiting for it leaves the tile's loads in flight
            issue_tile<KIND>(kv, s_row[wave], near, tb + STEP, kvh, l, nxt);
            __builtin_amdgcn_sched_barrier(0);           // the next tile's loads stay above this tile's arithmetic
            consume_tile<KIND, GP>(cur, qa, a.scale_log2, m, lsum, acc, s_p[wave], s_alpha[wave], l);
#else
            consume_tile<KIND, GP>(cur, qa, a.scale_log2, m, lsum, acc, s_p[wave], s_alpha[wave], l);
            __builtin_amdgcn_sched_barrier(0);
            far = page_entry(kv, pages, (int64_t)tb + 2 * STEP, t1, l);
            issue_tile<KIND>(kv, s_row[wave], near, tb + STEP, kvh, l, nxt);
#endif
            tb += STEP;
            return tb < t1;
        };
        while (step(tile_a, tile_b, ahead_a, ahead_b) && step(tile_b, tile_a, ahead_b, ahead_a)) {}
    }

    // ---- wave totals: acc over the eight token groups tg, l over the 16 token lanes c
#pragma unroll
    for (int h = 0; h < GP; ++h)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            acc[h][e] += __shfl_xor(acc[h][e], 8);
            acc[h][e] += __shfl_xor(acc[h][e], 16);
            acc[h][e] += __shfl_xor(acc[h][e], 32);
        }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) lsum[r] += __shfl_xor(lsum[r], o);
    if (c == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * kq + r < GP) {
                s_ml[wave][4 * kq + r][0] = m[r];
                s_ml[wave][4 * kq + r][1] = lsum[r];
            }
    }
    if (tg == 0) {
#pragma unroll
        for (int h = 0; h < GP; ++h)
#pragma unroll
            for (int e = 0; e < 8; ++e) s_o[wave][h][8 * dg + e] = acc[h][e];
    }
    __syncthreads();

    // ---- merge the four waves: thread -> (head, a pair of the 64 dims)
    for (int idx = threadIdx.x; idx < g * (D / 2); idx += 64 * WAVES) {
        const int h = idx / (D / 2), d = 2 * (idx % (D / 2));
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) M = fmaxf(M, s_ml[w][h][0]);
        float ls = 0.0f, o0 = 0.0f, o1 = 0.0f;
        if (M != -INFINITY) {
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                const float f = exp2f(s_ml[w][h][0] - M);      // 0 for a wave without tokens
                ls += f * s_ml[w][h][1];
                o0 += f * s_o[w][h][d];
                o1 += f * s_o[w][h][d + 1];
            }
        }
        const int hq = kvh * g + h;
        if (a.nc == 1) {
            const float inv = ls > 0.0f ? 1.0f / ls : 0.0f;
            *(uint32_t *)(a.o + ((int64_t)b * a.Hq + hq) * D + d) = pack_bf(o0 * inv, o1 * inv);
        } else {
            const int64_t part = (((int64_t)b * kv.Hkv + kvh) * a.nc + chunk) * g + h;
            *(float2 *)(a.ws + part * D + d) = make_float2(o0, o1);
            if (d == 0) *(float2 *)(a.ws + (int64_t)kv.B * a.Hq * a.nc * D + part * 2) = make_float2(M, ls);
        }
    }
}

// mx_paged_kv.h's merge_chunks with rows of 64 (that one indexes its partials by the 128 row): combines the nc chunk partials of two
// (sequence, query head) rows per wave, a thread per pair of dims
__global__ __launch_bounds__(64) void paged_decode_hd64_merge_kernel(const Decode64 a) {
    const int hq = 2 * blockIdx.x + (threadIdx.x >> 5), b = blockIdx.y, d = 2 * (threadIdx.x & 31);
    if (hq >= a.Hq) return;
    const int kvh = hq / a.g, h = hq % a.g;
    const float *ml = a.ws + (int64_t)a.kv.B * a.Hq * a.nc * D;
    const int64_t first = (((int64_t)b * a.kv.Hkv + kvh) * a.nc) * a.g + h;      // part index of chunk 0; chunk stride g
    float M = -INFINITY;
    for (int c = 0; c < a.nc; ++c) M = fmaxf(M, ml[(first + (int64_t)c * a.g) * 2]);
    float ls = 0.0f, o0 = 0.0f, o1 = 0.0f;
    if (M != -INFINITY) {
        for (int c = 0; c < a.nc; ++c) {
            const int64_t p = first + (int64_t)c * a.g;
            const float f = exp2f(ml[p * 2] - M);
            const float2 part = *(const float2 *)(a.ws + p * D + d);
            ls += f * ml[p * 2 + 1];
            o0 += f * part.x;
            o1 += f * part.y;
        }
    }
    const float inv = ls > 0.0f ? 1.0f / ls : 0.0f;
    *(uint32_t *)(a.o + ((int64_t)b * a.Hq + hq) * D + d) = pack_bf(o0 * inv, o1 * inv);
}

template <int KIND>
hipError_t launch_decode_g(const Decode64 &a, hipStream_t stream) {
    const dim3 grid(a.nc, a.kv.Hkv, a.kv.B);
    if (a.g <= 4) paged_decode_hd64_kernel<KIND, 4><<<grid, 64 * WAVES, 0, stream>>>(a);
    else if (a.g <= 8) paged_decode_hd64_kernel<KIND, 8><<<grid, 64 * WAVES, 0, stream>>>(a);
    else paged_decode_hd64_kernel<KIND, 16><<<grid, 64 * WAVES, 0, stream>>>(a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int TPW = MM_KV_HD64_APPEND_TOKENS, MAX_WAVES = 16;
static_assert(TPW == 16, "a wave is one 4-lane row group per token of the workgroup");

struct Append64 {
    PagedKV kv;
    const uint16_t *q, *k, *v, *cos, *sin;
    uint16_t *q_out, *k_out, *v_out;
    const int *append_indptr;
    int64_t qkv_stride, cs_stride;     // elements per token
    int T, Hq, G;                      // Hq: the q rows to do (0 without q); G: waves
};

// max over the four lanes of a row group: lane ^ 1, then lane ^ 2 (quad_perm)
__device__ inline uint32_t quad_max(uint32_t x) {
    x = max(x, dpp<0xb1>(x));
    return max(x, dpp<0x4e>(x));
}

// Writes row `row` (unless < 0) by the kind's rule and leaves in lo / hi what a reader of the slot gets back.  Lane j of the four holds
// elements 8 j .. 8 j + 7 (lo) and 32 + 8 j .. 32 + 8 j + 7 (hi): bf16 two 16-byte stores, fp8 two 8-byte stores and lane 0 the param dword
template <int KIND>
__device__ inline void store_row4(const PagedKV &kv, int64_t row, int j, v4u &lo, v4u &hi) {
    if constexpr (KIND == KV_BF16) {
        if (row >= 0) {
            v4u *dst = (v4u *)kv.data + row * (D / 8);
            dst[j] = lo;
            dst[4 + j] = hi;
        }
    } else {
        uint32_t amax = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) amax = max(max(amax, max(lo[m] & 0x7fffu, (lo[m] >> 16) & 0x7fffu)), max(hi[m] & 0x7fffu, (hi[m] >> 16) & 0x7fffu));
        amax = quad_max(amax);
        const int e = fp8_exponent(amax);
        const uint32_t top = fp8_top(e);
        const float scale = __uint_as_float((uint32_t)(127 + e) << 23);
        v2u code[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            v4u &x = half ? hi : lo;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                v2s r = fp8_codes<false>(v2s{0, 0}, fp8_clamp(x[2 * m], top), e);
                r = fp8_codes<true>(r, fp8_clamp(x[2 * m + 1], top), e);
                code[half][m] = __builtin_bit_cast(uint32_t, r);
                const v2u seen = fp8_seen(code[half][m], scale);
                x[2 * m] = seen.x;
                x[2 * m + 1] = seen.y;
            }
        }
        if (row >= 0) {
            v2u *dst = (v2u *)kv.data + row * (D / 8);
            dst[j] = code[0];
            dst[4 + j] = code[1];
            if (j == 0) ((uint32_t *)kv.param)[row] = fp8_param(e);
        }
    }
}

template <int KIND, bool ROT>
__global__ __launch_bounds__(64 * MAX_WAVES) void rope_kv_append_hd64_kernel(const Append64 a) {
    const int j = threadIdx.x & 3, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * TPW + ((threadIdx.x >> 2) & (TPW - 1));
    if (i >= a.T) return;                                     // whole row groups leave: the four lanes of a group stay together
    const PagedKV &kv = a.kv;
    const int64_t row0 = append_row(kv, a.append_indptr, (int)i, 0, 0);   // the K row of head 0; -1: nothing is written for this token
    v4u cl = {}, ch = {}, sl = {}, sh = {};
    if constexpr (ROT) {
        const v4u *cp = (const v4u *)(a.cos + i * a.cs_stride), *sp = (const v4u *)(a.sin + i * a.cs_stride);
        cl = cp[j]; ch = cp[4 + j]; sl = sp[j]; sh = sp[4 + j];
    }
    const int R = a.Hq + 2 * kv.Hkv;
    for (int r = wave; r < R; r += a.G) {
        const int which = r < a.Hq ? -1 : r < a.Hq + kv.Hkv ? 0 : 1;            // q, k, v
        const int h = which < 0 ? r : r - a.Hq - which * kv.Hkv;
        const uint16_t *base = which < 0 ? a.q : which == 0 ? a.k : a.v;
        const v4u *src = (const v4u *)(base + i * a.qkv_stride + (int64_t)h * D);
        v4u lo = src[j], hi = src[4 + j];                     // elements 8 j .. 8 j + 7 and their partners 32 + 8 j .. 32 + 8 j + 7
        if (ROT && which <= 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t xl = lo[e], xh = hi[e], nh = xh ^ 0x80008000u;      // rotate_half: -x[d + 32] below 32, x[d - 32] above
                lo[e] = rope_one(xl & 0xffffu, nh & 0xffffu, cl[e] & 0xffffu, sl[e] & 0xffffu) |
                        (rope_one(xl >> 16, nh >> 16, cl[e] >> 16, sl[e] >> 16) << 16);
                hi[e] = rope_one(xh & 0xffffu, xl & 0xffffu, ch[e] & 0xffffu, sh[e] & 0xffffu) |
                        (rope_one(xh >> 16, xl >> 16, ch[e] >> 16, sh[e] >> 16) << 16);
            }
        }
        uint16_t *out;
        if (which < 0) {
            out = a.q_out + (i * a.Hq + h) * D;
        } else {
            store_row4<KIND>(kv, row0 < 0 ? -1 : row_of(kv, row0, which, h), j, lo, hi);
            out = which ? a.v_out : a.k_out;
            if (!out) continue;
            out += (i * kv.Hkv + h) * D;
        }
        ((v4u *)out)[j] = lo;
        ((v4u *)out)[4 + j] = hi;
    }
}

template <int KIND>
hipError_t launch_append_kind(const Append64 &a, bool rot, hipStream_t stream) {
    const unsigned grid = (unsigned)(((int64_t)a.T + TPW - 1) / TPW);
    if (rot) rope_kv_append_hd64_kernel<KIND, true><<<grid, 64 * a.G, 0, stream>>>(a);
    else rope_kv_append_hd64_kernel<KIND, false><<<grid, 64 * a.G, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace

namespace mm {

void kv_decode_hd64_split(int B, int Hkv, int max_seq_len, int *nc, int *chunk) {
    // DESIGN 7b's rule, two workgroups per CU of the 256 on an MI355X; a chunk gives every wave whole tiles
    kv_chunks((long long)B * Hkv, 512, max_seq_len, TILE * WAVES, nc, chunk);
}

size_t kv_decode_hd64_workspace_bytes(int B, int Hq, int Hkv, int max_seq_len) {
    int nc, chunk;
    kv_decode_hd64_split(B, Hkv, max_seq_len, &nc, &chunk);
    return nc > 1 ? (size_t)B * Hq * nc * (D + 2) * sizeof(float) : 0;     // Decode64::ws
}

hipError_t launch_paged_decode_hd64(const PagedKV &kv, const void *q, int Hq, int max_seq_len, float sm_scale, void *ws, void *o,
                                    hipStream_t stream) {
    Decode64 a;
    a.kv = kv;
    a.q = (const uint16_t *)q;
    a.ws = (float *)ws;
    a.o = (uint16_t *)o;
    a.Hq = Hq;
    a.g = Hq / kv.Hkv;
    kv_decode_hd64_split(kv.B, kv.Hkv, max_seq_len, &a.nc, &a.chunk);
    a.scale_log2 = (sm_scale > 0.0f ? sm_scale : 0.125f) * 1.4426950408889634f;      // 1 / sqrt(64)
    const hipError_t e = kv.kind == KV_FP8 ? launch_decode_g<KV_FP8>(a, stream) : launch_decode_g<KV_BF16>(a, stream);
    if (e != hipSuccess || a.nc == 1) return e;
    paged_decode_hd64_merge_kernel<<<dim3((Hq + 1) / 2, kv.B), 64, 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t launch_rope_kv_append_hd64(const PagedKV &kv, const void *q, const void *k, const void *v, int64_t qkv_stride, int Hq,
                                      const void *cos, const void *sin, int64_t cs_stride, const int *append_indptr, int T, void *q_out,
                                      void *k_out, void *v_out, hipStream_t stream) {
    Append64 a{kv, (const uint16_t *)q, (const uint16_t *)k, (const uint16_t *)v, (const uint16_t *)cos, (const uint16_t *)sin,
               (uint16_t *)q_out, (uint16_t *)k_out, (uint16_t *)v_out, append_indptr, qkv_stride, cs_stride, T, q ? Hq : 0, 0};
    const int R = a.Hq + 2 * kv.Hkv;                          // four rows per row group, until 16 waves
    a.G = (R + 3) / 4 < MAX_WAVES ? (R + 3) / 4 : MAX_WAVES;
    return kv.kind == KV_FP8 ? launch_append_kind<KV_FP8>(a, cos != nullptr, stream) : launch_append_kind<KV_BF16>(a, cos != nullptr, stream);
}

}  // namespace mm
