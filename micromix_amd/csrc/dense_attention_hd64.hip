// Dense causal GQA attention and RoPE for 64-wide heads (mm_dense_attention_hd64, mm_rope_qk_hd64; include/micromix_attention_hd64.h
// states the functions): the cache-less route rope_qk -> dense_attention(_window) for Llama-3.2-1B / Qwen2.5-0.5B shaped models.
// dense_attention.hip's structure is kept where it does not depend on the head dimension; what a 128-byte K / V row changes is
// decided here (DESIGN 7z gives the arguments and the measurements).
//
// Attention.  One workgroup (4 waves) per (128-token query tile of one sequence, query head); wave w owns rows 32 w .. 32 w + 31 as two
// blocks of 16, with q (B fragments, 16 VGPRs) and the fp32 O^T accumulators (32) in registers for the whole walk.  The kv tokens are
// walked BK = 64 at a time: a tile is 8 KB of K and 8 KB of V, double buffered in 32 KB of LDS, so that four workgroups share a CU where
// the 128 kernel has two -- per tile a wave has 32 MFMAs against 32 v_exp_f32 and the softmax bookkeeping around them, the vector unit and
// not the matrix pipe is the longer of the two, and it is other waves of the SIMD that fill the matrix pipe meanwhile.
//   staging  K and V tiles go global -> LDS with the LDS-DMA (dma16: 64 lanes x 16 B = 8 rows per instruction, 4 per wave per tile),
//            both AS STORED ([token][64 dims], 128 B rows).  Two rows share the 64 banks, so the bank group (16 B) of position p of row r
//            is 8 (r & 1) + p, and the layout is chosen by which chunk a lane FETCHES: position p of row r holds chunk
//            p ^ ((r >> 1) & 7) of K and chunk p ^ (((r >> 1) & 3) << 1) of V.
//              K   a ds_read_b128 is served 16 lanes (16 rows r0 + c, one logical chunk j) at a time: rows of one parity differ in
//                  (r >> 1) & 7, so j ^ ((r >> 1) & 7) takes 8 different positions in each half: 16 bank groups, each once.
//              V   a ds_read_b64_tr_b16 is served 32 lanes at a time: 8 tokens x 32 B, the chunk pair (2 dt, 2 dt + 1) of each.  The 4
//                  tokens of one parity differ in (r >> 1) & 3, so the pair index dt ^ ((r >> 1) & 3) takes 4 different values in each
//                  half: again 16 bank groups, each once.  The low bit of a chunk is left alone, so a pair stays a pair.
//            Rows past the last token the tile's queries attend are fetched from that last token (finite, masked).
//   pipeline per tile: wait_vmcnt<0>, ONE barrier, issue tile t + 1 into the other buffer, then the math of tile t.
//   scores   S^T = K q^T on v_mfma_f32_16x16x32_bf16, two k steps (lane (c, kq) holds dims 16 kq + 8 s + e in step s, chunk 2 kq + s).
//            The softmax scale is not multiplied into the scores: the row max is taken over the raw dot products (the scale is positive)
//            and p = exp2(fma(s, scale_log2, -m)) -- one v_fma where the 128 kernel has a v_mul and a v_sub per score.
//   p.V      O^T += V^T P^T, B = bf16(p) from the score registers, A = V read transposed with ds_read_b64_tr_b16, 4 dim blocks of 16.
// blockIdx.x = tile * Hq + head, the last tiles first, sequence b owning tiles [seq_indptr[b] / 128 + b, seq_indptr[b + 1] / 128 + b + 1),
// as in dense_attention.hip.  WIN is the sliding-window instantiation, as there.
//
// RoPE.  A workgroup owns TPW = 16 consecutive tokens and is G waves wide.  Four lanes own a 64-element head row: lane j of the four holds
// chunk j (elements 8 j .. 8 j + 7) and chunk j + 4 (32 + 8 j ..), so both partners of every pair are its own.  A wave is 16 row groups,
// one per token, all on the same row number; the Hq + Hkv rows of a token are dealt to the waves round robin and a group keeps its
// token's cos / sin chunks (8 registers) over its rows.  16-byte accesses only, no LDS.
#include "../../include/micromix_attention_hd64.h"
#include "mx_buffer_ops.h"
#include "mx_kernels.h"
#include "mx_paged_kv.h"      // v8bf, v4u, v2u, pack_bf
#include "mx_rope.h"          // rope_one

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

namespace {

using mm::DenseAttention;
using mm::DenseAttentionWindow;
using mm::kv::pack_bf;
using mm::kv::rope_one;
using mm::kv::v2u;
using mm::kv::v4u;
using mm::kv::v8bf;
using mm::rsrc_t;
using mm::v4f;

constexpr int D = 64, BQ = MM_DENSE_ATTN_HD64_BQ, BK = MM_DENSE_ATTN_HD64_BK, NT = 256;
constexpr int ROWB = D * 2;                  // bytes of a K / V row in LDS
constexpr int TILEB = BK * ROWB;             // one K or V tile
constexpr int BUFB = 2 * TILEB;              // K | V of one kv tile
constexpr int LDS_BYTES = 2 * BUFB;          // double buffered
static_assert(BQ == 128 && BK == 64 && LDS_BYTES == 32768, "the lane maps below are written for these tiles");

typedef __bf16 bf16x4 __attribute__((__vector_size__(8)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// (sequence, tile of it, first token, token count) of workgroup tile index i; false for a surplus tile
__device__ inline bool tile_of(const DenseAttention &a, int i, int &b, int &j, int &q0, int &n) {
    int lo = 0, hi = a.B;                            // the largest b with start(b) = seq_indptr[b] / BQ + b <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (min(max(a.indptr[mid], 0), a.T) / BQ + mid <= i) lo = mid; else hi = mid;
    }
    b = lo;
    q0 = min(max(a.indptr[lo], 0), a.T);
    n = min(max(a.indptr[lo + 1], 0), a.T) - q0;
    j = i - (q0 / BQ + lo);
    return n > 0 && j >= 0 && j * BQ < n;
}

// V^T fragment of 4 tokens: lane c of a 16-lane group passes the address of token (c >> 2), dims 4 (c & 3) .. + 3 of a 4 x 16 block and
// receives the block's 4 tokens of dim c
__device__ __forceinline__ v2u read_tr(const uint8_t *p) {
    v2u r = {0u, 0u};
    MM_DEVICE_ONLY(r = __builtin_bit_cast(v2u, __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4 *)p));)
    return r;
}

// WIN: row i attends tokens i - W + 1 .. i (1 <= W < T, the launch sees to it): the walk starts at the tile that holds the lower edge of
// the query tile's first row, a wave also skips the tiles wholly below the window of its first row, and the lower-edge compare runs only
// on the tiles that cross the lower edge of some row of the wave.  With WIN false t0 and W are constants and those lines fold away.
//
// The register budget is held to 128, four waves per SIMD and so four workgroups per CU (the compiler takes 122 + 40 unasked).
// MM_HD64_LDS_PAD: dynamic LDS requested on top of the 32 KB and never touched -- the ablation builds that hold a CU to three
// (-DMM_HD64_LDS_PAD=20480) or two (32768) workgroups with the same code, for the occupancy measurement of DESIGN 7z.
#ifndef MM_HD64_LDS_PAD
#define MM_HD64_LDS_PAD 0
#endif
template <bool WIN>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void dense_attention_hd64_kernel(
    const std::conditional_t<WIN, DenseAttentionWindow, DenseAttention> a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];   // [2][K tile | V tile], written by the LDS-DMA only

    const int x = blockIdx.x, h = x % a.Hq, kvh = h / a.g;
    const int tile = a.tiles - 1 - x / a.Hq;               // the last tiles of a sequence carry the most work: they start first
    int b, j, q0, n;
    if (!tile_of(a, tile, b, j, q0, n)) return;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63, c = l & 15, kq = l >> 4;
    const int i0 = j * BQ;                                 // first token (of the sequence) of this query tile
    const int kend = min(n, i0 + BQ);                      // tokens 0 .. kend - 1 are attended by some row
    const int nt = (kend + BK - 1) / BK;
    const int wr0 = i0 + 32 * wave;                        // this wave's first row; its last valid one
    const bool wactive = wr0 < n;
    const int wmax = min(wr0 + 31, n - 1);
    int W = 0, t0 = 0;
    if constexpr (WIN) W = a.W, t0 = max(i0 - W + 1, 0) / BK;

    // ---- q as the MFMA B operand: row block rb, lane (c, kq) holds row wr0 + 16 rb + c, dims 16 kq + 8 s + e in step s
    v8bf qb[2][2];
    int irow[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        irow[rb] = wr0 + 16 * rb + c;
        const bool valid = irow[rb] < n;
        const v4u *qp = (const v4u *)(a.q + (int64_t)(q0 + (valid ? irow[rb] : i0)) * a.sq + (int64_t)h * D + 16 * kq);
#pragma unroll
        for (int s = 0; s < 2; ++s) qb[rb][s] = __builtin_bit_cast(v8bf, valid ? qp[s] : v4u{0, 0, 0, 0});
    }

    // ---- staging: DMA instruction i of wave w fills LDS rows 16 w + 8 i .. + 7 of a tile, lane l position l & 7 of row 16 w + 8 i + (l >> 3)
    const uint8_t *kseq = (const uint8_t *)(a.k + (int64_t)q0 * a.sk + (int64_t)kvh * D);
    const uint8_t *vseq = (const uint8_t *)(a.v + (int64_t)q0 * a.sv + (int64_t)kvh * D);
    const int skb = (int)a.sk * 2, svb = (int)a.sv * 2;    // bytes between two tokens (<= 2^23)
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(mm::lds_address(smem));
    const int dp = l & 7, dr = l >> 3;
    auto issue = [&](int t) {
        const int kt = t * BK, nrows = min(kend - kt, BK);            // >= 1
        const rsrc_t rk = mm::make_rsrc(kseq + (int64_t)kt * skb, (unsigned)((nrows - 1) * skb + ROWB));
        const rsrc_t rv = mm::make_rsrc(vseq + (int64_t)kt * svb, (unsigned)((nrows - 1) * svb + ROWB));
        const unsigned base = lds0 + ((t - t0) & 1) * BUFB + wave * 2048;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int rr = 16 * wave + 8 * i + dr, rc = min(rr, nrows - 1);
            mm::dma16(rk, rc * skb + ((dp ^ ((rr >> 1) & 7)) << 4), 0, base + i * 1024);
            mm::dma16(rv, rc * svb + ((dp ^ (((rr >> 1) & 3) << 1)) << 4), 0, base + TILEB + i * 1024);
        }
    };

    // ---- LDS read offsets of this lane.  K: row 16 blk + c, chunk 2 kq + s.  V (transposed read): token 32 ks + 16 u + 4 kq + (c >> 2),
    // dims 16 dt + 4 (c & 3) .. + 3, that is chunk 2 dt + ((c >> 1) & 1), its half c & 1
    int koff[2], voff[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) koff[s] = c * ROWB + (((2 * kq + s) ^ ((c >> 1) & 7)) << 4);
    const int vtok = 4 * kq + (c >> 2), vsw = ((vtok >> 1) & 3) << 1, vx = (c >> 1) & 1, vhalf = (c & 1) << 3;
#pragma unroll
    for (int u = 0; u < 2; ++u) voff[u] = (16 * u + vtok) * ROWB + vhalf;

    float m[2] = {-INFINITY, -INFINITY}, lsum[2] = {0.0f, 0.0f};    // m: the running max of score * scale_log2
    v4f o[2][4];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[rb][dt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};

    issue(t0);
    for (int t = t0; t < nt; ++t) {
        mm::wait_vmcnt<0>();                               // this wave's share of tile t is in LDS
        __syncthreads();                                   // ... everybody's is, and nobody still reads tile t - 1
        if (t + 1 < nt) issue(t + 1);                      // in flight during this tile's math
        const int kt = t * BK;
        if (!wactive || kt > wmax) continue;               // every row of this wave is masked on this tile
        if (WIN && kt + BK - 1 < wr0 - W + 1) continue;    // ... here too: the tile ends below the window of the wave's first row
        const uint8_t *sk = smem + ((t - t0) & 1) * BUFB, *sv = sk + TILEB;

        // ---- raw scores S^T: lane (c, kq) holds, for its row of each block, tokens kt + 16 blk + 4 kq + r
        float sc[2][4][4];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            v4f d0 = {0.0f, 0.0f, 0.0f, 0.0f}, d1 = d0;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const v8bf kf = __builtin_bit_cast(v8bf, *(const v4u *)(sk + blk * 16 * ROWB + koff[s]));
                d0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qb[0][s], d0, 0, 0, 0);
                d1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qb[1][s], d1, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) sc[0][blk][r] = d0[r], sc[1][blk][r] = d1[r];
        }
        if (kt + BK - 1 > wr0) {                           // the tile crosses the diagonal of some row of this wave
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kt + 16 * blk + 4 * kq + r > irow[rb]) sc[rb][blk][r] = -INFINITY;
        }
        if (WIN && kt < wmax - W + 1) {                    // the tile crosses the lower edge of some row of this wave: token j of it is
            const int kw = kt - wr0 + W;                   // masked for row wr0 + x when j + W <= wr0 + x; kw is uniform and small
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kw + 16 * blk + 4 * kq + r <= 16 * rb + c) sc[rb][blk][r] = -INFINITY;
        }
        // ---- online softmax (log2 domain), P as the B operand of p.V: k step ks covers tokens 32 ks + {4 kq + e, 16 + 4 kq + e}
        v8bf pb[2][2];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            float mt = -INFINITY;
#pragma unroll
            for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                for (int r = 0; r < 4; ++r) mt = fmaxf(mt, sc[rb][blk][r]);
            mt = fmaxf(mt, __shfl_xor(mt, 16));
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float mn = fmaxf(m[rb], mt * a.scale_log2), mb = mn == -INFINITY ? 0.0f : mn, alpha = __builtin_amdgcn_exp2f(m[rb] - mb);
            m[rb] = mn;
            float ps = 0.0f;
#pragma unroll
            for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sc[rb][blk][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[rb][blk][r], a.scale_log2, -mb));
                    ps += sc[rb][blk][r];
                }
            lsum[rb] = lsum[rb] * alpha + ps;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[rb][dt][r] *= alpha;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                v4u w;
                w.x = pack_bf(sc[rb][2 * ks][0], sc[rb][2 * ks][1]);
                w.y = pack_bf(sc[rb][2 * ks][2], sc[rb][2 * ks][3]);
                w.z = pack_bf(sc[rb][2 * ks + 1][0], sc[rb][2 * ks + 1][1]);
                w.w = pack_bf(sc[rb][2 * ks + 1][2], sc[rb][2 * ks + 1][3]);
                pb[rb][ks] = __builtin_bit_cast(v8bf, w);
            }
        }
        // ---- p.V: O^T lane (c, kq) holds row c of each block, dims 16 dt + 4 kq + r
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int chunk = (((2 * dt) ^ vsw) | vx) << 4;
                const v2u a0 = read_tr(sv + ks * 32 * ROWB + voff[0] + chunk), a1 = read_tr(sv + ks * 32 * ROWB + voff[1] + chunk);
                const v8bf va = __builtin_bit_cast(v8bf, v4u{a0.x, a0.y, a1.x, a1.y});
                o[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb[0][ks], o[0][dt], 0, 0, 0);
                o[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb[1][ks], o[1][dt], 0, 0, 0);
            }
        }
    }

    // ---- row totals over the 4 lanes of a row, then o = O / l, rounded to bf16 once
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        float ls = lsum[rb];
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        if (irow[rb] >= n) continue;
        const float inv = ls > 0.0f ? 1.0f / ls : 0.0f;
        uint16_t *orow = a.o + ((int64_t)(q0 + irow[rb]) * a.Hq + h) * D + 4 * kq;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            v2u w;
            w.x = pack_bf(o[rb][dt][0] * inv, o[rb][dt][1] * inv);
            w.y = pack_bf(o[rb][dt][2] * inv, o[rb][dt][3] * inv);
            *(v2u *)(orow + 16 * dt) = w;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int TPW = MM_ROPE_HD64_TOKENS, MAX_WAVES = 16;
static_assert(TPW == 16, "a wave is one 4-lane row group per token of the workgroup");

struct RopeHd64 {
    const uint16_t *q, *k, *cos, *sin;
    uint16_t *q_out, *k_out;
    int64_t qkv_stride, cs_stride;     // elements per token
    int T, Hq, Hkv, G;
};

__global__ __launch_bounds__(64 * MAX_WAVES) void rope_qk_hd64_kernel(const RopeHd64 a) {
    const int j = threadIdx.x & 3, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * TPW + ((threadIdx.x >> 2) & (TPW - 1));
    if (i >= a.T) return;                                     // whole row groups leave: the four lanes of a group stay together
    const v4u *cp = (const v4u *)(a.cos + i * a.cs_stride), *sp = (const v4u *)(a.sin + i * a.cs_stride);
    const v4u cl = cp[j], ch = cp[4 + j], sl = sp[j], sh = sp[4 + j];
    for (int r = wave; r < a.Hq + a.Hkv; r += a.G) {
        const bool isq = r < a.Hq;
        const int h = isq ? r : r - a.Hq;
        const v4u *src = (const v4u *)((isq ? a.q : a.k) + i * a.qkv_stride + (int64_t)h * D);
        v4u lo = src[j], hi = src[4 + j];                     // elements 8 j .. 8 j + 7 and their partners 32 + 8 j .. 32 + 8 j + 7
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t xl = lo[e], xh = hi[e], nh = xh ^ 0x80008000u;      // rotate_half: -x[d + 32] below 32, x[d - 32] above
            lo[e] = rope_one(xl & 0xffffu, nh & 0xffffu, cl[e] & 0xffffu, sl[e] & 0xffffu) |
                    (rope_one(xl >> 16, nh >> 16, cl[e] >> 16, sl[e] >> 16) << 16);
            hi[e] = rope_one(xh & 0xffffu, xl & 0xffffu, ch[e] & 0xffffu, sh[e] & 0xffffu) |
                    (rope_one(xh >> 16, xl >> 16, ch[e] >> 16, sh[e] >> 16) << 16);
        }
        v4u *dst = (v4u *)(isq ? a.q_out + (i * a.Hq + h) * D : a.k_out + (i * a.Hkv + h) * D);
        dst[j] = lo;
        dst[4 + j] = hi;
    }
}

}  // namespace

namespace mm {

// window 0: none.  A window that no row of T tokens can feel is the un-windowed kernel, which gives the same bits by construction; below
// that W < T, so no i - W + 1 of the kernel overflows.  The grid is the same for both, from host values alone.
hipError_t launch_dense_attention_hd64(DenseAttention a, float sm_scale, int window, hipStream_t stream) {
    DenseAttentionWindow w{};
    static_cast<DenseAttention &>(w) = a;
    w.g = a.Hq / a.Hkv;
    w.tiles = a.T / BQ + a.B;
    w.scale_log2 = (sm_scale > 0.0f ? sm_scale : 0.125f) * 1.4426950408889634f;      // 1 / sqrt(64)
    w.W = window;
    const unsigned grid = (unsigned)((long long)w.tiles * w.Hq);
    if (window == 0 || window >= a.T) dense_attention_hd64_kernel<false><<<grid, NT, LDS_BYTES + MM_HD64_LDS_PAD, stream>>>(w);
    else dense_attention_hd64_kernel<true><<<grid, NT, LDS_BYTES + MM_HD64_LDS_PAD, stream>>>(w);
    return hipGetLastError();
}

hipError_t launch_rope_qk_hd64(const void *q, const void *k, int64_t qkv_stride, int Hq, int Hkv, const void *cos, const void *sin,
                               int64_t cs_stride, int T, void *q_out, void *k_out, hipStream_t stream) {
    RopeHd64 a{(const uint16_t *)q, (const uint16_t *)k, (const uint16_t *)cos, (const uint16_t *)sin, (uint16_t *)q_out, (uint16_t *)k_out,
               qkv_stride, cs_stride, T, Hq, Hkv, 0};
    const int R = Hq + Hkv;                                   // four rows per row group, until 16 waves
    a.G = (R + 3) / 4 < MAX_WAVES ? (R + 3) / 4 : MAX_WAVES;
    rope_qk_hd64_kernel<<<(unsigned)(((int64_t)T + TPW - 1) / TPW), 64 * a.G, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace mm
