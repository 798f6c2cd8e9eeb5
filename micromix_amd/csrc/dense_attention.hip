// Dense causal GQA attention over contiguous bf16 q, k, v (mm_dense_attention, include/micromix_attention.h, which states the function).
// No cache and no page table: K and V rows of a sequence lie stride apart, so every address is affine in the tile index.
//
// One workgroup (4 waves) per (128-token query tile of one sequence, query head); wave w owns rows 32 w .. 32 w + 31 of the tile as two
// blocks of 16, with q (B fragments, 32 VGPRs) and the fp32 O^T accumulators (64 VGPRs) in registers for the whole walk.  The kv tokens
// are walked 64 at a time, tiles above the diagonal are not visited, a wave skips the tiles above its own rows, and the compare runs
// only on the tiles that cross a wave's diagonal.
//   staging  K and V tiles go global -> LDS with the LDS-DMA (dma16: 64 lanes x 16 B per instruction, 8 per wave per tile), both AS
//            STORED ([token][128 dims], 256 B rows), double buffered (2 x 32 KB).  The DMA writes LDS in lane order, so the layout is
//            chosen by which 16-byte chunk of the row a lane FETCHES: position p of row r holds chunk p ^ (r & 15) of K and chunk
//            p ^ ((r & 7) << 1) of V, which makes the reads below free of bank conflicts without padding.  Rows past the last token the
//            tile's queries attend are fetched from that last token (finite, masked), so nothing outside the sequence is ever read.
//   pipeline per tile: wait_vmcnt<0> (this wave's part of tile t has landed), ONE barrier (everybody's has, and everybody is done with
//            tile t - 1), issue tile t + 1 into the other buffer, then the math of tile t.  No load depends on another load.
//   scores   S^T = K q^T on v_mfma_f32_16x16x32_bf16, A = K rows from LDS (one ds_read_b128 serves both row blocks), B = q: a lane
//            holds 16 scores of one query row per block, the row max crosses 4 lanes.  Online softmax in fp32, log2 domain.
//   p.V      O^T += V^T P^T, B = bf16(p) straight from the score registers, A = V read TRANSPOSED from the as-stored tile with
//            ds_read_b64_tr_b16: the 16 lanes of a group fetch 4 tokens x 16 dims and each receives its dim's 4 tokens (again one read
//            for both row blocks).
// GQA: blockIdx.x = tile * Hq + head with the head fastest, so the g workgroups that share a kv head's K/V tiles are dispatched next
// to each other and all but the first find them in L2.  The last tiles (the longest walks) come first.
// Sequence b owns tiles [seq_indptr[b] / 128 + b, seq_indptr[b + 1] / 128 + b + 1), which hold its ceil(n_b / 128) tiles, so the grid
// (T / 128 + B) * Hq needs no host copy of seq_indptr; the surplus workgroups exit.
// The sliding-window form (mm_dense_attention_window, include/micromix_attention_window.h) is the kernel's second instantiation: the same
// tiles, staging and pipeline over a walk that starts at the window's lower edge, stated at the template below.
// The rectangular split-KV form (mm_dense_attention_prefix, include/micromix_attention_prefix.h) is the third: new query tokens over K / V
// that also hold the tokens in front of them, the diagonal moved nk - nq to the right, blockIdx also carrying a chunk of the kv tokens,
// and a small merge launch behind it; stated at the template too.
#include "../../include/micromix_attention.h"
#include "../../include/micromix_attention_prefix.h"
#include "mx_buffer_ops.h"
#include "mx_kernels.h"
#include "mx_paged_kv.h"      // v8bf, v4u, v2u, pack_bf, HD

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

namespace {

using mm::DenseAttention;
using mm::DenseAttentionPrefix;
using mm::DenseAttentionWindow;
using mm::kv::HD;
using mm::kv::pack_bf;
using mm::kv::v2u;
using mm::kv::v4u;
using mm::kv::v8bf;
using mm::rsrc_t;
using mm::v4f;

constexpr int BQ = MM_DENSE_ATTN_BQ, BK = MM_DENSE_ATTN_BK, NT = 256;
constexpr int ROWB = HD * 2;                 // bytes of a K / V row in LDS
constexpr int TILEB = BK * ROWB;             // one K or V tile
constexpr int BUFB = 2 * TILEB;              // K | V of one kv tile
constexpr int LDS_BYTES = 2 * BUFB;          // double buffered
static_assert(BQ == 128 && BK == 64 && HD == 128 && LDS_BYTES == 65536, "the lane maps below are written for these tiles");

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

// WIN: the sliding-window form (mm_dense_attention_window, include/micromix_attention_window.h): row i attends tokens i - W + 1 .. i, so
// the walk starts at the tile that holds the lower edge of the query tile's first row, a wave also skips the tiles wholly below the
// window of its first row, and a second compare runs on the tiles that cross the lower edge of some row of the wave.  With WIN false
// t0 and W are constants and every added line folds away: the un-windowed kernel's instructions are what they were without them.
// PFX: the rectangular split-KV form (mm_dense_attention_prefix, include/micromix_attention_prefix.h): the sequence's n = nq query rows
// lie at q0 and its nk kv tokens at k0 of their own split, row i attends tokens 0 .. off + i with off = nk - nq (uniform, any sign), so
// off moves kend, the wave skip and the compare; blockIdx.x = (tile * nc + chunk) * Hq + head, and the workgroup walks the kv tiles of
// tokens [chunk * a.chunk, (chunk + 1) * a.chunk) below kend, leaving at once when there are none.  With nc > 1 the epilogue stores
// the accumulators as they lie, unnormalised, and (m, l) per row for dense_prefix_merge_kernel; with nc == 1 it is the other forms'.
// With PFX false off is 0, k0 is q0, nk is n and t1 is nt: the two instantiations above keep their instructions.
template <bool WIN, bool PFX = false>
__global__ __launch_bounds__(NT) void dense_attention_kernel(
    const std::conditional_t<PFX, DenseAttentionPrefix, std::conditional_t<WIN, DenseAttentionWindow, DenseAttention>> a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];   // [2][K tile | V tile], written by the LDS-DMA only

    const int x = blockIdx.x, h = x % a.Hq, kvh = h / a.g;
    int xt = x / a.Hq, ck = 0;                            // PFX: the head is fastest, then the chunk
    if constexpr (PFX) ck = xt % a.nc, xt /= a.nc;
    const int tile = a.tiles - 1 - xt;                    // the last tiles of a sequence carry the most work: they start first
    int b, j, q0, n;
    if (!tile_of(a, tile, b, j, q0, n)) return;
    int k0 = q0, nk = n, off = 0;                         // where the sequence's kv tokens lie, and how far right the diagonal sits
    if constexpr (PFX) {
        k0 = min(max(a.kv_indptr[b], 0), a.Tk);
        nk = max(min(max(a.kv_indptr[b + 1], 0), a.Tk) - k0, 0);
        off = nk - n;
    }
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63, c = l & 15, kq = l >> 4;
    const int i0 = j * BQ;                                // first token (of the sequence) of this query tile
    const int kend = min(nk, off + i0 + BQ);              // tokens 0 .. kend - 1 are attended by some row (PFX: none when kend <= 0)
    const int nt = PFX && kend <= 0 ? 0 : (kend + BK - 1) / BK;
    const int wr0 = i0 + 32 * wave;                       // this wave's first row; its last valid one
    const bool wactive = wr0 < n;
    const int wmax = min(wr0 + 31, n - 1);
    int W = 0, t0 = 0;                                    // the window (1 <= W < T, the launch sees to it) and the first kv tile of the walk
    if constexpr (WIN) W = a.W, t0 = max(i0 - W + 1, 0) / BK;
    int t1 = nt;                                          // the end of the walk
    if constexpr (PFX) {
        t0 = ck * (a.chunk / BK);
        t1 = min(nt, t0 + a.chunk / BK);
        if (t0 >= t1 && a.nc > 1) return;                 // nothing of this chunk lies below the tile's diagonal: the merge knows
    }

    // ---- q as the MFMA B operand: row block rb, lane (c, kq) holds row wr0 + 16 rb + c, dims 32 kq + 8 s + e in step s
    v8bf qb[2][4];
    int irow[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        irow[rb] = wr0 + 16 * rb + c;
        const bool valid = irow[rb] < n;
        const v4u *qp = (const v4u *)(a.q + (int64_t)(q0 + (valid ? irow[rb] : i0)) * a.sq + (int64_t)h * HD + 32 * kq);
#pragma unroll
        for (int s = 0; s < 4; ++s) qb[rb][s] = __builtin_bit_cast(v8bf, valid ? qp[s] : v4u{0, 0, 0, 0});
    }

    // ---- staging: DMA instruction i of wave w fills LDS rows 16 w + 4 i .. + 3 of a tile, lane (kq, c) position c of row 16 w + 4 i + kq
    const uint8_t *kseq = (const uint8_t *)(a.k + (int64_t)k0 * a.sk + (int64_t)kvh * HD);
    const uint8_t *vseq = (const uint8_t *)(a.v + (int64_t)k0 * a.sv + (int64_t)kvh * HD);
    const int skb = (int)a.sk * 2, svb = (int)a.sv * 2;   // bytes between two tokens (<= 2^23)
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(mm::lds_address(smem));
    auto issue = [&](int t) {
        const int kt = t * BK, nrows = min(kend - kt, BK);           // >= 1
        const rsrc_t rk = mm::make_rsrc(kseq + (int64_t)kt * skb, (unsigned)((nrows - 1) * skb + ROWB));
        const rsrc_t rv = mm::make_rsrc(vseq + (int64_t)kt * svb, (unsigned)((nrows - 1) * svb + ROWB));
        const unsigned base = lds0 + ((t - t0) & 1) * BUFB + wave * 4096;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rr = 16 * wave + 4 * i + kq, rc = min(rr, nrows - 1);
            mm::dma16(rk, rc * skb + ((c ^ (rr & 15)) << 4), 0, base + i * 1024);
            mm::dma16(rv, rc * svb + ((c ^ ((rr & 7) << 1)) << 4), 0, base + TILEB + i * 1024);
        }
    };

    // ---- LDS read offsets of this lane.  K: row 16 blk + c, chunk 4 kq + s.  V (transposed read): token 32 ks + 16 u + 4 kq + (c >> 2),
    // dims 16 dt + 4 (c & 3) .. + 3, that is chunk 2 dt + ((c >> 1) & 1), its half c & 1
    int koff[4], voff[2];
#pragma unroll
    for (int s = 0; s < 4; ++s) koff[s] = c * ROWB + (((4 * kq + s) ^ c) << 4);
    const int vtok = 4 * kq + (c >> 2), vsw = (vtok & 7) << 1, vx = (c >> 1) & 1, vhalf = (c & 1) << 3;
#pragma unroll
    for (int u = 0; u < 2; ++u) voff[u] = (16 * u + vtok) * ROWB + vhalf;

    float m[2] = {-INFINITY, -INFINITY}, lsum[2] = {0.0f, 0.0f};
    v4f o[2][8];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[rb][dt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};

    if constexpr (PFX) { if (t0 < t1) issue(t0); }         // nc == 1 and no token attended: no walk, the epilogue writes zeros
    else if constexpr (WIN) issue(t0); else issue(0);      // the literal: with issue(t0) the un-windowed prologue is scheduled differently
    for (int t = t0; t < t1; ++t) {
        mm::wait_vmcnt<0>();                               // this wave's share of tile t is in LDS
        __syncthreads();                                   // ... everybody's is, and nobody still reads tile t - 1
        if (t + 1 < t1) issue(t + 1);                      // in flight during this tile's math
        const int kt = t * BK, ko = kt - off;              // ko: the tile's first token seen from the diagonal, uniform
        if (!wactive || ko > wmax) continue;               // every row of this wave is masked on this tile
        if (WIN && kt + BK - 1 < wr0 - W + 1) continue;    // ... here too: the tile ends below the window of the wave's first row
        const uint8_t *sk = smem + ((t - t0) & 1) * BUFB, *sv = sk + TILEB;

        // ---- scores S^T: lane (c, kq) holds, for its row of each block, tokens kt + 16 blk + 4 kq + r
        float sc[2][4][4];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            v4f d0 = {0.0f, 0.0f, 0.0f, 0.0f}, d1 = d0;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const v8bf kf = __builtin_bit_cast(v8bf, *(const v4u *)(sk + blk * 16 * ROWB + koff[s]));
                d0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qb[0][s], d0, 0, 0, 0);
                d1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qb[1][s], d1, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[0][blk][r] = d0[r] * a.scale_log2;
                sc[1][blk][r] = d1[r] * a.scale_log2;
            }
        }
        if (ko + BK - 1 > wr0) {                           // the tile crosses the diagonal of some row of this wave
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (ko + 16 * blk + 4 * kq + r > irow[rb]) sc[rb][blk][r] = -INFINITY;
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
            const float mn = fmaxf(m[rb], mt), mb = mn == -INFINITY ? 0.0f : mn, alpha = __builtin_amdgcn_exp2f(m[rb] - mb);
            m[rb] = mn;
            float ps = 0.0f;
#pragma unroll
            for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sc[rb][blk][r] = __builtin_amdgcn_exp2f(sc[rb][blk][r] - mb);
                    ps += sc[rb][blk][r];
                }
            lsum[rb] = lsum[rb] * alpha + ps;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt)
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
            for (int dt = 0; dt < 8; ++dt) {
                const int chunk = (((2 * dt) ^ vsw) | vx) << 4;
                const v2u a0 = read_tr(sv + ks * 32 * ROWB + voff[0] + chunk), a1 = read_tr(sv + ks * 32 * ROWB + voff[1] + chunk);
                const v8bf va = __builtin_bit_cast(v8bf, v4u{a0.x, a0.y, a1.x, a1.y});
                o[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb[0][ks], o[0][dt], 0, 0, 0);
                o[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb[1][ks], o[1][dt], 0, 0, 0);
            }
        }
    }

    // ---- PFX, split: the partial rows as the accumulators hold them (lane (c, kq): row c of a block, dims 16 dt + 4 kq .. + 3, 16 bytes)
    // and (m, l) per row, at part index ((tile * Hq + h) * nc + chunk) * BQ + row, the layout kv::merge_chunks reads with stride BQ
    if constexpr (PFX) {
        if (a.nc > 1) {
            const int64_t part0 = (((int64_t)tile * a.Hq + h) * a.nc + ck) * BQ;
            float *ml = a.ws + (int64_t)a.tiles * a.Hq * a.nc * BQ * HD;
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                float ls = lsum[rb];
                ls += __shfl_xor(ls, 16);
                ls += __shfl_xor(ls, 32);
                if (irow[rb] >= n) continue;
                const int64_t part = part0 + (irow[rb] - i0);
                float *op = a.ws + part * HD + 4 * kq;
#pragma unroll
                for (int dt = 0; dt < 8; ++dt) *(v4f *)(op + 16 * dt) = o[rb][dt];
                if (kq == 0) *(float2 *)(ml + part * 2) = make_float2(m[rb], ls);
            }
            return;
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
        uint16_t *orow = a.o + ((int64_t)(q0 + irow[rb]) * a.Hq + h) * HD + 4 * kq;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
            v2u w;
            w.x = pack_bf(o[rb][dt][0] * inv, o[rb][dt][1] * inv);
            w.y = pack_bf(o[rb][dt][2] * inv, o[rb][dt][3] * inv);
            *(v2u *)(orow + 16 * dt) = w;
        }
    }
}

// combines the chunk partials of the rows of one (query tile, head): only the chunks that hold tokens below the tile's diagonal were
// written, the first ceil(nt / tiles per chunk) of them, by the same kend as the kernel's; none: the rows attend nothing and get zeros
__global__ __launch_bounds__(NT) void dense_prefix_merge_kernel(const DenseAttentionPrefix a) {
    const int x = blockIdx.x, h = x % a.Hq, tile = a.tiles - 1 - x / a.Hq;
    int b, j, q0, n;
    if (!tile_of(a, tile, b, j, q0, n)) return;
    const int k0 = min(max(a.kv_indptr[b], 0), a.Tk), nk = max(min(max(a.kv_indptr[b + 1], 0), a.Tk) - k0, 0);
    const int i0 = j * BQ, kend = min(nk, nk - n + i0 + BQ), nt = kend <= 0 ? 0 : (kend + BK - 1) / BK, cpt = a.chunk / BK;
    const int live = min(a.nc, (nt + cpt - 1) / cpt), rows = min(BQ, n - i0);
    const int64_t first = ((int64_t)tile * a.Hq + h) * a.nc * BQ;       // part index of chunk 0, row 0; chunk stride BQ
    const float *ml = a.ws + (int64_t)a.tiles * a.Hq * a.nc * BQ * HD;
    for (int idx = threadIdx.x; idx < rows * (HD / 4); idx += NT) {
        const int row = idx / (HD / 4), d = 4 * (idx % (HD / 4));
        float o[4];
        mm::kv::merge_chunks<4>(ml, a.ws + d, first + row, BQ, live, o);
        v2u w;
        w.x = pack_bf(o[0], o[1]);
        w.y = pack_bf(o[2], o[3]);
        *(v2u *)(a.o + ((int64_t)(q0 + i0 + row) * a.Hq + h) * HD + d) = w;
    }
}

}  // namespace

namespace mm {

hipError_t launch_dense_attention(DenseAttention a, float sm_scale, hipStream_t stream) {
    a.g = a.Hq / a.Hkv;
    a.tiles = a.T / BQ + a.B;
    a.scale_log2 = kv_scale_log2(sm_scale);
    dense_attention_kernel<false><<<(unsigned)((long long)a.tiles * a.Hq), NT, LDS_BYTES, stream>>>(a);
    return hipGetLastError();
}

// window >= 1.  A window that no row of T tokens can feel is the un-windowed kernel, which gives the same bits by construction; below
// that W < T, so no i - W + 1 of the kernel overflows.  The grid is the same, from host values alone.
hipError_t launch_dense_attention_window(DenseAttention a, float sm_scale, int window, hipStream_t stream) {
    if (window >= a.T) return launch_dense_attention(a, sm_scale, stream);
    DenseAttentionWindow w{};
    static_cast<DenseAttention &>(w) = a;
    w.g = a.Hq / a.Hkv;
    w.tiles = a.T / BQ + a.B;
    w.scale_log2 = kv_scale_log2(sm_scale);
    w.W = window;
    dense_attention_kernel<true><<<(unsigned)((long long)w.tiles * w.Hq), NT, LDS_BYTES, stream>>>(w);
    return hipGetLastError();
}

// nc chunks of `chunk` tokens from host values alone (kv_chunks, as the paged kernels get theirs): `tiles * Hq` workgroups per chunk
// against MM_DENSE_PREFIX_TARGET = 512, the workgroups of 64 KB LDS an MI355X holds at once (2 per CU, 256 CUs) -- a second round of
// them would wait for the first -- and kv_chunks' 256-token minimum, four kv tiles, below which the prologue and the partial rows
// outweigh the walk
void dense_prefix_split(int total_q, int B, int Hq, int max_kv_len, int *nc, int *chunk) {
    *nc = 1, *chunk = BK;
    if (total_q <= 0 || B <= 0 || Hq < 1 || max_kv_len <= 0) return;
    kv_chunks(((long long)total_q / BQ + B) * Hq, MM_DENSE_PREFIX_TARGET, max_kv_len, BK, nc, chunk);
}

size_t dense_prefix_workspace_bytes(int total_q, int B, int Hq, int max_kv_len) {
    int nc, chunk;
    dense_prefix_split(total_q, B, Hq, max_kv_len, &nc, &chunk);
    return nc > 1 ? (size_t)((long long)total_q / BQ + B) * Hq * nc * BQ * (HD + 2) * sizeof(float) : 0;    // DenseAttentionPrefix::ws
}

hipError_t launch_dense_attention_prefix(DenseAttention a, const int *kv_indptr, int total_kv, int max_kv_len, float sm_scale, void *ws,
                                         hipStream_t stream) {
    DenseAttentionPrefix p{};
    static_cast<DenseAttention &>(p) = a;
    p.g = a.Hq / a.Hkv;
    p.tiles = a.T / BQ + a.B;
    p.scale_log2 = kv_scale_log2(sm_scale);
    p.kv_indptr = kv_indptr;
    p.Tk = total_kv;
    p.ws = (float *)ws;
    dense_prefix_split(a.T, a.B, a.Hq, max_kv_len, &p.nc, &p.chunk);
    dense_attention_kernel<false, true><<<(unsigned)((long long)p.tiles * p.Hq * p.nc), NT, LDS_BYTES, stream>>>(p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.nc == 1) return e;
    dense_prefix_merge_kernel<<<(unsigned)((long long)p.tiles * p.Hq), NT, 0, stream>>>(p);
    return hipGetLastError();
}

}  // namespace mm
