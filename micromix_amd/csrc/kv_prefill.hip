// Causal multi-token attention over the paged int4 / bf16 / fp8 KV cache (include/micromix_hip.h, mm_paged_prefill).  Same cache layout,
// page table and head rules as mm_paged_decode (kv_cache.hip); the queries q [T, Hq, 128] are split among the sequences by qo_indptr
// (the append_indptr of mm_kv_append), and the mask is causal, aligned bottom-right: query j of sequence b sits at position
// p = len_b - n_b + j and attends cache positions 0..p.
//
// One workgroup (4 waves) per (query tile of one sequence, kv head, kv chunk).  Its 64 MFMA rows are (token, head) pairs over the g
// query heads of the kv head: BQ = 64 / g tokens x g heads (row r = token r / g, head r % g), 16 rows per wave, so each K/V byte is
// staged once per query tile.  Per 64-token kv tile:
//   staging  all 256 threads load the tile's K rows into LDS as stored, and V transposed ([dim][token], bf16: the int4 codes as exact
//            bf16 integers), plus per-token (scale, zero) of K and V; the next tile's global loads are issued before this tile's math
//   scores   S^T = K q^T, v_mfma_f32_16x16x32_bf16 with A = K (int4: 16 + code, exact), B = q (kept in registers), so a lane holds 16
//            scores of ONE query row; int4: s = sk (q.(16 + c)) - (16 sk + zk) sum(q)
//   softmax  online, fp32, log2 domain; the row max over the 4 lanes of a row; the causal mask only on tiles that cross the diagonal
//   p.V      O^T += V^T P^T on the MFMA: B = bf16(p * s_v) (int4) or bf16(p) (bf16 cache) straight from the score registers, A = the
//            transposed V image; int4 subtracts sum(p z_v) once at the end in fp32
//   fp8      staging widens the e4m3 codes of K and V to bf16 (exact), K into the bf16 kind's row layout and V into the same transposed
//            image, so scores and p.V read LDS exactly as the bf16 kind does; s = sk (q.code), B = bf16(p * s_v), no z: the power-of-two
//            scales move no rounding.  K is widened once per workgroup here, not once per wave at the MFMA operand as int4's nibbles are
// Split-KV: the kv range is cut into chunks chosen from host values only (kv_prefill_split); with more than one chunk each workgroup
// writes (m, l, o) partials and a merge launch combines them.  The tile -> (sequence, tile of it) map needs no host knowledge of
// qo_indptr: sequence b owns tiles [qo_indptr[b] / BQ + b, qo_indptr[b + 1] / BQ + b + 1), which hold its ceil(n_b / BQ) tiles;
// the surplus workgroups exit.
// Sliding window (mm_paged_prefill_window, the WINDOW kernels): a query at position p attends max(0, p - W + 1) .. p.  A query tile's
// walk starts at the kv tile that holds its first token's window start, its chunks are laid over the W + BQ + 62 tokens from there, a
// wave skips the tiles below all its rows' windows, and the lower-edge compare runs only on the tiles that cross one.  The un-windowed
// kernels are the WINDOW = false instantiations, instruction for instruction what they were.
// Tree mask (mm_paged_prefill_tree, the TREE kernels): among the n_b <= 64 tokens a sequence has just appended, query j attends new
// slot base_b + i (base_b = len_b - n_b) when i <= j and bit i of its word tree_mask[q0_b + j] is set, and every committed position
// below base_b.  A lane owns one query row, so it holds one word, with the bits above j cleared: the triangle is then a special case
// of the word, kend and the wave's skip stay what they are, and on the tiles that reach base_b the word's test stands where the
// diagonal's compare stood -- same elements set to -inf for a chain's words, so the same bits as the TREE = false kernel.  A sequence
// with n_b > 64 has no words and takes the diagonal (uniform over the workgroup).  TREE = false: the six kernels as they were.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

#include "mx_kernels.h"
#include "mx_paged_kv.h"

namespace {

using namespace mm::kv;       // the page-table walk, the int4 decoding and the chunk merge
using mm::PagedKV;

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int ROWS = 64;             // MFMA rows (token, head) per workgroup
constexpr int KT = 64;               // kv tokens per tile
constexpr int NT = 256;              // threads per workgroup
constexpr int KSTR4 = 64 + 16;       // LDS row stride of an int4 K row (bytes)
constexpr int KSTR16 = 256 + 16;     // LDS row stride of a bf16 K row (bytes)
constexpr int VSTR = 2 * KT + 8;     // LDS row stride of the transposed V image (bytes)

struct PrefillArgs {
    PagedKV kv;
    const uint16_t *q;
    const int *qo_indptr;
    float *ws;                 // partials: o [tiles, Hkv, nc, 64, 128], then (m, l) [tiles, Hkv, nc, 64, 2]
    uint16_t *o;
    int T, Hq, g, bq, tiles, nc, chunk;
    float scale_log2;          // sm_scale * log2(e)
    int window;                // WINDOW kernels: a query at position p attends positions max(0, p - window + 1) .. p
    const uint64_t *tree;      // TREE kernels: one word per query token, [T]
};

// (sequence, tile of it, its token count) of workgroup tile index i; false for a surplus tile
__device__ inline bool tile_of(const PrefillArgs &a, int i, int &b, int &j, int &q0, int &n) {
    int lo = 0, hi = a.kv.B;                         // the largest b with start(b) = qo_indptr[b] / bq + b <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (min(max(a.qo_indptr[mid], 0), a.T) / a.bq + mid <= i) lo = mid; else hi = mid;
    }
    b = lo;
    q0 = min(max(a.qo_indptr[b], 0), a.T);
    n = min(max(a.qo_indptr[b + 1], 0), a.T) - q0;
    j = i - (q0 / a.bq + b);
    return n > 0 && j * a.bq < n;
}

// WINDOW: a query tile walks the kv tiles from the window of its first token on (rounded down to KT), chunk c from there + c * chunk;
// a wave skips the tiles that lie below the windows of all its rows and compares against the lower edge only on the tiles that cross
// one of them -- both wave-uniform, like the diagonal's gate
template <int KIND, bool WINDOW, bool TREE = false>
__global__ __launch_bounds__(NT) void paged_prefill_kernel(const PrefillArgs a) {
    constexpr bool INT4 = KIND == KV_INT4, FP8 = KIND == KV_FP8;
    constexpr int KSTR = INT4 ? KSTR4 : KSTR16;       // fp8: the bf16 layout, widened at staging
    __shared__ __attribute__((aligned(16))) uint8_t s_k[KT * KSTR];
    __shared__ __attribute__((aligned(16))) uint8_t s_vt[HD * VSTR];
    __shared__ __attribute__((aligned(16))) float s_par[5][KT];      // per token: K scale, K offset, K bias (0 / -inf), V scale, V zero
    float *s_ks = s_par[0], *s_kc = s_par[1], *s_kb = s_par[2], *s_vs = s_par[3], *s_vz = s_par[4];

    const int tile = a.tiles - 1 - (int)blockIdx.x;      // the last tiles of a sequence carry the most work: they start first
    const int kvh = blockIdx.y, chunk = blockIdx.z;
    int b, j, q0, n;
    if (!tile_of(a, tile, b, j, q0, n)) return;
    const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, c = l & 15, kq = l >> 4;
    const PagedKV &kv = a.kv;
    const int g = a.g;
    const int len = seq_len(kv, b);
    const int *pages = kv.indices + kv.indptr[b];
    const int ntok = min(a.bq, n - j * a.bq);             // query tokens of this tile
    const int pos0 = len - n + j * a.bq;                   // position of its first token
    const int pmax = pos0 + ntok - 1;                      // the last position any row attends
    const int t0 = (WINDOW ? window_begin(max(pos0, -1), a.window) & ~(KT - 1) : 0) + chunk * a.chunk;
    const int t1 = chunk == a.nc - 1 ? len : min(len, t0 + a.chunk);   // the last chunk runs to the end, whatever max_seq_len said
    const int kend = min(t1, pmax + 1);

    // ---- this lane's query row: (token r / g, head r % g); q as the MFMA B operand, dims 32 kq + 8 s + e in step s
    const int row = 16 * wave + c, rt = row / g, rh = row - rt * g;
    const bool rvalid = rt < ntok;
    const int prow = rvalid ? pos0 + rt : -1;             // -1: attends nothing (also a query whose position is negative)
    const int64_t qrow = (int64_t)(q0 + j * a.bq + rt) * a.Hq + (int64_t)kvh * g + rh;
    v8bf qb[4];
    float sq = 0.0f;
    {
        const v4u *qp = (const v4u *)(a.q + (rvalid ? qrow : 0) * HD + 32 * kq);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const v4u w = rvalid ? qp[s] : v4u{0, 0, 0, 0};
            qb[s] = __builtin_bit_cast(v8bf, w);
#pragma unroll
            for (int e = 0; e < 4; ++e) sq += bf16f(w[e] & 0xffffu) + bf16f(w[e] >> 16);
        }
    }
    sq += __shfl_xor(sq, 16);
    sq += __shfl_xor(sq, 32);
    // rows of this wave: first / last position (wave-uniform)
    const int wr0 = 16 * wave, wt0 = wr0 / g, wt1 = min((wr0 + 15) / g, ntok - 1);
    const bool wactive = wt0 < ntok;
    const int wpmin = pos0 + wt0, wpmax = pos0 + wt1;
    // TREE: new slot i of the sequence is cache position base + i; this row is new token jt < 64 and keeps bits 0 .. jt of its word
    const bool tree = TREE && n <= 64;
    const int base = len - n, jt = j * a.bq + rt;
    uint64_t word = 0;
    if (TREE && tree && rvalid) word = a.tree[q0 + jt] & ((2ull << jt) - 1ull);

    float m = -INFINITY, lsum = 0.0f, pz = 0.0f;
    v4f o[8];
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[dt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};

    // ---- staging: thread (tg, dg) owns tokens 4 tg .. 4 tg + 3 of the tile: V dims 8 dg .. 8 dg + 7 of each, the K bytes of token
    // 4 tg + (dg >> 2) part dg & 3, and (dg == 0) the K params / (dg == 1) the V params of its four tokens
    const int tg = tid & 15, dg = tid >> 4, uk = dg >> 2, kpart = dg & 3;
    v4u kreg[INT4 ? 1 : FP8 ? 2 : 4];
    v4u vreg[4];                // int4: .x holds the token's 8 codes; fp8: .x, .y; bf16: the 8 values
    uint32_t preg[4];
    bool okreg[4];
    auto load = [&](int kt) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int64_t rk;
            const bool ok = okreg[u] = k_row(kv, pages, kt + 4 * tg + u, len, kvh, rk);
            const int64_t rv = rk + v_offset(kv);
            if (INT4) {
                vreg[u].x = ok ? *(const uint32_t *)(kv.data + rv * (HD / 2) + 4 * dg) : 0u;
                if (u == uk) kreg[0] = ok ? *(const v4u *)(kv.data + rk * (HD / 2) + 16 * kpart) : v4u{0, 0, 0, 0};
                if (dg < 2) preg[u] = ok ? *(const uint32_t *)(kv.param + (dg ? rv : rk) * 2) : 0u;
            } else if (FP8) {
                const v2u vc = ok ? *(const v2u *)(kv.data + rv * HD + 8 * dg) : v2u{0, 0};
                vreg[u].x = vc.x;
                vreg[u].y = vc.y;
                if (u == uk) {
                    kreg[0] = ok ? *(const v4u *)(kv.data + rk * HD + 32 * kpart) : v4u{0, 0, 0, 0};
                    kreg[1] = ok ? *(const v4u *)(kv.data + rk * HD + 32 * kpart + 16) : v4u{0, 0, 0, 0};
                }
                if (dg < 2) preg[u] = ok ? *(const uint32_t *)(kv.param + (dg ? rv : rk) * 2) : 0u;
            } else {
                vreg[u] = ok ? *(const v4u *)(kv.data + rv * (HD * 2) + 16 * dg) : v4u{0, 0, 0, 0};
                if (u == uk) {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        kreg[s] = ok ? *(const v4u *)(kv.data + rk * (HD * 2) + 64 * kpart + 16 * s) : v4u{0, 0, 0, 0};
                }
            }
        }
    };
    auto store = [&]() {
        if (INT4) {
            *(v4u *)(s_k + (4 * tg + uk) * KSTR + 16 * kpart) = kreg[0];
            float f[4][8];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t w = vreg[u].x, lo = w & 0x0f0f0f0fu, hi = (w >> 4) & 0x0f0f0f0fu;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    f[u][2 * e] = (float)((lo >> (8 * e)) & 0xffu);
                    f[u][2 * e + 1] = (float)((hi >> (8 * e)) & 0xffu);
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v2u w;
                w.x = __builtin_amdgcn_perm(__float_as_uint(f[1][e]), __float_as_uint(f[0][e]), 0x07060302u);   // exact: small integers
                w.y = __builtin_amdgcn_perm(__float_as_uint(f[3][e]), __float_as_uint(f[2][e]), 0x07060302u);
                *(v2u *)(s_vt + (8 * dg + e) * VSTR + 8 * tg) = w;
            }
            if (dg < 2) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float s = scale_of(preg[u]), z = zero_of(preg[u]);
                    const int t = 4 * tg + u;
                    if (dg == 0) {
                        s_ks[t] = okreg[u] ? s * a.scale_log2 : 0.0f;
                        s_kc[t] = okreg[u] ? (16.0f * s + z) * a.scale_log2 : 0.0f;
                        s_kb[t] = okreg[u] ? 0.0f : -INFINITY;
                    } else {
                        s_vs[t] = okreg[u] ? s : 0.0f;
                        s_vz[t] = okreg[u] ? z : 0.0f;
                    }
                }
            }
        } else if (FP8) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {      // 8 codes -> 8 bf16, the bf16 kind's row
                const v2u lo = fp8x4_to_bf16(kreg[s >> 1][2 * (s & 1)]), hi = fp8x4_to_bf16(kreg[s >> 1][2 * (s & 1) + 1]);
                *(v4u *)(s_k + (4 * tg + uk) * KSTR + 64 * kpart + 16 * s) = v4u{lo.x, lo.y, hi.x, hi.y};
            }
            v4u vb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const v2u lo = fp8x4_to_bf16(vreg[u].x), hi = fp8x4_to_bf16(vreg[u].y);
                vb[u] = v4u{lo.x, lo.y, hi.x, hi.y};
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int sh = 16 * (e & 1);
                v2u w;
                w.x = ((vb[0][e >> 1] >> sh) & 0xffffu) | (((vb[1][e >> 1] >> sh) & 0xffffu) << 16);
                w.y = ((vb[2][e >> 1] >> sh) & 0xffffu) | (((vb[3][e >> 1] >> sh) & 0xffffu) << 16);
                *(v2u *)(s_vt + (8 * dg + e) * VSTR + 8 * tg) = w;
            }
            if (dg < 2) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float s = scale_of(preg[u]);
                    const int t = 4 * tg + u;
                    if (dg == 0) {
                        s_ks[t] = okreg[u] ? s * a.scale_log2 : 0.0f;
                        s_kb[t] = okreg[u] ? 0.0f : -INFINITY;
                    } else {
                        s_vs[t] = okreg[u] ? s : 0.0f;
                    }
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) *(v4u *)(s_k + (4 * tg + uk) * KSTR + 64 * kpart + 16 * s) = kreg[s];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int sh = 16 * (e & 1);
                v2u w;
                w.x = ((vreg[0][e >> 1] >> sh) & 0xffffu) | (((vreg[1][e >> 1] >> sh) & 0xffffu) << 16);
                w.y = ((vreg[2][e >> 1] >> sh) & 0xffffu) | (((vreg[3][e >> 1] >> sh) & 0xffffu) << 16);
                *(v2u *)(s_vt + (8 * dg + e) * VSTR + 8 * tg) = w;
            }
            if (dg == 0) {
#pragma unroll
                for (int u = 0; u < 4; ++u) s_kb[4 * tg + u] = okreg[u] ? 0.0f : -INFINITY;
            }
        }
    };

    if (t0 < kend) load(t0);
    for (int kt = t0; kt < kend; kt += KT) {
        __syncthreads();                                   // the previous tile's LDS reads are done
        store();
        __syncthreads();
        if (kt + KT < kend) load(kt + KT);                 // in flight during this tile's math
        if (!wactive || kt > wpmax) continue;              // every row of this wave is masked on this tile
        if (WINDOW && wpmin - (kt + KT - 1) >= a.window) continue;   // ... it lies below the windows of all of them

        // ---- scores S^T: lane (c, kq) holds rows' scores of tokens kt + 16 blk + 4 kq + r for its row
        float sc[4][4];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            v4f d = {0.0f, 0.0f, 0.0f, 0.0f};
            const int tl = 16 * blk + 4 * kq;
            if (INT4) {
                const v4u kc = *(const v4u *)(s_k + (16 * blk + c) * KSTR + 16 * kq);
#pragma unroll
                for (int s = 0; s < 4; ++s) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(codes_to_bf16(kc[s]), qb[s], d, 0, 0, 0);
                const v4f ks = *(const v4f *)(s_ks + tl), kcs = *(const v4f *)(s_kc + tl), kb = *(const v4f *)(s_kb + tl);
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[blk][r] = ks[r] * d[r] - kcs[r] * sq + kb[r];
            } else if (FP8) {
                const v4u *kr = (const v4u *)(s_k + (16 * blk + c) * KSTR + 64 * kq);
#pragma unroll
                for (int s = 0; s < 4; ++s) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, kr[s]), qb[s], d, 0, 0, 0);
                const v4f ks = *(const v4f *)(s_ks + tl), kb = *(const v4f *)(s_kb + tl);
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[blk][r] = ks[r] * d[r] + kb[r];
            } else {
                const v4u *kr = (const v4u *)(s_k + (16 * blk + c) * KSTR + 64 * kq);
#pragma unroll
                for (int s = 0; s < 4; ++s) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, kr[s]), qb[s], d, 0, 0, 0);
                const v4f kb = *(const v4f *)(s_kb + tl);
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[blk][r] = d[r] * a.scale_log2 + kb[r];
            }
        }
        if (TREE && tree) {
            if (kt + KT - 1 >= base) {                     // the tile holds new slots: the word decides, the diagonal is in it
#pragma unroll
                for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = kt + 16 * blk + 4 * kq + r - base;      // committed (i < 0): kept; past the 64 slots: masked
                        if (i >= 0 && !(i < 64 && ((word >> (i & 63)) & 1ull))) sc[blk][r] = -INFINITY;
                    }
            }
        } else if (kt + KT - 1 > wpmin) {                  // the tile crosses the diagonal of some row of this wave
#pragma unroll
            for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kt + 16 * blk + 4 * kq + r > prow) sc[blk][r] = -INFINITY;
        }
        if (WINDOW && wpmax - kt >= a.window) {            // the tile crosses the lower edge of some row's window
#pragma unroll
            for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (prow - (kt + 16 * blk + 4 * kq + r) >= a.window) sc[blk][r] = -INFINITY;
        }
        // ---- online softmax (log2 domain)
        float mt = -INFINITY;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
#pragma unroll
            for (int r = 0; r < 4; ++r) mt = fmaxf(mt, sc[blk][r]);
        mt = fmaxf(mt, __shfl_xor(mt, 16));
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float mn = fmaxf(m, mt), mb = mn == -INFINITY ? 0.0f : mn, alpha = exp2f(m - mb);
        m = mn;
        float p[4][4], ps = 0.0f;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[blk][r] = exp2f(sc[blk][r] - mb);
                ps += p[blk][r];
            }
        lsum = lsum * alpha + ps;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[dt] *= alpha;
        // ---- p.V: k step ks covers tokens 32 ks + {4 kq + e, 16 + 4 kq + e}, e = 0..3
        if (INT4) pz *= alpha;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            v4u pb;
            if (INT4) {
                const v4f vs0 = *(const v4f *)(s_vs + 32 * ks + 4 * kq), vs1 = *(const v4f *)(s_vs + 32 * ks + 16 + 4 * kq);
                const v4f vz0 = *(const v4f *)(s_vz + 32 * ks + 4 * kq), vz1 = *(const v4f *)(s_vz + 32 * ks + 16 + 4 * kq);
#pragma unroll
                for (int r = 0; r < 4; ++r) pz += p[2 * ks][r] * vz0[r] + p[2 * ks + 1][r] * vz1[r];
                pb.x = pack_bf(p[2 * ks][0] * vs0[0], p[2 * ks][1] * vs0[1]);
                pb.y = pack_bf(p[2 * ks][2] * vs0[2], p[2 * ks][3] * vs0[3]);
                pb.z = pack_bf(p[2 * ks + 1][0] * vs1[0], p[2 * ks + 1][1] * vs1[1]);
                pb.w = pack_bf(p[2 * ks + 1][2] * vs1[2], p[2 * ks + 1][3] * vs1[3]);
            } else if (FP8) {
                const v4f vs0 = *(const v4f *)(s_vs + 32 * ks + 4 * kq), vs1 = *(const v4f *)(s_vs + 32 * ks + 16 + 4 * kq);
                pb.x = pack_bf(p[2 * ks][0] * vs0[0], p[2 * ks][1] * vs0[1]);
                pb.y = pack_bf(p[2 * ks][2] * vs0[2], p[2 * ks][3] * vs0[3]);
                pb.z = pack_bf(p[2 * ks + 1][0] * vs1[0], p[2 * ks + 1][1] * vs1[1]);
                pb.w = pack_bf(p[2 * ks + 1][2] * vs1[2], p[2 * ks + 1][3] * vs1[3]);
            } else {
                pb.x = pack_bf(p[2 * ks][0], p[2 * ks][1]);
                pb.y = pack_bf(p[2 * ks][2], p[2 * ks][3]);
                pb.z = pack_bf(p[2 * ks + 1][0], p[2 * ks + 1][1]);
                pb.w = pack_bf(p[2 * ks + 1][2], p[2 * ks + 1][3]);
            }
            const v8bf pbf = __builtin_bit_cast(v8bf, pb);
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                const uint8_t *vr = s_vt + (16 * dt + c) * VSTR + 2 * (32 * ks + 4 * kq);
                v4u va;
                const v2u a0 = *(const v2u *)vr, a1 = *(const v2u *)(vr + 32);
                va.x = a0.x; va.y = a0.y; va.z = a1.x; va.w = a1.y;
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, va), pbf, o[dt], 0, 0, 0);
            }
        }
    }

    // ---- row totals: l and sum(p z) over the 4 lanes of a row; o^T lane (c, kq) holds row c, dims 16 dt + 4 kq + r
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    if (INT4) {
        pz += __shfl_xor(pz, 16);
        pz += __shfl_xor(pz, 32);
    }
    if (!rvalid) return;
    if (a.nc == 1) {
        const float inv = lsum > 0.0f ? 1.0f / lsum : 0.0f;
        uint16_t *orow = a.o + qrow * HD + 4 * kq;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
            v2u w;
            w.x = pack_bf((o[dt][0] - pz) * inv, (o[dt][1] - pz) * inv);
            w.y = pack_bf((o[dt][2] - pz) * inv, (o[dt][3] - pz) * inv);
            *(v2u *)(orow + 16 * dt) = w;
        }
    } else {
        const int64_t part = (((int64_t)tile * kv.Hkv + kvh) * a.nc + chunk) * ROWS + row;
        float *op = a.ws + part * HD + 4 * kq;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) *(v4f *)(op + 16 * dt) = o[dt] - pz;
        if (kq == 0) *(float2 *)(a.ws + (int64_t)a.tiles * kv.Hkv * a.nc * ROWS * HD + part * 2) = make_float2(m, lsum);
    }
}

// combines the nc chunk partials of the rows of one (tile, kv head)
__global__ __launch_bounds__(NT) void paged_prefill_merge_kernel(const PrefillArgs a) {
    const int tile = blockIdx.x, kvh = blockIdx.y;
    int b, j, q0, n;
    if (!tile_of(a, tile, b, j, q0, n)) return;
    const int rows = min(a.bq, n - j * a.bq) * a.g;
    const int64_t first = ((int64_t)tile * a.kv.Hkv + kvh) * a.nc * ROWS;     // part index of chunk 0, row 0; chunk stride ROWS
    const float *ml = a.ws + (int64_t)a.tiles * a.kv.Hkv * a.nc * ROWS * HD;
    for (int idx = threadIdx.x; idx < rows * (HD / 4); idx += NT) {
        const int row = idx / (HD / 4), d = 4 * (idx % (HD / 4));
        float o[4];
        merge_chunks<4>(ml, a.ws + d, first + row, ROWS, a.nc, o);
        const int rt = row / a.g, rh = row - rt * a.g;
        const int64_t qrow = (int64_t)(q0 + j * a.bq + rt) * a.Hq + (int64_t)kvh * a.g + rh;
        v2u w;
        w.x = pack_bf(o[0], o[1]);
        w.y = pack_bf(o[2], o[3]);
        *(v2u *)(a.o + qrow * HD + d) = w;
    }
}

}  // namespace

namespace mm {

void kv_prefill_split(int T, int B, int Hq, int Hkv, int max_seq_len, int window, int *tiles, int *nc, int *chunk) {
    // tiles: an upper bound on sum ceil(n_b / BQ), BQ = 64 / g query tokens per tile.  Chunks: four workgroups per CU of the 256 on an MI355X
    const int g = Hkv > 0 && Hq >= Hkv ? Hq / Hkv : 1;
    const int bq = ROWS / (g > 0 && g <= ROWS ? g : 1);
    *tiles = T / bq + B;
    // a window: a query tile walks from the kv tile that holds the window's start of its first token (at most KT - 1 tokens below it)
    // to its last token's position, bq - 1 above the first's
    kv_chunks((long long)(*tiles > 0 ? *tiles : 1) * (Hkv > 0 ? Hkv : 1), 1024, kv_window_span(max_seq_len, window, bq - 1 + KT - 1), KT, nc,
              chunk);
}

size_t kv_prefill_workspace_bytes(int T, int B, int Hq, int Hkv, int max_seq_len, int window) {
    int tiles, nc, chunk;
    kv_prefill_split(T, B, Hq, Hkv, max_seq_len, window, &tiles, &nc, &chunk);
    return nc > 1 ? (size_t)tiles * Hkv * nc * ROWS * (HD + 2) * sizeof(float) : 0;
}

hipError_t launch_paged_prefill(const PagedKV &kv, const void *q, const int *qo_indptr, int T, int Hq, int max_seq_len, int window,
                                const void *tree_mask, float sm_scale, void *ws, void *o, hipStream_t stream) {
    PrefillArgs a;
    a.kv = kv;
    a.q = (const uint16_t *)q;
    a.qo_indptr = qo_indptr;
    a.ws = (float *)ws;
    a.o = (uint16_t *)o;
    a.T = T;
    a.Hq = Hq;
    a.g = Hq / kv.Hkv;
    a.bq = ROWS / a.g;
    kv_prefill_split(T, kv.B, Hq, kv.Hkv, max_seq_len, window, &a.tiles, &a.nc, &a.chunk);
    a.scale_log2 = kv_scale_log2(sm_scale);
    a.window = window;
    a.tree = (const uint64_t *)tree_mask;
    const dim3 grid(a.tiles, kv.Hkv, a.nc);
    if (tree_mask) {                                       // no window form (capi.hip passes window = 0)
        if (kv.kind == KV_INT4) paged_prefill_kernel<KV_INT4, false, true><<<grid, NT, 0, stream>>>(a);
        else if (kv.kind == KV_FP8) paged_prefill_kernel<KV_FP8, false, true><<<grid, NT, 0, stream>>>(a);
        else paged_prefill_kernel<KV_BF16, false, true><<<grid, NT, 0, stream>>>(a);
    } else if (window > 0) {
        if (kv.kind == KV_INT4) paged_prefill_kernel<KV_INT4, true><<<grid, NT, 0, stream>>>(a);
        else if (kv.kind == KV_FP8) paged_prefill_kernel<KV_FP8, true><<<grid, NT, 0, stream>>>(a);
        else paged_prefill_kernel<KV_BF16, true><<<grid, NT, 0, stream>>>(a);
    } else if (kv.kind == KV_INT4) paged_prefill_kernel<KV_INT4, false><<<grid, NT, 0, stream>>>(a);
    else if (kv.kind == KV_FP8) paged_prefill_kernel<KV_FP8, false><<<grid, NT, 0, stream>>>(a);
    else paged_prefill_kernel<KV_BF16, false><<<grid, NT, 0, stream>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.nc == 1) return e;
    paged_prefill_merge_kernel<<<dim3(a.tiles, kv.Hkv), NT, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace mm
