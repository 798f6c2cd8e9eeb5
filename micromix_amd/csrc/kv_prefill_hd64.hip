// Causal multi-token attention over the paged KV cache for 64-wide heads (include/micromix_kv_prefill_hd64.h states the function;
// DESIGN 7ab gives the arguments and the measurements).  The cache, its page walk and the fp8 element rules are kv_hd64.hip's and
// mx_paged_kv.h's; the kernel is this file's own: it is not kv_prefill.hip with rows of 64.
//
// One workgroup (4 waves) per (query tile of one sequence, kv head, kv chunk).  Its ROWS MFMA rows are (token, head) pairs over the
// g = Hq / Hkv heads of the kv head (row r = token r / g, head r % g), so every K / V byte is staged once for all g heads.  ROWS = 128
// (32 rows, two blocks of 16, per wave: half of 7c's staging per FLOP) or, for calls that bring few tokens per sequence, 64 (one block
// per wave); the host picks from host values only (kv_prefill_hd64_plan).  Tile ownership is read from qo_indptr on the device, as in
// 7c: sequence b owns tiles [qo_indptr[b] / bq + b, ..), surplus tiles exit, the last tiles (the most work) start first.
//   staging  kv tiles of 64 tokens, K | V as stored ([token][64 dims], 128 B rows = one LDS bank span), double buffered, under 7z's
//            chunk swizzles: position p of row r holds chunk p ^ ((r >> 1) & 7) of K and p ^ (((r >> 1) & 3) << 1) of V, applied on
//            the SOURCE side -- a lane picks which 16-byte chunk of which token's row it fetches.
//            bf16: global -> LDS by LDS-DMA with per-lane 64-bit addresses (global_load_lds_dwordx4: the pages of a tile are scattered
//            and a cache may exceed the 4 GiB a buffer offset spans); 4 instructions per wave and tile, no register round trip.
//            fp8: the 16 codes and the fp16 scale of a lane's quarter row are loaded into registers before tile n's arithmetic and,
//            after it, widened by fp8_seen (decode(code) * 2^e, exact in bf16) into the SAME swizzled bf16 image, so the arithmetic
//            loop is one piece of code and bit equality with a bf16 cache of the dequantized values holds by construction.
//            A token past the rows' last position or on a page outside the cache fetches a 128-byte row of zeros (below: why not
//            row 0 of the cache) and carries -inf in a per-token bias kept beside the tile; every other token 0.
//   pipeline per tile: wait for the own DMA of tile n, ONE barrier, load the page-table entries of tile n + 2, issue tile n + 1 from
//            the entries loaded a tile earlier, then the arithmetic of tile n: no load waits on another load.
//   scores   S^T = K q^T on v_mfma_f32_16x16x32_bf16, A = K by ds_read_b128, B = q in registers for the whole walk
//   softmax  fp32, log2 domain, the scores scaled before the max is taken (the largest gives p = 1 exactly), lane-local state, the row
//            max across 4 lanes.  Each row
//            has its own diagonal: tiles wholly above the tile's last position are not visited, the compare runs only on tiles that
//            cross the diagonal of some row of the wave, and a wave whose rows are all masked on a tile skips its arithmetic
//   p.V      O^T += V^T P^T, A = V by ds_read_b64_tr_b16, B = bf16(p) straight from the score registers
//   split    chunks of whole tiles from host values; more than one: fp32 (o[64], m, l) partials per row and a small merge launch.  A
//            chunk past a tile's causal bound walks no tile and writes m = -inf, l = 0.
// The zero row: p = 0 does not remove a NaN from p.V on the matrix unit, and row 0 of a cache may hold anything (a free page), so
// masked tokens read zeros from this file's own 128 bytes instead -- the one place the kernel departs from "a valid address of the cache".
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/micromix_kv_prefill_hd64.h"
#include "mx_buffer_ops.h"
#include "mx_kv_hd64.h"
#include "mx_paged_kv.h"

namespace {

using namespace mm::kv;
using mm::PagedKV;
using mm::v4f;

constexpr int D = 64, KT = MM_KV_PREFILL_HD64_TILE, NT = 256;
constexpr int ROWB = D * 2;                  // bytes of a K / V row in LDS
constexpr int TILEB = KT * ROWB;             // one K or V tile
constexpr int BUFB = 2 * TILEB;              // K | V of one kv tile
constexpr int BIAS0 = 2 * BUFB;              // then the bias [2][KT] floats
constexpr int LDS_BYTES = BIAS0 + 2 * KT * 4;
static_assert(KT == 64 && BIAS0 == 32768, "the lane maps below are written for 64-token tiles");

typedef __bf16 bf16x4 __attribute__((__vector_size__(8)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__device__ __attribute__((aligned(128))) const uint32_t zero_row[ROWB / 4] = {};

struct Prefill64 {
    PagedKV kv;
    const uint16_t *q;
    const int *qo_indptr;
    float *ws;                 // partials: o [tiles, Hkv, nc, rows, 64], then (m, l) [tiles, Hkv, nc, rows, 2]
    uint16_t *o;
    int T, Hq, g, rows, bq, tiles, nc, chunk;
    int pshift;                // log2(page_size) when it is a power of two, else -1
    float scale_log2;          // sm_scale * log2(e)
};

// (sequence, tile of it, first query token, token count) of workgroup tile index i; false for a surplus tile
__device__ inline bool tile_of(const Prefill64 &a, int i, int &b, int &j, int &q0, int &n) {
    int lo = 0, hi = a.kv.B;                         // the largest b with start(b) = qo_indptr[b] / bq + b <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (min(max(a.qo_indptr[mid], 0), a.T) / a.bq + mid <= i) lo = mid; else hi = mid;
    }
    b = lo;
    q0 = min(max(a.qo_indptr[b], 0), a.T);
    n = min(max(a.qo_indptr[b + 1], 0), a.T) - q0;
    j = i - (q0 / a.bq + b);
    return n > 0 && j >= 0 && j * a.bq < n;
}

// one global_load_lds_dwordx4: 64 lanes x 16 B, lane l's 16 bytes at src (its own 64-bit address) -> LDS bytes [lds_addr + 16 l, + 16).
// M0 holds the wave-uniform LDS base; it belongs to the compiler, so it is saved and restored inside the statement (s_nop 0: one state
// between the M0 write and the LDS-DMA that reads it).  The compiler does not see the LDS writes: ordering is wait_vmcnt + barrier
__device__ __forceinline__ void dma16_global(const uint8_t *src, unsigned lds_addr) {
    MM_DEVICE_ONLY(unsigned keep;
                   asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                                "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                                : "=&s"(keep)
                                : "v"(src), "s"(lds_addr)
                                : "memory");)
}

// V^T fragment of 4 tokens: lane c of a 16-lane group passes the address of token (c >> 2), dims 4 (c & 3) .. + 3 of a 4 x 16 block and
// receives the block's 4 tokens of dim c
__device__ __forceinline__ v2u read_tr(const uint8_t *p) {
    v2u r = {0u, 0u};
    MM_DEVICE_ONLY(r = __builtin_bit_cast(v2u, __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4 *)p));)
    return r;
}

// x * y rounded to fp32 on its own: a product whose use the compiler sees (`x * y`, __fmul_rn) is contracted with a later subtraction into
// one fma, whose exponent then differs from the rounded product the row max was taken of.  The empty statement makes the product opaque;
// the multiply itself stays the compiler's to select and schedule
__device__ __forceinline__ float mul_rounded(float x, float y) {
    float r = x * y;
    MM_DEVICE_ONLY(asm("" : "+v"(r));)
    return r;
}

// The register budget is held to 128: the 32.5 KB of LDS let four workgroups share a CU, four waves a SIMD.  The fp8 kernel of 128 rows
// holds a tile's codes and params (10 registers) across the arithmetic on top of that and does not fit: it takes 168 and three
constexpr int waves_per_simd(int kind, int rows) { return kind == KV_FP8 && rows == 128 ? 3 : 4; }
template <int KIND, int ROWS>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(waves_per_simd(KIND, ROWS), waves_per_simd(KIND, ROWS))))
void paged_prefill_hd64_kernel(const Prefill64 a) {
    constexpr bool FP8 = KIND == KV_FP8;
    constexpr int RW = ROWS / 4, RB = RW / 16;       // rows and 16-row blocks of a wave
    constexpr int NTOK = FP8 ? 1 : 2;                // tokens of a tile whose row a lane fetches from
    static_assert(ROWS == 128 || ROWS == 64, "two or one row block per wave");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];   // [2][K tile | V tile], then the bias [2][KT]
    float *s_bias = (float *)(smem + BIAS0);

    const int tile = a.tiles - 1 - (int)blockIdx.x;  // the last tiles of a sequence carry the most work: they start first
    const int kvh = blockIdx.y, chunk = blockIdx.z;
    int b, j, q0, n;
    if (!tile_of(a, tile, b, j, q0, n)) return;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63, c = l & 15, kq = l >> 4;
    const PagedKV &kv = a.kv;
    const int g = a.g;
    const int len = seq_len(kv, b);
    const int *pages = kv.indices + kv.indptr[b];
    const int ntok = min(a.bq, n - j * a.bq);              // query tokens of this tile
    const int pos0 = len - n + j * a.bq;                   // position of its first token
    const int pmax = pos0 + ntok - 1;                      // the last position any row attends
    const int t0 = chunk * a.chunk;
    const int t1 = chunk == a.nc - 1 ? len : min(len, t0 + a.chunk);   // the last chunk runs to the end, whatever max_seq_len said
    const int kend = min(t1, pmax + 1);
    const int nt = kend > t0 ? (kend - t0 + KT - 1) / KT : 0;

    // ---- q as the MFMA B operand: row block rb, lane (c, kq) holds row RW wave + 16 rb + c, dims 16 kq + 8 s + e in step s
    v8bf qb[RB][2];
    int prow[RB];                                          // the row's position; -1: attends nothing
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int row = RW * wave + 16 * rb + c, rt = row / g, rh = row - rt * g;
        const bool valid = rt < ntok;
        prow[rb] = valid ? max(pos0 + rt, -1) : -1;
        const int64_t qrow = (int64_t)(q0 + j * a.bq + rt) * a.Hq + (int64_t)kvh * g + rh;
        const v4u *qp = (const v4u *)(a.q + (valid ? qrow : 0) * D + 16 * kq);
#pragma unroll
        for (int s = 0; s < 2; ++s) qb[rb][s] = __builtin_bit_cast(v8bf, valid ? qp[s] : v4u{0, 0, 0, 0});
    }
    // the wave's rows: first and last position (wave-uniform)
    const int wt0 = RW * wave / g, wt1 = min((RW * wave + RW - 1) / g, ntok - 1);
    const bool wactive = wt0 < ntok;
    const int wpmin = pos0 + wt0, wpmax = pos0 + wt1;

    // ---- staging.  bf16: DMA instruction i of wave w fills LDS rows 16 w + 8 i .. + 7 of a tile, lane l position l & 7 of row
    // 16 w + 8 i + (l >> 3).  fp8: thread t owns codes 16 (t & 3) .. + 15 of row t >> 2, the logical chunks 2 (t & 3) and 2 (t & 3) + 1
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(mm::lds_address(smem));
    const int dp = FP8 ? tid & 3 : l & 7;
    int tk[NTOK];
#pragma unroll
    for (int i = 0; i < NTOK; ++i) tk[i] = FP8 ? tid >> 2 : 16 * wave + 8 * i + (l >> 3);
    const int64_t voff = v_offset(kv);
    // the page-table entries of this lane's tokens of tile index ti; -1 past the attended tokens (no read)
    auto entries = [&](int ti, int (&pe)[NTOK]) {
#pragma unroll
        for (int i = 0; i < NTOK; ++i) {
            const int t = t0 + ti * KT + tk[i];
            pe[i] = t < kend ? pages[a.pshift >= 0 ? t >> a.pshift : t / kv.P] : -1;
        }
    };
    // the K row of token i of tile ti given its entry; false: the token is not attended
    auto krow_of = [&](int ti, int i, int pe, int64_t &row) {
        const int t = t0 + ti * KT + tk[i];
        const bool ok = pe >= 0 && pe < kv.max_pages;
        row = ok ? kv_row(kv, pe, 0, kvh, a.pshift >= 0 ? t & (kv.P - 1) : t % kv.P) : 0;
        return ok;
    };
    auto issue_dma = [&](int ti, const int (&pe)[NTOK]) {   // bf16: tile ti into buffer ti & 1
        const unsigned base = lds0 + (ti & 1) * BUFB + wave * 2048;
#pragma unroll
        for (int i = 0; i < NTOK; ++i) {
            int64_t row;
            const bool ok = krow_of(ti, i, pe[i], row);
            const int rr = tk[i];
            const uint8_t *ks = ok ? kv.data + row * ROWB : (const uint8_t *)zero_row;
            const uint8_t *vs = ok ? ks + voff * ROWB : (const uint8_t *)zero_row;
            dma16_global(ks + ((dp ^ ((rr >> 1) & 7)) << 4), base + i * 1024);
            dma16_global(vs + ((dp ^ (((rr >> 1) & 3) << 1)) << 4), base + TILEB + i * 1024);
            if (dp == 0) s_bias[(ti & 1) * KT + rr] = ok ? 0.0f : -INFINITY;
        }
    };
    v4u kc = {}, vc = {};                                   // fp8: the codes in flight, their rows' params, and whether the token is attended
    uint32_t pk = 0, pv = 0;
    bool okf = false;
    auto load_codes = [&](int ti, const int (&pe)[NTOK]) {
        int64_t row;
        okf = krow_of(ti, 0, pe[0], row);                   // row 0 is always there to address; what it holds is never used
        kc = ((const v4u *)(kv.data + row * D))[dp];
        vc = ((const v4u *)(kv.data + (row + voff) * D))[dp];
        pk = ((const uint32_t *)kv.param)[row];
        pv = ((const uint32_t *)kv.param)[row + voff];
    };
    auto widen = [&](int ti) {                              // fp8: the codes in flight -> the swizzled bf16 image of buffer ti & 1
        const int rr = tk[0];
        uint8_t *img = smem + (ti & 1) * BUFB + rr * ROWB;
        const float sk = scale_of(pk), sv = scale_of(pv);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ck = 2 * dp + h;
            const v2u k0 = fp8_seen(kc[2 * h], sk), k1 = fp8_seen(kc[2 * h + 1], sk);
            const v2u v0 = fp8_seen(vc[2 * h], sv), v1 = fp8_seen(vc[2 * h + 1], sv);
            *(v4u *)(img + ((ck ^ ((rr >> 1) & 7)) << 4)) = okf ? v4u{k0.x, k0.y, k1.x, k1.y} : v4u{0, 0, 0, 0};
            *(v4u *)(img + TILEB + ((ck ^ (((rr >> 1) & 3) << 1)) << 4)) = okf ? v4u{v0.x, v0.y, v1.x, v1.y} : v4u{0, 0, 0, 0};
        }
        if (dp == 0) s_bias[(ti & 1) * KT + rr] = okf ? 0.0f : -INFINITY;
    };

    // ---- LDS read offsets of this lane.  K: row 16 blk + c, chunk 2 kq + s.  V (transposed read): token 32 ks + 16 u + 4 kq + (c >> 2),
    // dims 16 dt + 4 (c & 3) .. + 3, that is chunk 2 dt + ((c >> 1) & 1), its half c & 1
    int koff[2], vofs[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) koff[s] = c * ROWB + (((2 * kq + s) ^ ((c >> 1) & 7)) << 4);
    const int vtok = 4 * kq + (c >> 2), vsw = ((vtok >> 1) & 3) << 1, vx = (c >> 1) & 1, vhalf = (c & 1) << 3;
#pragma unroll
    for (int u = 0; u < 2; ++u) vofs[u] = (16 * u + vtok) * ROWB + vhalf;

    float m[RB], lsum[RB];                                  // m: the running max of score * scale_log2
    v4f o[RB][4];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        m[rb] = -INFINITY;
        lsum[rb] = 0.0f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[rb][dt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    }

    int pe_near[NTOK], pe_far[NTOK];
    if (nt > 0) {
        entries(0, pe_far);
        entries(1, pe_near);
        if constexpr (FP8) {
            load_codes(0, pe_far);
            widen(0);
        } else {
            issue_dma(0, pe_far);
        }
    }
    for (int ti = 0; ti < nt; ++ti) {
        if constexpr (!FP8) mm::wait_vmcnt<0>();           // this wave's share of tile ti is in LDS
        __syncthreads();                                   // ... everybody's is, and nobody still reads tile ti - 1
        entries(ti + 2, pe_far);                           // first: what waits for it is the next tile's issue, a tile from now
        if (ti + 1 < nt) {
            if constexpr (FP8) load_codes(ti + 1, pe_near);
            else issue_dma(ti + 1, pe_near);
        }
        __builtin_amdgcn_sched_barrier(0);                 // the next tile's loads stay above this tile's arithmetic
        const int kt = t0 + ti * KT;
        if (wactive && kt <= wpmax) {                      // else: every row of this wave is masked on this tile
            const uint8_t *sk = smem + (ti & 1) * BUFB, *sv = sk + TILEB;
            // ---- raw scores S^T: lane (c, kq) holds, for its row of each block, tokens kt + 16 blk + 4 kq + r
            float sc[RB][4][4];
#pragma unroll
            for (int blk = 0; blk < 4; ++blk) {
                // the accumulators start from the tokens' bias (0, or -inf for a token that is not attended): the mask costs no instruction
                const v4f bz = *(const v4f *)(s_bias + (ti & 1) * KT + 16 * blk + 4 * kq);
                v4f d[RB];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) d[rb] = bz;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const v8bf kf = __builtin_bit_cast(v8bf, *(const v4u *)(sk + blk * 16 * ROWB + koff[s]));
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) d[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qb[rb][s], d[rb], 0, 0, 0);
                }
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[rb][blk][r] = d[rb][r];
            }
            if (kt + KT - 1 > wpmin) {                     // the tile crosses the diagonal of some row of this wave
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (kt + 16 * blk + 4 * kq + r > prow[rb]) sc[rb][blk][r] = -INFINITY;
            }
            // ---- online softmax (log2 domain), P as the B operand of p.V: k step ks covers tokens 32 ks + {4 kq + e, 16 + 4 kq + e}
            v8bf pb[RB][2];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                // The scores are scaled first and the max is taken of the scaled values (7c's order), so the row's largest score gives
                // p = exp2(0) = 1 exactly, whatever its size.  exp2(fma(score, scale, -max)) with max = fl(score * scale) leaves the
                // product's rounding error in the exponent of that token: at scores of 2^18 its p is up to 1 +- 0.011, bf16(p) then
                // differs from the p that went into l, and a row that attends one token returns V (1 +- 2^-8), not V
                float mt = -INFINITY;
#pragma unroll
                for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        sc[rb][blk][r] = mul_rounded(sc[rb][blk][r], a.scale_log2);    // scale_log2 > 0: -inf stays -inf
                        mt = fmaxf(mt, sc[rb][blk][r]);
                    }
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
                    const int ch = (((2 * dt) ^ vsw) | vx) << 4;
                    const v2u a0 = read_tr(sv + ks * 32 * ROWB + vofs[0] + ch), a1 = read_tr(sv + ks * 32 * ROWB + vofs[1] + ch);
                    const v8bf va = __builtin_bit_cast(v8bf, v4u{a0.x, a0.y, a1.x, a1.y});
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) o[rb][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb[rb][ks], o[rb][dt], 0, 0, 0);
                }
            }
        }
        if constexpr (FP8) {
            if (ti + 1 < nt) widen(ti + 1);                // into the buffer everybody left before this tile's barrier
        }
#pragma unroll
        for (int i = 0; i < NTOK; ++i) pe_near[i] = pe_far[i];
    }

    // ---- row totals over the 4 lanes of a row; one chunk: o = O / l, rounded to bf16 once; else the row's partial
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        float ls = lsum[rb];
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        if (a.nc == 1) {
            const int row = RW * wave + 16 * rb + c, rt = row / g, rh = row - rt * g;
            if (rt >= ntok) continue;
            const float inv = ls > 0.0f ? 1.0f / ls : 0.0f;
            uint16_t *orow = a.o + ((int64_t)(q0 + j * a.bq + rt) * a.Hq + (int64_t)kvh * g + rh) * D + 4 * kq;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                v2u w;
                w.x = pack_bf(o[rb][dt][0] * inv, o[rb][dt][1] * inv);
                w.y = pack_bf(o[rb][dt][2] * inv, o[rb][dt][3] * inv);
                *(v2u *)(orow + 16 * dt) = w;
            }
        } else {
            const int64_t part = (((int64_t)tile * kv.Hkv + kvh) * a.nc + chunk) * ROWS + RW * wave + 16 * rb + c;
            float *op = a.ws + part * D + 4 * kq;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) *(v4f *)(op + 16 * dt) = o[rb][dt];
            if (kq == 0) *(float2 *)(a.ws + (int64_t)a.tiles * kv.Hkv * a.nc * ROWS * D + part * 2) = make_float2(m[rb], ls);
        }
    }
}

// combines the nc chunk partials of the rows of one (tile, kv head): a thread per (row, 4 dims)
__global__ __launch_bounds__(NT) void paged_prefill_hd64_merge_kernel(const Prefill64 a) {
    const int tile = blockIdx.x, kvh = blockIdx.y;
    int b, j, q0, n;
    if (!tile_of(a, tile, b, j, q0, n)) return;
    const int rows = min(a.bq, n - j * a.bq) * a.g;
    const int64_t first = ((int64_t)tile * a.kv.Hkv + kvh) * a.nc * a.rows;      // part index of chunk 0, row 0; chunk stride a.rows
    const float *ml = a.ws + (int64_t)a.tiles * a.kv.Hkv * a.nc * a.rows * D;
    for (int idx = threadIdx.x; idx < rows * (D / 4); idx += NT) {
        const int row = idx / (D / 4), d = 4 * (idx % (D / 4));
        float M = -INFINITY;
        for (int c = 0; c < a.nc; ++c) M = fmaxf(M, ml[(first + (int64_t)c * a.rows + row) * 2]);
        float ls = 0.0f;
        v4f acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = 0; c < a.nc; ++c) {
            const int64_t p = first + (int64_t)c * a.rows + row;
            if (ml[p * 2] == -INFINITY) continue;          // a chunk without attended tokens
            const float f = exp2f(ml[p * 2] - M);
            ls += f * ml[p * 2 + 1];
            acc += f * *(const v4f *)(a.ws + p * D + d);
        }
        const float inv = ls > 0.0f ? 1.0f / ls : 0.0f;
        const int rt = row / a.g, rh = row - rt * a.g;
        const int64_t qrow = (int64_t)(q0 + j * a.bq + rt) * a.Hq + (int64_t)kvh * a.g + rh;
        v2u w;
        w.x = pack_bf(acc[0] * inv, acc[1] * inv);
        w.y = pack_bf(acc[2] * inv, acc[3] * inv);
        *(v2u *)(a.o + qrow * D + d) = w;
    }
}

template <int ROWS>
hipError_t launch_rows(const Prefill64 &a, hipStream_t stream) {
    const dim3 grid(a.tiles, a.kv.Hkv, a.nc);
    if (a.kv.kind == KV_FP8) paged_prefill_hd64_kernel<KV_FP8, ROWS><<<grid, NT, LDS_BYTES, stream>>>(a);
    else paged_prefill_hd64_kernel<KV_BF16, ROWS><<<grid, NT, LDS_BYTES, stream>>>(a);
    return hipGetLastError();
}

}  // namespace

namespace mm {

void kv_prefill_hd64_plan(int T, int B, int Hq, int Hkv, int max_seq_len, int *rows, int *bq, int *tiles, int *nc, int *chunk) {
    const int g = Hkv > 0 && Hq >= Hkv ? Hq / Hkv : 1;
    // few tokens per sequence (speculative widths): when a sequence's (token, head) rows fill at most half a 128-row tile on average,
    // the 64-row kernel leaves fewer MFMA rows empty.  -DMM_KV_PREFILL_HD64_FORCE_ROWS: tools/time_kv_prefill_hd64.py's ablation,
    // never the product build
#ifdef MM_KV_PREFILL_HD64_FORCE_ROWS
    *rows = MM_KV_PREFILL_HD64_FORCE_ROWS;
#else
    *rows = (long long)T * g <= 64LL * B ? MM_KV_PREFILL_HD64_ROWS_FEW : MM_KV_PREFILL_HD64_ROWS;
#endif
    *bq = *rows / (g <= 16 ? g : 16);
    *tiles = T / *bq + B;                                  // an upper bound on sum ceil(n_b / bq)
    // DESIGN 7c's rule: four workgroups per CU of the 256 on an MI355X, chunks of whole 64-token tiles
    kv_chunks((long long)(*tiles > 0 ? *tiles : 1) * (Hkv > 0 ? Hkv : 1), 1024, max_seq_len, KT, nc, chunk);
}

size_t kv_prefill_hd64_workspace_bytes(int T, int B, int Hq, int Hkv, int max_seq_len) {
    int rows, bq, tiles, nc, chunk;
    kv_prefill_hd64_plan(T, B, Hq, Hkv, max_seq_len, &rows, &bq, &tiles, &nc, &chunk);
    return nc > 1 ? (size_t)tiles * Hkv * nc * rows * (D + 2) * sizeof(float) : 0;     // Prefill64::ws
}

hipError_t launch_paged_prefill_hd64(const PagedKV &kv, const void *q, const int *qo_indptr, int T, int Hq, int max_seq_len,
                                     float sm_scale, void *ws, void *o, hipStream_t stream) {
    Prefill64 a;
    a.kv = kv;
    a.q = (const uint16_t *)q;
    a.qo_indptr = qo_indptr;
    a.ws = (float *)ws;
    a.o = (uint16_t *)o;
    a.T = T;
    a.Hq = Hq;
    a.g = Hq / kv.Hkv;
    kv_prefill_hd64_plan(T, kv.B, Hq, kv.Hkv, max_seq_len, &a.rows, &a.bq, &a.tiles, &a.nc, &a.chunk);
    a.pshift = -1;
    for (int s = 0; s < 31; ++s)
        if (kv.P == 1 << s) a.pshift = s;
    a.scale_log2 = (sm_scale > 0.0f ? sm_scale : 0.125f) * 1.4426950408889634f;      // 1 / sqrt(64)
    const hipError_t e = a.rows == 64 ? launch_rows<64>(a, stream) : launch_rows<128>(a, stream);
    if (e != hipSuccess || a.nc == 1) return e;
    paged_prefill_hd64_merge_kernel<<<dim3(a.tiles, kv.Hkv), NT, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace mm
