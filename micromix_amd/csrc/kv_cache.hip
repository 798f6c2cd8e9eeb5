// Paged KV cache: append (int4 or fp8 quantize, or bf16 copy) and GQA split-KV decode attention (include/micromix_hip.h, mm_kv_append /
// mm_paged_decode).  Layout and parameter convention of the reference's vendored FlashInfer cache (flashinfer/page.cuh:15,75-103,
// quantization.cuh:60-80); the quantization rule is quantize_int_group(x, 4, 128) (model/qLlamaLayer.py:13-23) with fp16 parameters.
//
//   kv_data  int4: uint8 [max_pages, L, 2, Hkv, P, 64]  (byte j = element 2j low nibble | element 2j+1 high nibble)
//            bf16: bf16  [max_pages, L, 2, Hkv, P, 128]
//            fp8:  uint8 [max_pages, L, 2, Hkv, P, 128] (OCP e4m3fn codes, element j in byte j)
//   kv_param int4 and fp8: fp16 [max_pages, L, 2, Hkv, P, 2] = (scale, zero);  value = decode(code) * scale - zero
//            (fp8: scale = 2^e, the smallest e in [-14, 15] with amax <= 448 * 2^e, and zero = +0.0)
//
// Decode: one workgroup (4 waves) per (sequence, kv head, chunk of tokens) handles all g = Hq / Hkv query heads of that kv head, so every
// cache byte is read once.  Each wave walks 32-token tiles of the chunk:
//   scores  one v_mfma_f32_16x16x32_bf16 chain per 16 tokens: A = q (16 head rows, g used), B = the K codes as bf16 (16 + code, exact),
//           so q.k = s * (q.(16 + c)) - (16 s + z) * sum(q);  for the bf16 cache B is the K row itself;  fp8: B = the codes widened to
//           bf16 (exact, one v_cvt_scalef32_pk_bf16_fp8 per two), q.k = s * (q.code): the power-of-two s moves no rounding
//   softmax online, in the log2 domain, the max across the tile's 16 token lanes, l and sum(p z) as per-lane partials
//   p.V     VALU, fp32: a lane owns 8 dims of 8 tokens of the tile, acc[h][8] += (p s_v)[h] * code  (minus sum(p z_v) once at the end;
//           fp8: the codes by v_cvt_pk_f32_fp8, no z)
// The waves merge through LDS; with one chunk the workgroup writes o, otherwise (m, l, o) partials that mm_paged_decode's merge kernel
// combines.
// Sliding window (mm_paged_decode_window, the WINDOW kernels): the walk starts at token max(0, len - W) instead of at token 0 and the
// chunks are laid over the W tokens from there, so a long sequence costs its window; the un-windowed kernels are the WINDOW = false
// instantiations, instruction for instruction what they were.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

#include "mx_kernels.h"
#include "mx_paged_kv.h"

namespace {

using namespace mm::kv;       // the page-table walk, the append rule, the int4 decoding and the chunk merge
using mm::PagedKV;

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int DEC_WAVES = 4;
constexpr int TILE = 32;           // tokens per wave iteration

// One workgroup per appended token and kv head; wave 0 writes K, wave 1 writes V (the slot and the int4 rule: mx_paged_kv.h).
template <int KIND>
__global__ __launch_bounds__(128) void kv_append_kernel(const PagedKV kv, const uint16_t *__restrict__ k, const uint16_t *__restrict__ v,
                                                        const int *__restrict__ append_indptr) {
    const int i = blockIdx.x, h = blockIdx.y, which = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = append_row(kv, append_indptr, i, which, h);
    if (row < 0) return;
    const uint32_t two = ((const uint32_t *)((which ? v : k) + ((int64_t)i * kv.Hkv + h) * HD))[lane];   // elements 2 lane, 2 lane + 1
    store_row<KIND>(kv, row, lane, two);
}

struct DecodeArgs {
    PagedKV kv;
    const uint16_t *q;
    float *ws;                 // partials: o [B, Hkv, nc, g, 128], then (m, l) [B, Hkv, nc, g, 2]
    uint16_t *o;
    int Hq, g, nc, chunk;
    float scale_log2;          // sm_scale * log2(e)
    int window;                // WINDOW kernels: the query attends its last `window` >= 1 tokens (itself included)
};

// WINDOW: the workgroups of sequence b walk [lo_b, len_b), lo_b = max(0, len_b - window), chunk c from lo_b + c * chunk on.  The tiles
// start at lo_b itself -- a lane addresses its token's row on its own, so a tile need not start on a multiple of 32 -- and no token
// below the window is ever looked at: no compare, no page-table read, the span exactly min(len_b, window) tokens
template <int KIND, int GP, bool WINDOW>
__global__ __launch_bounds__(256) void paged_decode_kernel(const DecodeArgs a) {
    __shared__ float s_p[DEC_WAVES][TILE][16];        // (p * scale) of the tile, [token][head]
    __shared__ float s_alpha[DEC_WAVES][16];
    __shared__ int64_t s_row[DEC_WAVES][TILE];        // V row of each token of the tile (-1: past the chunk)
    __shared__ float s_o[DEC_WAVES][GP][HD];
    __shared__ float s_ml[DEC_WAVES][GP][2];

    const int chunk = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, kq = l >> 4;
    const PagedKV &kv = a.kv;
    const int g = a.g;
    const int len = seq_len(kv, b);
    const int t0 = (WINDOW ? window_begin(len - 1, a.window) : 0) + chunk * a.chunk;
    const int t1 = chunk == a.nc - 1 ? len : min(len, t0 + a.chunk);   // the last chunk runs to the end, whatever max_seq_len said
    const int *pages = kv.indices + kv.indptr[b];

    // q as the MFMA A operand: lane (c, kq) holds head c, dims 32 kq + 8 s + j in step s
    v8bf qa[4];
    float qsum = 0.0f;
    {
        const v4u *qrow = (const v4u *)(a.q + ((int64_t)b * a.Hq + (int64_t)kvh * g + c) * HD + 32 * kq);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            v4u w = c < g ? qrow[s] : v4u{0, 0, 0, 0};
            qa[s] = __builtin_bit_cast(v8bf, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) qsum += bf16f(w[j] & 0xffffu) + bf16f(w[j] >> 16);
        }
    }
    qsum += __shfl_xor(qsum, 16);
    qsum += __shfl_xor(qsum, 32);
    float sq[4];                                       // sum(q) of the heads this lane's scores belong to (4 kq + r)
#pragma unroll
    for (int r = 0; r < 4; ++r) sq[r] = __shfl(qsum, 4 * kq + r);

    float m[4], lsum[4], pz[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; lsum[r] = 0.0f; pz[r] = 0.0f; }
    float acc[GP][8];
#pragma unroll
    for (int h = 0; h < GP; ++h)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[h][e] = 0.0f;

    const int dg = l & 15, tq = l >> 4;                // p.V layout: dims 8 dg .. 8 dg + 7 of tokens 4 i + tq
    for (int tb = t0 + TILE * wave; tb < t1; tb += TILE * DEC_WAVES) {
        // ---- scores of tokens tb + 16 G + c for heads 4 kq + r
        float sc[2][4], sv[2], zv[2];                  // sv, zv: the V row's (scale, zero) of the token
#pragma unroll
        for (int G = 0; G < 2; ++G) {
            int64_t rk;
            const bool ok = k_row(kv, pages, tb + 16 * G + c, t1, kvh, rk);
            if (kq == 0) s_row[wave][16 * G + c] = ok ? rk + v_offset(kv) : -1;
            v4f d = {0.0f, 0.0f, 0.0f, 0.0f};
            if (KIND == KV_INT4) {
                v4u kc = *(const v4u *)(kv.data + rk * (HD / 2) + 16 * kq);
                const uint32_t pk = *(const uint32_t *)(kv.param + rk * 2);
                const uint32_t pv = *(const uint32_t *)(kv.param + (rk + v_offset(kv)) * 2);
                if (!ok) kc = v4u{0, 0, 0, 0};
                // the conversions stay inside the selects: which of the products below the compiler fuses follows this shape
                const float sk = ok ? scale_of(pk) : 0.0f, zk = ok ? zero_of(pk) : 0.0f;
                sv[G] = ok ? scale_of(pv) : 0.0f;
                zv[G] = ok ? zero_of(pv) : 0.0f;
#pragma unroll
                for (int s = 0; s < 4; ++s) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[s], codes_to_bf16(kc[s]), d, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[G][r] = sk * d[r] - (16.0f * sk + zk) * sq[r];
            } else if (KIND == KV_FP8) {
                const v4u *kr = (const v4u *)(kv.data + rk * HD + 32 * kq);      // dims 32 kq .. 32 kq + 31: step s is dwords 2 s, 2 s + 1
                v4u kc[2];
                kc[0] = ok ? kr[0] : v4u{0, 0, 0, 0};
                kc[1] = ok ? kr[1] : v4u{0, 0, 0, 0};
                const uint32_t pk = *(const uint32_t *)(kv.param + rk * 2);
                const uint32_t pv = *(const uint32_t *)(kv.param + (rk + v_offset(kv)) * 2);
                const float sk = ok ? scale_of(pk) : 0.0f;
                sv[G] = ok ? scale_of(pv) : 0.0f;
                zv[G] = 0.0f;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const v2u lo = fp8x4_to_bf16(kc[s >> 1][2 * (s & 1)]), hi = fp8x4_to_bf16(kc[s >> 1][2 * (s & 1) + 1]);
                    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[s], __builtin_bit_cast(v8bf, (v4u{lo.x, lo.y, hi.x, hi.y})), d, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[G][r] = sk * d[r];
            } else {
                const v4u *kr = (const v4u *)(kv.data + rk * (HD * 2) + 64 * kq);
                v4u kb[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) kb[s] = ok ? kr[s] : v4u{0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < 4; ++s) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[s], __builtin_bit_cast(v8bf, kb[s]), d, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[G][r] = d[r];
                sv[G] = 1.0f;
                zv[G] = 0.0f;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) sc[G][r] = ok ? sc[G][r] * a.scale_log2 : -INFINITY;
        }
        // ---- online softmax (log2 domain); the tile always holds a valid token, so the new max is finite
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mt = fmaxf(sc[0][r], sc[1][r]);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) mt = fmaxf(mt, __shfl_xor(mt, o));
            const float mn = fmaxf(m[r], mt), alpha = exp2f(m[r] - mn);
            const float p0 = exp2f(sc[0][r] - mn), p1 = exp2f(sc[1][r] - mn);
            m[r] = mn;
            lsum[r] = lsum[r] * alpha + p0 + p1;
            pz[r] = pz[r] * alpha + p0 * zv[0] + p1 * zv[1];
            s_p[wave][c][4 * kq + r] = p0 * sv[0];
            s_p[wave][16 + c][4 * kq + r] = p1 * sv[1];
            if (c == 0) s_alpha[wave][4 * kq + r] = alpha;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's own LDS exchange (LDS operations of a wave run in order)
        // ---- p.V
#pragma unroll
        for (int h = 0; h < GP; ++h) {
            const float al = s_alpha[wave][h];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[h][e] *= al;
        }
        int64_t rv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) rv[i] = s_row[wave][4 * i + tq];
        if (KIND == KV_INT4) {
            uint32_t vc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) vc[i] = *(const uint32_t *)(kv.data + (rv[i] < 0 ? 0 : rv[i]) * (HD / 2) + 4 * dg);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (rv[i] < 0) continue;
                float cv[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    cv[2 * j] = (float)((vc[i] >> (8 * j)) & 15u);
                    cv[2 * j + 1] = (float)((vc[i] >> (8 * j + 4)) & 15u);
                }
#pragma unroll
                for (int h = 0; h < GP; ++h) {
                    const float p = s_p[wave][4 * i + tq][h];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[h][e] = fmaf(p, cv[e], acc[h][e]);
                }
            }
        } else if (KIND == KV_FP8) {
            v2u vc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) vc[i] = *(const v2u *)(kv.data + (rv[i] < 0 ? 0 : rv[i]) * HD + 8 * dg);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (rv[i] < 0) continue;
                float cv[8];
                fp8x4_to_f32(vc[i].x, cv);
                fp8x4_to_f32(vc[i].y, cv + 4);
#pragma unroll
                for (int h = 0; h < GP; ++h) {
                    const float p = s_p[wave][4 * i + tq][h];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[h][e] = fmaf(p, cv[e], acc[h][e]);
                }
            }
        } else {
            v4u vb[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) vb[i] = *(const v4u *)(kv.data + (rv[i] < 0 ? 0 : rv[i]) * (HD * 2) + 16 * dg);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (rv[i] < 0) continue;
                float vv[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    vv[2 * j] = bf16f(vb[i][j] & 0xffffu);
                    vv[2 * j + 1] = bf16f(vb[i][j] >> 16);
                }
#pragma unroll
                for (int h = 0; h < GP; ++h) {
                    const float p = s_p[wave][4 * i + tq][h];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[h][e] = fmaf(p, vv[e], acc[h][e]);
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads of this tile's exchange done before the next tile writes it
    }

    // ---- wave totals: acc over the four token lanes tq, l and sum(p z) over the 16 token lanes c
#pragma unroll
    for (int h = 0; h < GP; ++h)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            acc[h][e] += __shfl_xor(acc[h][e], 16);
            acc[h][e] += __shfl_xor(acc[h][e], 32);
        }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            lsum[r] += __shfl_xor(lsum[r], o);
            pz[r] += __shfl_xor(pz[r], o);
        }
    if (c == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * kq + r < GP) {
                s_ml[wave][4 * kq + r][0] = m[r];
                s_ml[wave][4 * kq + r][1] = lsum[r];
                s_alpha[wave][4 * kq + r] = pz[r];
            }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (tq == 0) {
#pragma unroll
        for (int h = 0; h < GP; ++h) {
            const float zsum = s_alpha[wave][h];
#pragma unroll
            for (int e = 0; e < 8; ++e) s_o[wave][h][8 * dg + e] = acc[h][e] - zsum;
        }
    }
    __syncthreads();

    // ---- merge the four waves: thread -> (head, 128 / 2 dims pair)
    const bool single = a.nc == 1;
    for (int idx = threadIdx.x; idx < g * (HD / 2); idx += 256) {
        const int h = idx / (HD / 2), d = 2 * (idx % (HD / 2));
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < DEC_WAVES; ++w) M = fmaxf(M, s_ml[w][h][0]);
        float ls = 0.0f, o0 = 0.0f, o1 = 0.0f;
        if (M != -INFINITY) {
#pragma unroll
            for (int w = 0; w < DEC_WAVES; ++w) {
                const float f = exp2f(s_ml[w][h][0] - M);      // 0 for a wave without tokens
                ls += f * s_ml[w][h][1];
                o0 += f * s_o[w][h][d];
                o1 += f * s_o[w][h][d + 1];
            }
        }
        const int hq = kvh * g + h;
        if (single) {
            const float inv = ls > 0.0f ? 1.0f / ls : 0.0f;
            *(uint32_t *)(a.o + ((int64_t)b * a.Hq + hq) * HD + d) = pack_bf(o0 * inv, o1 * inv);
        } else {
            const int64_t part = (((int64_t)b * kv.Hkv + kvh) * a.nc + chunk) * g + h;
            *(float2 *)(a.ws + part * HD + d) = make_float2(o0, o1);
            if (d == 0) *(float2 *)(a.ws + (int64_t)kv.B * a.Hq * a.nc * HD + part * 2) = make_float2(M, ls);
        }
    }
}

// combines the nc chunk partials of one (sequence, query head)
__global__ __launch_bounds__(64) void paged_decode_merge_kernel(const DecodeArgs a) {
    const int hq = blockIdx.x, b = blockIdx.y, kvh = hq / a.g, h = hq % a.g, d = 2 * threadIdx.x;
    const int64_t first = (((int64_t)b * a.kv.Hkv + kvh) * a.nc) * a.g + h;      // part index of chunk 0; chunk stride g
    float o[2];
    merge_chunks<2>(a.ws + (int64_t)a.kv.B * a.Hq * a.nc * HD, a.ws + d, first, a.g, a.nc, o);
    *(uint32_t *)(a.o + ((int64_t)b * a.Hq + hq) * HD + d) = pack_bf(o[0], o[1]);
}

template <int KIND, bool WINDOW>
hipError_t launch_decode_g(const DecodeArgs &a, hipStream_t stream) {
    const dim3 grid(a.nc, a.kv.Hkv, a.kv.B);
    if (a.g <= 4) paged_decode_kernel<KIND, 4, WINDOW><<<grid, 256, 0, stream>>>(a);
    else if (a.g <= 8) paged_decode_kernel<KIND, 8, WINDOW><<<grid, 256, 0, stream>>>(a);
    else paged_decode_kernel<KIND, 16, WINDOW><<<grid, 256, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace

namespace mm {

void kv_chunks(long long work, int target_workgroups, int max_seq_len, int round_to, int *nc, int *chunk) {
    if (work < 1) work = 1;
    const long long want = (target_workgroups + work - 1) / work;
    const int most = (max_seq_len + 255) / 256;
    int n = want < most ? (int)want : most;
    if (n < 1) n = 1;
    int cl = (max_seq_len + n - 1) / n;
    cl = (cl + round_to - 1) / round_to * round_to;
    if (cl < round_to) cl = round_to;
    *chunk = cl;
    *nc = max_seq_len > 0 ? (max_seq_len + cl - 1) / cl : 1;
}

int kv_window_span(int max_seq_len, int window, int slack) {
    return window > 0 && (long long)window + slack < max_seq_len ? window + slack : max_seq_len;
}

void kv_decode_split(int B, int Hkv, int max_seq_len, int window, int *nc, int *chunk) {
    // two workgroups per CU of the 256 on an MI355X; a chunk gives every wave whole tiles.  A window's range is the window: no slack
    kv_chunks((long long)B * Hkv, 512, kv_window_span(max_seq_len, window, 0), TILE * DEC_WAVES, nc, chunk);
}

size_t kv_decode_workspace_bytes(int B, int Hq, int Hkv, int max_seq_len, int window) {
    int nc, chunk;
    kv_decode_split(B, Hkv, max_seq_len, window, &nc, &chunk);
    return nc > 1 ? (size_t)B * Hq * nc * (HD + 2) * sizeof(float) : 0;     // DecodeArgs::ws
}

hipError_t launch_kv_append(const PagedKV &kv, const void *k, const void *v, const int *append_indptr, int T, hipStream_t stream) {
    const dim3 grid(T, kv.Hkv);
    if (kv.kind == KV_INT4) kv_append_kernel<KV_INT4><<<grid, 128, 0, stream>>>(kv, (const uint16_t *)k, (const uint16_t *)v, append_indptr);
    else if (kv.kind == KV_FP8) kv_append_kernel<KV_FP8><<<grid, 128, 0, stream>>>(kv, (const uint16_t *)k, (const uint16_t *)v, append_indptr);
    else kv_append_kernel<KV_BF16><<<grid, 128, 0, stream>>>(kv, (const uint16_t *)k, (const uint16_t *)v, append_indptr);
    return hipGetLastError();
}

hipError_t launch_paged_decode(const PagedKV &kv, const void *q, int Hq, int max_seq_len, int window, float sm_scale, void *ws, void *o,
                               hipStream_t stream) {
    DecodeArgs a;
    a.kv = kv;
    a.q = (const uint16_t *)q;
    a.ws = (float *)ws;
    a.o = (uint16_t *)o;
    a.Hq = Hq;
    a.g = Hq / kv.Hkv;
    kv_decode_split(kv.B, kv.Hkv, max_seq_len, window, &a.nc, &a.chunk);
    a.scale_log2 = kv_scale_log2(sm_scale);
    a.window = window;
    hipError_t e;
    if (kv.kind == KV_INT4) e = window > 0 ? launch_decode_g<KV_INT4, true>(a, stream) : launch_decode_g<KV_INT4, false>(a, stream);
    else if (kv.kind == KV_FP8) e = window > 0 ? launch_decode_g<KV_FP8, true>(a, stream) : launch_decode_g<KV_FP8, false>(a, stream);
    else e = window > 0 ? launch_decode_g<KV_BF16, true>(a, stream) : launch_decode_g<KV_BF16, false>(a, stream);
    if (e != hipSuccess || a.nc == 1) return e;
    paged_decode_merge_kernel<<<dim3(Hq, kv.B), 64, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace mm
