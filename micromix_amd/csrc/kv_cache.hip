// Paged KV cache: append (int4 quantize or bf16 copy) and GQA split-KV decode attention (include/micromix_hip.h, mm_kv_append /
// mm_paged_decode).  Layout and parameter convention of the reference's vendored FlashInfer cache (flashinfer/page.cuh:15,75-103,
// quantization.cuh:60-80); the quantization rule is quantize_int_group(x, 4, 128) (model/qLlamaLayer.py:13-23) with fp16 parameters.
//
//   kv_data  int4: uint8 [max_pages, L, 2, Hkv, P, 64]  (byte j = element 2j low nibble | element 2j+1 high nibble)
//            bf16: bf16  [max_pages, L, 2, Hkv, P, 128]
//   kv_param int4 only: fp16 [max_pages, L, 2, Hkv, P, 2] = (scale, zero);  value = code * scale - zero
//
// Decode: one workgroup (4 waves) per (sequence, kv head, chunk of tokens) handles all g = Hq / Hkv query heads of that kv head, so every
// cache byte is read once.  Each wave walks 32-token tiles of the chunk:
//   scores  one v_mfma_f32_16x16x32_bf16 chain per 16 tokens: A = q (16 head rows, g used), B = the K codes as bf16 (16 + code, exact),
//           so q.k = s * (q.(16 + c)) - (16 s + z) * sum(q);  for the bf16 cache B is the K row itself
//   softmax online, in the log2 domain, the max across the tile's 16 token lanes, l and sum(p z) as per-lane partials
//   p.V     VALU, fp32: a lane owns 8 dims of 8 tokens of the tile, acc[h][8] += (p s_v)[h] * code  (minus sum(p z_v) once at the end)
// The waves merge through LDS; with one chunk the workgroup writes o, otherwise (m, l, o) partials that mm_paged_decode's merge kernel
// combines.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

#include "mx_kernels.h"
#include "mx_kv_append.h"

namespace {

using namespace mm::kva;      // HD, bf16f, f2bf_rne, seq_len, kv_row, append_row, store_row

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int DEC_WAVES = 4;
constexpr int TILE = 32;           // tokens per wave iteration

// One workgroup per appended token and kv head; wave 0 writes K, wave 1 writes V (the slot and the int4 rule: mx_kv_append.h).
template <bool INT4>
__global__ __launch_bounds__(128) void kv_append_kernel(uint8_t *__restrict__ kv_data, __half *__restrict__ kv_param,
                                                        const int *__restrict__ kv_indptr, const int *__restrict__ kv_indices,
                                                        const int *__restrict__ last_page_len, const uint16_t *__restrict__ k,
                                                        const uint16_t *__restrict__ v, const int *__restrict__ append_indptr, int B,
                                                        int max_pages, int L, int layer, int Hkv, int P) {
    const int i = blockIdx.x, h = blockIdx.y, which = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = append_row(kv_indptr, kv_indices, last_page_len, append_indptr, B, i, max_pages, L, layer, which, Hkv, h, P);
    if (row < 0) return;
    const uint32_t two = ((const uint32_t *)((which ? v : k) + ((int64_t)i * Hkv + h) * HD))[lane];   // elements 2 lane, 2 lane + 1
    store_row<INT4>(kv_data, kv_param, row, lane, two);
}

// 8 int4 codes (one dword, element 2j in the low nibble of byte j) -> 8 bf16 values 16 + code (exact), MFMA operand order
__device__ inline v8bf codes_to_bf16(uint32_t w) {
    const uint32_t lo = w & 0x0f0f0f0fu, hi = (w >> 4) & 0x0f0f0f0fu;
    v4u r;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const uint32_t sel = 0x0c000c00u | ((4u + m) << 16) | (uint32_t)m;  // byte0 = lo.byte m, byte2 = hi.byte m, bytes 1, 3 = 0
        r[m] = (__builtin_amdgcn_perm(hi, lo, sel) << 3) | 0x41804180u;    // bf16 0x4180 | c << 3 = 16 + c
    }
    return __builtin_bit_cast(v8bf, r);
}

struct DecodeArgs {
    const uint16_t *q;
    const uint8_t *kv_data;
    const __half *kv_param;
    const int *kv_indptr, *kv_indices, *last_page_len;
    float *ws;                 // partials: o [B, Hkv, nc, g, 128], then (m, l) [B, Hkv, nc, g, 2]
    uint16_t *o;
    int max_pages, L, layer, Hkv, P, B, Hq, g, nc, chunk;
    float scale_log2;          // sm_scale * log2(e)
};

template <bool INT4, int GP>
__global__ __launch_bounds__(256) void paged_decode_kernel(const DecodeArgs a) {
    __shared__ float s_p[DEC_WAVES][TILE][16];        // (p * scale) of the tile, [token][head]
    __shared__ float s_alpha[DEC_WAVES][16];
    __shared__ int64_t s_row[DEC_WAVES][TILE];        // V row of each token of the tile (-1: past the chunk)
    __shared__ float s_o[DEC_WAVES][GP][HD];
    __shared__ float s_ml[DEC_WAVES][GP][2];

    const int chunk = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, kq = l >> 4;
    const int g = a.g, P = a.P;
    const int len = seq_len(a.kv_indptr, a.last_page_len, b, P);
    const int t0 = chunk * a.chunk;
    const int t1 = chunk == a.nc - 1 ? len : min(len, t0 + a.chunk);   // the last chunk runs to the end, whatever max_seq_len said
    const int *pages = a.kv_indices + a.kv_indptr[b];

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
            const int t = tb + 16 * G + c;
            int page = t < t1 ? pages[t / P] : -1;
            const bool ok = page >= 0 && page < a.max_pages;
            const int64_t rk = ok ? kv_row(page, a.L, a.layer, 0, a.Hkv, kvh, P, t % P) : 0;
            if (kq == 0) s_row[wave][16 * G + c] = ok ? rk + (int64_t)a.Hkv * P : -1;
            v4f d = {0.0f, 0.0f, 0.0f, 0.0f};
            if (INT4) {
                v4u kc = *(const v4u *)(a.kv_data + rk * (HD / 2) + 16 * kq);
                const uint32_t pk = *(const uint32_t *)(a.kv_param + rk * 2);
                const uint32_t pv = *(const uint32_t *)(a.kv_param + (rk + (int64_t)a.Hkv * P) * 2);
                if (!ok) kc = v4u{0, 0, 0, 0};
                const float sk = ok ? __half2float(__ushort_as_half((unsigned short)(pk & 0xffffu))) : 0.0f;
                const float zk = ok ? __half2float(__ushort_as_half((unsigned short)(pk >> 16))) : 0.0f;
                sv[G] = ok ? __half2float(__ushort_as_half((unsigned short)(pv & 0xffffu))) : 0.0f;
                zv[G] = ok ? __half2float(__ushort_as_half((unsigned short)(pv >> 16))) : 0.0f;
#pragma unroll
                for (int s = 0; s < 4; ++s) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[s], codes_to_bf16(kc[s]), d, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[G][r] = sk * d[r] - (16.0f * sk + zk) * sq[r];
            } else {
                const v4u *kr = (const v4u *)(a.kv_data + rk * (HD * 2) + 64 * kq);
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
        if (INT4) {
            uint32_t vc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) vc[i] = *(const uint32_t *)(a.kv_data + (rv[i] < 0 ? 0 : rv[i]) * (HD / 2) + 4 * dg);
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
        } else {
            v4u vb[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) vb[i] = *(const v4u *)(a.kv_data + (rv[i] < 0 ? 0 : rv[i]) * (HD * 2) + 16 * dg);
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
            const uint32_t packed = (uint32_t)f2bf_rne(o0 * inv) | ((uint32_t)f2bf_rne(o1 * inv) << 16);
            *(uint32_t *)(a.o + ((int64_t)b * a.Hq + hq) * HD + d) = packed;
        } else {
            const int64_t part = (((int64_t)b * a.Hkv + kvh) * a.nc + chunk) * g + h;
            *(float2 *)(a.ws + part * HD + d) = make_float2(o0, o1);
            if (d == 0) *(float2 *)(a.ws + (int64_t)a.B * a.Hq * a.nc * HD + part * 2) = make_float2(M, ls);
        }
    }
}

// combines the nc chunk partials of one (sequence, query head); a chunk without tokens has m = -inf and l = 0
__global__ __launch_bounds__(64) void paged_decode_merge_kernel(const DecodeArgs a) {
    const int hq = blockIdx.x, b = blockIdx.y, kvh = hq / a.g, h = hq % a.g, d = 2 * threadIdx.x;
    const int64_t first = (((int64_t)b * a.Hkv + kvh) * a.nc) * a.g + h;      // part index of chunk 0; chunk stride g
    const float *ml = a.ws + (int64_t)a.B * a.Hq * a.nc * HD;
    float M = -INFINITY;
    for (int c = 0; c < a.nc; ++c) M = fmaxf(M, ml[(first + (int64_t)c * a.g) * 2]);
    float ls = 0.0f, o0 = 0.0f, o1 = 0.0f;
    if (M != -INFINITY) {
        for (int c = 0; c < a.nc; ++c) {
            const int64_t part = first + (int64_t)c * a.g;
            const float f = exp2f(ml[part * 2] - M);
            const float2 v = *(const float2 *)(a.ws + part * HD + d);
            ls += f * ml[part * 2 + 1];
            o0 += f * v.x;
            o1 += f * v.y;
        }
    }
    const float inv = ls > 0.0f ? 1.0f / ls : 0.0f;
    *(uint32_t *)(a.o + ((int64_t)b * a.Hq + hq) * HD + d) = (uint32_t)f2bf_rne(o0 * inv) | ((uint32_t)f2bf_rne(o1 * inv) << 16);
}

template <bool INT4>
hipError_t launch_decode_g(const DecodeArgs &a, hipStream_t stream) {
    const dim3 grid(a.nc, a.Hkv, a.B);
    if (a.g <= 4) paged_decode_kernel<INT4, 4><<<grid, 256, 0, stream>>>(a);
    else if (a.g <= 8) paged_decode_kernel<INT4, 8><<<grid, 256, 0, stream>>>(a);
    else paged_decode_kernel<INT4, 16><<<grid, 256, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace

namespace mm {

void kv_decode_split(int B, int Hkv, int max_seq_len, int *nc, int *chunk) {
    // enough workgroups for two per CU of the 256 on an MI355X, chunks of at least 256 tokens (two tiles per wave);
    // host-known values only, so a captured graph stays valid while the sequences grow up to max_seq_len
    const int work = B * Hkv > 0 ? B * Hkv : 1;
    const int want = (512 + work - 1) / work;
    const int most = (max_seq_len + 255) / 256;
    int n = want < most ? want : most;
    if (n < 1) n = 1;
    int cl = (max_seq_len + n - 1) / n;
    cl = (cl + TILE * DEC_WAVES - 1) / (TILE * DEC_WAVES) * (TILE * DEC_WAVES);
    if (cl < TILE * DEC_WAVES) cl = TILE * DEC_WAVES;
    *chunk = cl;
    *nc = max_seq_len > 0 ? (max_seq_len + cl - 1) / cl : 1;
}

hipError_t launch_kv_append(void *kv_data, void *kv_param, bool int4, const int *kv_indptr, const int *kv_indices, const int *last_page_len,
                            int B, const void *k, const void *v, const int *append_indptr, int T, int max_pages, int L, int layer, int Hkv,
                            int P, hipStream_t stream) {
    const dim3 grid(T, Hkv);
    if (int4)
        kv_append_kernel<true><<<grid, 128, 0, stream>>>((uint8_t *)kv_data, (__half *)kv_param, kv_indptr, kv_indices, last_page_len,
                                                         (const uint16_t *)k, (const uint16_t *)v, append_indptr, B, max_pages, L, layer, Hkv, P);
    else
        kv_append_kernel<false><<<grid, 128, 0, stream>>>((uint8_t *)kv_data, nullptr, kv_indptr, kv_indices, last_page_len,
                                                          (const uint16_t *)k, (const uint16_t *)v, append_indptr, B, max_pages, L, layer, Hkv, P);
    return hipGetLastError();
}

hipError_t launch_paged_decode(const void *q, const void *kv_data, const void *kv_param, bool int4, const int *kv_indptr, const int *kv_indices,
                               const int *last_page_len, int B, int Hq, int Hkv, int max_pages, int L, int layer, int P, int max_seq_len,
                               float sm_scale, void *ws, void *o, hipStream_t stream) {
    DecodeArgs a;
    a.q = (const uint16_t *)q;
    a.kv_data = (const uint8_t *)kv_data;
    a.kv_param = (const __half *)kv_param;
    a.kv_indptr = kv_indptr;
    a.kv_indices = kv_indices;
    a.last_page_len = last_page_len;
    a.ws = (float *)ws;
    a.o = (uint16_t *)o;
    a.max_pages = max_pages;
    a.L = L;
    a.layer = layer;
    a.Hkv = Hkv;
    a.P = P;
    a.B = B;
    a.Hq = Hq;
    a.g = Hq / Hkv;
    kv_decode_split(B, Hkv, max_seq_len, &a.nc, &a.chunk);
    a.scale_log2 = sm_scale * 1.4426950408889634f;
    hipError_t e = int4 ? launch_decode_g<true>(a, stream) : launch_decode_g<false>(a, stream);
    if (e != hipSuccess || a.nc == 1) return e;
    paged_decode_merge_kernel<<<dim3(Hq, B), 64, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace mm
