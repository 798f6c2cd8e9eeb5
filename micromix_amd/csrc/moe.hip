// The glue of a sparse MoE block around the grouped expert GEMMs (include/micromix_hip.h, mm_moe_*): top-k routing of the gate logits,
// a stable counting sort of the (token, k-slot) pairs by expert, the gather of every expert's rows, and the weighted combine of the
// expert outputs.  Four small kernels; none reads device data on the host, needs zeroed state or a workspace, and no atomic decides an
// order, so every result is the same in every launch and the launches are capture-safe.
//
//   route    one wave per token, lane e holds logit e (E <= 64); top_k rounds of a cross-lane arg-max over (value, lower index first)
//   plan     one workgroup per chunk of PLAN_CHUNK pairs.  A workgroup counts, by reading the ids again, what every expert owns in all
//            pairs and in the pairs before its chunk (O(n^2 / PLAN_CHUNK) id reads in all, from L2; no scratch array between
//            workgroups, hence no second launch and nothing to clear), then ranks its own pairs in order
//   gather   one workgroup per sorted row, 16-byte loads and stores
//   combine  one workgroup per token: the token's top_k entries sorted by expert id (a fixed network on 8 packed keys, wave-uniform),
//            then acc = bf16(acc + bf16(y * w)) in that order -- what zeros + index_add_ expert by expert computes
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mx_kernels.h"

namespace {

constexpr int MAX_E = 64, MAX_K = 8;

__device__ inline float bf16f(uint32_t bits16) { return __uint_as_float(bits16 << 16); }

__device__ inline uint32_t f2bf_rne(float f) {    // torch's rounding: NaN -> 0x7fc0, the rest to nearest even (overflow to inf)
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ inline uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
        const uint64_t other = ((uint64_t)hi << 32) | lo;
        v = other > v ? other : v;
    }
    return v;
}

// ---- route ------------------------------------------------------------------------------------------------------------------------
constexpr int ROUTE_WAVES = 4;

__global__ __launch_bounds__(64 * ROUTE_WAVES) void moe_route_kernel(const uint16_t *logits, int T, int E, int top_k, int *ids, uint16_t *w) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * ROUTE_WAVES + (threadIdx.x >> 6);
    if (t >= T) return;                                       // whole waves leave
    float l = 0.0f;
    uint64_t key = 0;                                         // 0: not a candidate (lane >= E, or already taken)
    if (lane < E) {
        uint32_t u = (uint32_t)logits[t * E + lane] << 16;
        if ((u & 0x7fffffffu) == 0) u = 0;                    // -0.0 ties with +0.0
        l = __uint_as_float(u);
        const uint32_t ordered = u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);       // unsigned order = float order
        key = (((uint64_t)ordered + 1) << 8) | (uint32_t)(63 - lane);               // equal values: the lower lane is the larger key
    }
    int my_id = 0;
    float my_l = 0.0f, top = 0.0f;
    for (int j = 0; j < top_k; ++j) {
        const int win = 63 - (int)(wave_max_u64(key) & 0xff);
        const float lw = __shfl(l, win);
        if (lane == win) key = 0;
        if (lane == j) { my_id = win; my_l = lw; }
        if (j == 0) top = lw;
    }
    float e = lane < top_k ? expf(my_l - top) : 0.0f, sum = e;
#pragma unroll
    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);  // the same tree in every launch
    if (lane < top_k) {
        ids[t * top_k + lane] = my_id;
        w[t * top_k + lane] = (uint16_t)f2bf_rne(__fdiv_rn(e, sum));
    }
}

// ---- plan -------------------------------------------------------------------------------------------------------------------------
constexpr int PLAN_WAVES = 16, PLAN_THREADS = 64 * PLAN_WAVES, PLAN_ROUNDS = 4, PLAN_CHUNK = PLAN_THREADS * PLAN_ROUNDS;

// Integer LDS adds only sum counts (any order gives the same sum); where an add hands out slots, one lane per (wave, expert) issues
// it on the wave's own counter, in program order.
__global__ __launch_bounds__(PLAN_THREADS) void moe_plan_kernel(const int *ids, int n, int E, int top_k, int *offsets, int *sorted_token,
                                                               int *slot_of) {
    __shared__ int hist[PLAN_WAVES][MAX_E];                   // per wave: counts, later the next free slot of (wave, expert)
    __shared__ int before[MAX_E], start[MAX_E], routed;       // routed: pairs with an id inside [0, E)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t chunk0 = (int64_t)blockIdx.x * PLAN_CHUNK;
    auto clear = [&]() {
        for (int i = tid; i < PLAN_WAVES * MAX_E; i += PLAN_THREADS) (&hist[0][0])[i] = 0;
        __syncthreads();
    };
    auto count = [&](int64_t lo, int64_t hi) {
        for (int64_t p = lo + tid; p < hi; p += PLAN_THREADS) {
            const int e = ids[p];
            if (e >= 0 && e < E) atomicAdd(&hist[wave][e], 1);
        }
        __syncthreads();
    };
    auto total = [&](int e) {
        int s = 0;
        for (int w = 0; w < PLAN_WAVES; ++w) s += hist[w][e];
        return s;
    };
    clear();
    count(0, chunk0);                                         // what every expert owns before this chunk
    if (tid < E) before[tid] = total(tid);
    __syncthreads();
    count(chunk0, n);                                         // ... and in all pairs (the counters go on)
    if (tid < MAX_E) {                                        // wave 0: exclusive scan of the totals over the experts
        const int c = tid < E ? total(tid) : 0;
        int s = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(s, o);
            if (lane >= o) s += up;
        }
        if (tid < E) start[tid] = s - c;
        if (tid == E - 1) routed = s;
        if (blockIdx.x == 0) {
            if (tid < E) offsets[tid] = s - c;
            if (tid == E - 1) offsets[E] = s;
        }
    }
    __syncthreads();
    clear();
    // this wave's pairs: chunk0 + wave * 256 + r * 64 + lane, in that order
    int my[PLAN_ROUNDS];
#pragma unroll
    for (int r = 0; r < PLAN_ROUNDS; ++r) {
        const int64_t p = chunk0 + wave * (64 * PLAN_ROUNDS) + r * 64 + lane;
        const int e = p < n ? ids[p] : -1;
        my[r] = e >= 0 && e < E ? e : -1;
        if (my[r] >= 0) atomicAdd(&hist[wave][my[r]], 1);
    }
    __syncthreads();
    if (tid < E) {                                            // counts -> first slot of (wave, expert)
        int run = start[tid] + before[tid];
        for (int w = 0; w < PLAN_WAVES; ++w) {
            const int c = hist[w][tid];
            hist[w][tid] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PLAN_ROUNDS; ++r) {
        const int64_t p = chunk0 + wave * (64 * PLAN_ROUNDS) + r * 64 + lane;
        const int e = my[r];
        uint64_t same = __ballot(e >= 0);                     // the lanes of this round with my expert
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const uint64_t bit = __ballot((e >> b) & 1);
            same &= ((e >> b) & 1) ? bit : ~bit;
        }
        int base = 0;
        if (e >= 0) {
            const int first = __ffsll((unsigned long long)same) - 1;
            if (lane == first) base = atomicAdd(&hist[wave][e], __popcll(same));
            base = __shfl(base, first);
            const int slot = base + __popcll(same & ((1ull << lane) - 1));
            sorted_token[slot] = (int)(p / top_k);
            slot_of[p] = slot;
        } else if (p < n) {
            slot_of[p] = -1;
        }
        if (p >= routed && p < n) sorted_token[p] = -1;       // the slots no pair owns (ids outside [0, E) were not counted)
    }
}

// ---- gather -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void moe_gather_kernel(const uint4 *x, const int *sorted_token, int T, int V, uint4 *x_sorted) {
    const int t = sorted_token[blockIdx.x];
    if (t < 0 || t >= T) return;
    const uint4 *src = x + (int64_t)t * V;
    uint4 *dst = x_sorted + (int64_t)blockIdx.x * V;
    int v = threadIdx.x;
    for (; v + (int)blockDim.x < V; v += 2 * blockDim.x) {    // two loads in flight per lane
        const uint4 a = src[v], b = src[v + blockDim.x];
        dst[v] = a;
        dst[v + blockDim.x] = b;
    }
    if (v < V) dst[v] = src[v];
}

// ---- combine ----------------------------------------------------------------------------------------------------------------------
__device__ inline void order(uint64_t &a, uint64_t &b) {
    const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// one bf16 pair of acc (as floats holding bf16 values) += bf16(y * w)
__device__ inline void add_pair(float &a0, float &a1, uint32_t y, float w) {
    const float c0 = bf16f(f2bf_rne(bf16f(y & 0xffffu) * w)), c1 = bf16f(f2bf_rne(bf16f(y >> 16) * w));
    a0 = bf16f(f2bf_rne(a0 + c0));
    a1 = bf16f(f2bf_rne(a1 + c1));
}

template <int K>
__global__ __launch_bounds__(256) void moe_combine_kernel(const uint4 *y, const int *ids, const uint16_t *w, const int *slot_of, int n_rows,
                                                         int V, uint4 *out) {
    const int64_t t = blockIdx.x;
    // key: expert id | k-slot | weight bits | slot, so that sorting the keys sorts by expert id (the k-slot breaks a tie that a routed
    // token never has); entries without a slot sort wherever their id puts them and are skipped below
    uint64_t key[MAX_K];
#pragma unroll
    for (int j = 0; j < MAX_K; ++j) {
        key[j] = ~0ull;
        if (j < K) {
            const int id = ids[t * K + j], s = slot_of[t * K + j];
            const bool ok = s >= 0 && s < n_rows;
            key[j] = ((uint64_t)(uint32_t)(id & 0xff) << 56) | ((uint64_t)j << 53) | ((uint64_t)w[t * K + j] << 32) | (ok ? (uint32_t)s : 0xffffffffu);
        }
    }
    // Batcher's odd-even merge sort of 8, 19 exchanges
    order(key[0], key[1]); order(key[2], key[3]); order(key[4], key[5]); order(key[6], key[7]);
    order(key[0], key[2]); order(key[1], key[3]); order(key[4], key[6]); order(key[5], key[7]);
    order(key[1], key[2]); order(key[5], key[6]);
    order(key[0], key[4]); order(key[1], key[5]); order(key[2], key[6]); order(key[3], key[7]);
    order(key[2], key[4]); order(key[3], key[5]);
    order(key[1], key[2]); order(key[3], key[4]); order(key[5], key[6]);
    for (int v = threadIdx.x; v < V; v += blockDim.x) {
        uint4 row[K];
#pragma unroll
        for (int r = 0; r < K; ++r) {                         // every load issued before the first is used
            const uint32_t s = (uint32_t)key[r];
            row[r] = y[(int64_t)(s == 0xffffffffu ? 0u : s) * V + v];
        }
        float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int r = 0; r < K; ++r) {
            if ((uint32_t)key[r] == 0xffffffffu) continue;
            const float wr = bf16f((uint32_t)(key[r] >> 32) & 0xffffu);
            add_pair(acc[0], acc[1], row[r].x, wr);
            add_pair(acc[2], acc[3], row[r].y, wr);
            add_pair(acc[4], acc[5], row[r].z, wr);
            add_pair(acc[6], acc[7], row[r].w, wr);
        }
        uint4 o;
        o.x = (__float_as_uint(acc[0]) >> 16) | (__float_as_uint(acc[1]) & 0xffff0000u);
        o.y = (__float_as_uint(acc[2]) >> 16) | (__float_as_uint(acc[3]) & 0xffff0000u);
        o.z = (__float_as_uint(acc[4]) >> 16) | (__float_as_uint(acc[5]) & 0xffff0000u);
        o.w = (__float_as_uint(acc[6]) >> 16) | (__float_as_uint(acc[7]) & 0xffff0000u);
        out[t * V + v] = o;
    }
}

// ---- zero rows (mm_moe_matmul without a segment) ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void moe_zero_rows_kernel(uint16_t *D, const int *offsets, int E, int n, int N) {
    const int owned = offsets[E];
    if ((int)blockIdx.x >= owned || owned > n) return;
    uint16_t *row = D + (int64_t)blockIdx.x * N;
    for (int c = threadIdx.x; c < N; c += blockDim.x) row[c] = 0;
}

int row_threads(int V) { return V >= 256 ? 256 : (V + 63) / 64 * 64; }

}  // namespace

namespace mm {

hipError_t launch_moe_route(const void *logits, int T, int E, int top_k, int *ids, void *w, hipStream_t stream) {
    moe_route_kernel<<<(T + ROUTE_WAVES - 1) / ROUTE_WAVES, 64 * ROUTE_WAVES, 0, stream>>>((const uint16_t *)logits, T, E, top_k, ids, (uint16_t *)w);
    return hipGetLastError();
}

hipError_t launch_moe_plan(const int *ids, int n, int E, int top_k, int *offsets, int *sorted_token, int *slot_of, hipStream_t stream) {
    moe_plan_kernel<<<(n + PLAN_CHUNK - 1) / PLAN_CHUNK, PLAN_THREADS, 0, stream>>>(ids, n, E, top_k, offsets, sorted_token, slot_of);
    return hipGetLastError();
}

hipError_t launch_moe_gather(const void *x, const int *sorted_token, int T, int n_rows, int H, void *x_sorted, hipStream_t stream) {
    const int V = H / 8;
    moe_gather_kernel<<<n_rows, row_threads(V), 0, stream>>>((const uint4 *)x, sorted_token, T, V, (uint4 *)x_sorted);
    return hipGetLastError();
}

hipError_t launch_moe_combine(const void *y, const int *ids, const void *w, const int *slot_of, int T, int top_k, int H, void *out,
                              hipStream_t stream) {
    const int V = H / 8, threads = row_threads(V), n_rows = T * top_k;
    const uint4 *y4 = (const uint4 *)y;
    const uint16_t *w16 = (const uint16_t *)w;
    uint4 *o4 = (uint4 *)out;
    switch (top_k) {
        case 1: moe_combine_kernel<1><<<T, threads, 0, stream>>>(y4, ids, w16, slot_of, n_rows, V, o4); break;
        case 2: moe_combine_kernel<2><<<T, threads, 0, stream>>>(y4, ids, w16, slot_of, n_rows, V, o4); break;
        case 3: moe_combine_kernel<3><<<T, threads, 0, stream>>>(y4, ids, w16, slot_of, n_rows, V, o4); break;
        case 4: moe_combine_kernel<4><<<T, threads, 0, stream>>>(y4, ids, w16, slot_of, n_rows, V, o4); break;
        case 5: moe_combine_kernel<5><<<T, threads, 0, stream>>>(y4, ids, w16, slot_of, n_rows, V, o4); break;
        case 6: moe_combine_kernel<6><<<T, threads, 0, stream>>>(y4, ids, w16, slot_of, n_rows, V, o4); break;
        case 7: moe_combine_kernel<7><<<T, threads, 0, stream>>>(y4, ids, w16, slot_of, n_rows, V, o4); break;
        default: moe_combine_kernel<8><<<T, threads, 0, stream>>>(y4, ids, w16, slot_of, n_rows, V, o4); break;
    }
    return hipGetLastError();
}

hipError_t launch_moe_zero_rows(void *D, const int *offsets, int E, int n, int N, hipStream_t stream) {
    moe_zero_rows_kernel<<<n, 256, 0, stream>>>((uint16_t *)D, offsets, E, n, N);
    return hipGetLastError();
}

}  // namespace mm
