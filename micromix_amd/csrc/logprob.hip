// Token log-probabilities of rows of bf16 logits (mm_logprob_rows, include/micromix_logprob.h): a target's log-probability and rank, the
// row's log-sum-exp, and the top_n tokens with their log-probabilities, the rule stated in the header.
//
// The distribution is the one sample.hip draws from: mx_row_weights.h holds the one copy of the weight w, its integer form
// W = trunc(w * 2^43) and the walk over a part, so S = sum W is the same 64-bit integer here and there, whatever the order of the sum.
// The logarithm is taken once per row, of that integer, in fp64; everything before it is exact integer arithmetic on the device, and
// so are the rank (a count of keys) and the top_n (a selection under the total order on (key, index) of mx_argmax_key.h).
//
// The launches of one call, each on the whole batch:
//   argmax_rows (verify.hip)     amax[r] = the row's argmax, so m = logits[r][amax[r]] for the sweep
//   sweep, grid (parts, rows)    a lane keeps its 32 (+ 1 peeled) columns in registers; a part writes its sum of W, its count of keys
//                                above the target's, and -- top_n > 0 -- its top_n largest (key, index) pairs in descending order
//   finish, grid rows            adds the parts, selects the row's top_n among the parts' candidates, takes the logarithm, writes all
// Selecting the n largest of a workgroup's register-held values is a radix select in LDS: a 256-bin count histogram of the key's high
// byte, the bin in which the count from the top reaches n, a second histogram of the low byte inside that bin: the threshold key.
// Only keys at or above a floor are counted (block_select says which), so the atomics of a wave do not all fall on a few LDS words.
// Every value above it is taken, and of the values at it the lowest indices, one workgroup maximum each.  The histograms are integer
// LDS atomics and the taken values are ranked against each other before they are written, so nothing depends on the order in which
// lanes or workgroups run.  Every workspace word read was stored by an earlier kernel of the same call.
#include "../../include/micromix_logprob.h"
#include "mx_argmax_key.h"
#include "mx_kernels.h"
#include "mx_row_weights.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

constexpr int LP_MAX_TOP = 32;                                                      // top_n of the header
constexpr int LP_SLOTS = SMP_RUN + 1;                                               // a lane's columns of a part: 4 vectors and a peeled one
constexpr int LP_MERGE = MM_ARGMAX_MAX_VOCAB / MM_ARGMAX_CHUNK * LP_MAX_TOP / SMP_THREADS;   // a lane's candidates of a row in the finish
static_assert(LP_MERGE * SMP_THREADS == MM_ARGMAX_MAX_VOCAB / MM_ARGMAX_CHUNK * LP_MAX_TOP, "the candidates of a row divide among the lanes");

struct LogprobParams {
    const uint16_t *logits;
    long long ld;
    int vocab;
    const int *amax;         // the argmax of every row, written by argmax_rows before any kernel here
    const int *target;
    const float *temperature;
    int top_n;
};

// a row's parameters as the rule reads them
struct LogprobRule {
    float m, c, T;           // the maximum, log2e / T', T'
    unsigned tbits, tkey;    // the target's logit and its key
    bool degenerate, has_target;
};

__device__ inline LogprobRule logprob_rule(const LogprobParams &a, int row) {
    LogprobRule r;
    const uint16_t *p = a.logits + (long long)row * a.ld;
    const unsigned mbits = p[a.amax[row]], mkey = argmax_key(mbits);
    const float T = a.temperature ? a.temperature[row] : 1.0f;
    r.T = T > 0.0f ? T : 1.0f;                                                       // T <= 0 or NaN: the unscaled distribution
    r.m = __uint_as_float(mbits << 16);
    r.c = LOG2E / r.T;
    r.degenerate = mkey == 0u || mkey >= KEY_POS_INF;                               // -inf, +inf, NaN
    const int tgt = a.target ? a.target[row] : -1;
    r.has_target = tgt >= 0 && tgt < a.vocab;
    r.tbits = r.has_target ? p[tgt] : 0u;                                           // nothing is read through an ignored index
    r.tkey = argmax_key(r.tbits);
    return r;
}

// the log-probability of a token of a row whose S gave L
__device__ inline float logprob_of(unsigned bits, const LogprobRule &r, double L) {
    if (r.degenerate) return __builtin_nanf("");
    if (argmax_key(bits) == 0u) return -__builtin_inff();
    return (float)(((double)__uint_as_float(bits << 16) - (double)r.m) / (double)r.T - L);
}

// ---- the n largest of a workgroup's values ------------------------------------------------------------------------------------------
// A value holds a key above the bitwise complement of an index (argmax_pack's layout, in 32 or 64 bits), so the larger value is the
// larger key, then the lower index; values are pairwise distinct and never 0, and 0 marks a register that holds none.
struct SelectShared {
    unsigned cnt[256], wave[SMP_THREADS / 64];
    u64 list[LP_MAX_TOP], out[LP_MAX_TOP], red[SMP_THREADS / 64];
    unsigned group[SMP_THREADS / 32];
    unsigned n_list, need;
    int bin;
};

__device__ inline u64 wave_max64(u64 x) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const u64 y = (u64)__shfl_xor((long long)x, off);
        x = x > y ? x : y;
    }
    return x;
}

// s.out[0 .. n) = the n largest of the workgroup's values v, in descending order; 1 <= n <= LP_MAX_TOP and at least n values exist.
// SHIFT: the bits below the 16-bit key.  Every lane of the workgroup calls it, with the same n
template <class P, int SHIFT, int SLOTS>
__device__ inline void block_select(const P (&v)[SLOTS], unsigned n, int t, SelectShared &s) {
    static_assert(LP_MAX_TOP <= 32, "a group of 32 lanes that all hold a value holds n values at or above its smallest lane maximum");
    unsigned kt = 0, need = n;                                                      // the threshold key, high byte first; values still wanted
    if (t == 0) s.n_list = 0;
    // a floor under the threshold key, so that the histograms count a few values and not all: the smallest lane maximum of a group of
    // 32 lanes has 32 >= n values at or above it; the largest such over the groups is taken.  Kept as key + 1, 0 for a lane without a
    // value (its group then gives no floor)
    unsigned top = 0;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i)
        if (v[i] != 0) top = max(top, (unsigned)(v[i] >> SHIFT) + 1u);
#pragma unroll
    for (int off = 16; off; off >>= 1) top = min(top, (unsigned)__shfl_xor((int)top, off));
    if ((t & 31) == 0) s.group[t >> 5] = top;
    unsigned floor_key = 0;
#pragma unroll
    for (int level = 1; level <= 2; ++level) {
        s.cnt[t] = 0;
        __syncthreads();
        if (level == 1) {
#pragma unroll
            for (int g = 0; g < SMP_THREADS / 32; ++g) floor_key = max(floor_key, s.group[g]);
            floor_key = floor_key ? floor_key - 1u : 0u;
        }
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const unsigned key = (unsigned)(v[i] >> SHIFT);
            if (v[i] != 0 && key >= floor_key && (level == 1 || (key >> 8) == kt)) atomicAdd(&s.cnt[level == 1 ? key >> 8 : key & 255u], 1u);
        }
        __syncthreads();
        const unsigned own = s.cnt[t];
        unsigned here = own;                                                        // suffix sums: bin t and every bin above it,
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {                                    // inside the wave by shuffles ...
            const unsigned above = (unsigned)__shfl_down((int)here, off);
            if ((t & 63) + off < 64) here += above;
        }
        if ((t & 63) == 0) s.wave[t >> 6] = here;
        __syncthreads();
        for (int w = (t >> 6) + 1; w < SMP_THREADS / 64; ++w) here += s.wave[w];    // ... and the waves above
        const unsigned next = here - own;
        if (here >= need && next < need) {                                          // one lane: the largest bin that reaches `need`
            s.bin = t;
            s.need = need - next;
        }
        __syncthreads();
        kt = kt << 8 | (unsigned)s.bin;
        need = min(s.need, n);                                                      // (at most n by construction: the loop below is bounded)
        __syncthreads();
    }
    // the n - need values above the threshold key, in any order
#pragma unroll
    for (int i = 0; i < SLOTS; ++i)
        if (v[i] != 0 && (unsigned)(v[i] >> SHIFT) > kt) s.list[atomicAdd(&s.n_list, 1u)] = (u64)v[i];
    // the `need` largest values at the threshold key: the lowest indices
    P last = ~(P)0;
    for (unsigned r = 0; r < need; ++r) {
        P mine = 0;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i)
            if ((unsigned)(v[i] >> SHIFT) == kt && v[i] < last && v[i] > mine) mine = v[i];
        const u64 w = wave_max64((u64)mine);
        if ((t & 63) == 0) s.red[t >> 6] = w;
        __syncthreads();
        u64 best = s.red[0];
#pragma unroll
        for (int k = 1; k < SMP_THREADS / 64; ++k) best = best > s.red[k] ? best : s.red[k];
        if (t == 0) s.list[n - need + r] = best;
        last = (P)best;
        __syncthreads();
    }
    // each taken value finds its place among the others
    if ((unsigned)t < n) {
        const u64 x = s.list[t];
        unsigned place = 0;
        for (unsigned j = 0; j < n; ++j) place += s.list[j] > x;
        s.out[place] = x;
    }
    __syncthreads();
}

__device__ inline unsigned wave_add(unsigned x) {
#pragma unroll
    for (int off = 32; off; off >>= 1) x += (unsigned)__shfl_xor((int)x, off);
    return x;
}

// grid (parts, rows): the part's sum of W, its count of keys above the target's, its top_n candidates
__global__ __launch_bounds__(SMP_THREADS) void logprob_sweep_kernel(LogprobParams a, u64 *__restrict__ part_sum,
                                                                    unsigned *__restrict__ part_cnt, u64 *__restrict__ cand) {
    __shared__ SelectShared s;
    __shared__ u64 s_sum[SMP_THREADS / 64];
    __shared__ unsigned s_cnt[SMP_THREADS / 64];
    const int t = threadIdx.x, row = blockIdx.y, lo = blockIdx.x * MM_ARGMAX_CHUNK;
    const int len = min(a.vocab - lo, MM_ARGMAX_CHUNK);
    const LogprobRule r = logprob_rule(a, row);
    unsigned v[LP_SLOTS];                                                           // key << 16 | 0xFFFF - the column inside the part
#pragma unroll
    for (int i = 0; i < LP_SLOTS; ++i) v[i] = 0u;
    u64 sum = 0;
    unsigned above = 0;
    for_each_in_part_at(a.logits + (long long)row * a.ld + lo, len, t, [&](unsigned bits, int slot, int col) {
        const unsigned key = argmax_key(bits);
        sum += fixed(weight(bits, key, r));
        above += key > r.tkey;
        v[slot] = key << 16 | (0xFFFFu - (unsigned)col);
    });
    sum = wave_sum(sum);
    above = wave_add(above);
    if ((t & 63) == 0) {
        s_sum[t >> 6] = sum;
        s_cnt[t >> 6] = above;
    }
    __syncthreads();
    const long long at = (long long)row * gridDim.x + blockIdx.x;
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < SMP_THREADS / 64; ++w) {
            sum += s_sum[w];
            above += s_cnt[w];
        }
        part_sum[at] = sum;
        part_cnt[at] = above;
    }
    if (a.top_n == 0) return;
    const unsigned n = (unsigned)min(a.top_n, len);
    block_select<unsigned, 16, LP_SLOTS>(v, n, t, s);
    if (t < a.top_n) {                                                              // a short part fills up with "none"
        const unsigned x = (unsigned)s.out[(unsigned)t < n ? t : 0];
        const unsigned col = (unsigned)lo + (0xFFFFu - (x & 0xFFFFu));
        cand[at * a.top_n + t] = (unsigned)t < n ? (u64)(x >> 16) << 32 | (0xFFFFFFFFu - col) : 0ull;
    }
}

// grid rows: S and the count over the parts, the row's top_n among the parts' candidates, the logarithm, every output
__global__ __launch_bounds__(SMP_THREADS) void logprob_finish_kernel(LogprobParams a, int parts, const u64 *__restrict__ part_sum,
                                                                     const unsigned *__restrict__ part_cnt, const u64 *__restrict__ cand,
                                                                     float *__restrict__ logprob, int *__restrict__ rank,
                                                                     float *__restrict__ lse, int *__restrict__ top_idx,
                                                                     float *__restrict__ top_logprob) {
    __shared__ SelectShared s;
    __shared__ u64 s_sum[SMP_THREADS / 64];
    __shared__ unsigned s_cnt[SMP_THREADS / 64];
    const int t = threadIdx.x, row = blockIdx.x;
    const LogprobRule r = logprob_rule(a, row);
    u64 sum = 0;
    unsigned above = 0;
    for (int c = t; c < parts; c += SMP_THREADS) {
        sum += part_sum[(long long)row * parts + c];
        above += part_cnt[(long long)row * parts + c];
    }
    sum = wave_sum(sum);
    above = wave_add(above);
    if ((t & 63) == 0) {
        s_sum[t >> 6] = sum;
        s_cnt[t >> 6] = above;
    }
    __syncthreads();
    sum = s_sum[0];
    above = s_cnt[0];
#pragma unroll
    for (int w = 1; w < SMP_THREADS / 64; ++w) {
        sum += s_sum[w];
        above += s_cnt[w];
    }
    const double L = log((double)sum * 0x1p-43);                                    // the product is exact: S = 2^43 gives 0
    if (t == 0) {
        if (lse) lse[row] = r.degenerate ? __builtin_nanf("") : (float)((double)r.m / (double)r.T + L);
        if (logprob) logprob[row] = r.has_target ? logprob_of(r.tbits, r, L) : 0.0f;
        if (rank) rank[row] = r.has_target ? (int)above : -1;
    }
    if (a.top_n == 0) return;
    const int total = parts * a.top_n;
    u64 v[LP_MERGE];
#pragma unroll
    for (int i = 0; i < LP_MERGE; ++i) {
        const int at = t + i * SMP_THREADS;
        v[i] = at < total ? cand[(long long)row * total + at] : 0ull;
    }
    const unsigned n = (unsigned)min(a.top_n, a.vocab);
    block_select<u64, 32, LP_MERGE>(v, n, t, s);
    if (t < a.top_n) {
        const long long at = (long long)row * a.top_n + t;
        const unsigned col = 0xFFFFFFFFu - (unsigned)s.out[(unsigned)t < n ? t : 0];
        if ((unsigned)t < n && col < (unsigned)a.vocab) {                           // (a column is inside the row by construction)
            top_idx[at] = (int)col;
            top_logprob[at] = logprob_of(a.logits[(long long)row * a.ld + col], r, L);
        } else {                                                                    // beyond the vocabulary
            top_idx[at] = -1;
            top_logprob[at] = -__builtin_inff();
        }
    }
}

struct LogprobWorkspace {
    size_t amax, argmax, part_sum, cand, part_cnt, total;
};

static LogprobWorkspace logprob_layout(int rows, int vocab, int top_n) {
    const size_t n = (size_t)rows * (size_t)argmax_parts(vocab);
    LogprobWorkspace w;
    w.amax = 0;
    w.argmax = w.amax + ((size_t)rows * sizeof(int) + 7) / 8 * 8;
    w.part_sum = w.argmax + argmax_workspace_bytes(rows, vocab);
    w.cand = w.part_sum + n * sizeof(u64);
    w.part_cnt = w.cand + n * (size_t)top_n * sizeof(u64);
    w.total = w.part_cnt + (n * sizeof(unsigned) + 7) / 8 * 8;
    return w;
}

size_t logprob_workspace_bytes(int rows, int vocab, int top_n) { return logprob_layout(rows, vocab, top_n).total; }

hipError_t launch_logprob_rows(const void *logits, int rows, int vocab, long long ld, const int *target, const float *temperature,
                               float *logprob, int *rank, float *lse, int top_n, int *top_idx, float *top_logprob, void *ws,
                               hipStream_t stream) {
    static_assert(LP_SLOTS <= 64 && MM_ARGMAX_CHUNK <= 65536, "a column inside a part fits the 16 bits below the key");
    const int parts = argmax_parts(vocab);
    const LogprobWorkspace w = logprob_layout(rows, vocab, top_n);
    char *base = (char *)ws;
    int *amax = (int *)(base + w.amax);
    u64 *part_sum = (u64 *)(base + w.part_sum), *cand = (u64 *)(base + w.cand);
    unsigned *part_cnt = (unsigned *)(base + w.part_cnt);
    hipError_t e = launch_argmax_rows(logits, rows, vocab, ld, amax, base + w.argmax, stream);
    if (e != hipSuccess) return e;
    const LogprobParams a{(const uint16_t *)logits, ld, vocab, amax, target, temperature, top_n};
    logprob_sweep_kernel<<<dim3(parts, rows), SMP_THREADS, 0, stream>>>(a, part_sum, part_cnt, cand);
    logprob_finish_kernel<<<rows, SMP_THREADS, 0, stream>>>(a, parts, part_sum, part_cnt, cand, logprob, rank, lse, top_idx, top_logprob);
    return hipGetLastError();
}

}  // namespace mm
