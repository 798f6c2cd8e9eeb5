// The weights of a row of bf16 logits as integers, and the walk over one part of a row, shared by sample.hip (mm_sample_rows) and
// logprob.hip (mm_logprob_rows): one copy, so that the distribution whose logarithm is reported is the one that is drawn from.
//
// A weight w = exp2((l - m) * c), c = log2e / T, fp32 in [0, 1], becomes W = trunc(w * 2^43), a 64-bit integer: 2^20 of them cannot
// overflow and integer addition is associative, so a sum of W's is the same number however a row is divided among lanes, waves and
// workgroups and whoever finishes first.
//
// logits_process.hip (mm_process_logits) uses the walk alone, and the two helpers that write a walked part back: part_head, store_part.
#pragma once

#include "../../include/micromix_hip.h"
#include "mx_argmax_key.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

typedef unsigned long long u64;

constexpr int SMP_THREADS = 256, SMP_VECS = MM_ARGMAX_CHUNK / 8 / SMP_THREADS;      // lanes per workgroup; 16-byte vectors per lane
constexpr int SMP_RUN = MM_ARGMAX_CHUNK / SMP_THREADS;                              // consecutive columns per lane in the draw
static_assert(SMP_VECS * SMP_THREADS * 8 == MM_ARGMAX_CHUNK && SMP_RUN * SMP_THREADS == MM_ARGMAX_CHUNK, "a part divides among the lanes");
constexpr float SMP_ONE = 0x1p43f;                                                  // W of the maximum: 2^20 tokens stay below 2^64
constexpr float LOG2E = 1.4426950408889634f;

// w of one token of a row whose rule `r` holds the maximum r.m and r.c = log2e / T.  l == m gives exactly 1 whatever T (0 * inf never
// forms); -inf gives 0 whatever T (inf * 0 never forms)
template <class Rule>
__device__ inline float weight(unsigned bits, unsigned key, const Rule &r) {
    const float d = __uint_as_float(bits << 16) - r.m;
    const float t = d == 0.0f ? 0.0f : d * r.c;
    return key == 0u ? 0.0f : __builtin_amdgcn_exp2f(t);
}

__device__ inline u64 fixed(float w) { return (u64)(w * SMP_ONE); }

// f(bits, slot, col) for every column of a part, each once, in no particular order: the peel and the vector loads of
// argmax_rows_kernel.  `col` counts from the part's first column; `slot` names the register the lane holds the column in, a constant
// once the loops are unrolled: 8 u + e for element e of the lane's vector u, SMP_RUN for its peeled element
template <class F>
__device__ inline void for_each_in_part_at(const uint16_t *p, int len, int t, F f) {
    const int head = min(len, (int)((8u - (unsigned)((uintptr_t)p >> 1)) & 7u));    // elements in front of the first 16-byte boundary
    const int nb = (len - head) >> 3, tail = len - head - 8 * nb;                   // whole vectors; elements behind the last
    const us8 *body = (const us8 *)(p + head);
    us8 raw[SMP_VECS];
#pragma unroll
    for (int u = 0; u < SMP_VECS; ++u) {
        const int v = t + u * SMP_THREADS;
        raw[u] = v < nb ? body[v] : (us8)BF16_NEG_INF;
    }
    // lanes 0 .. 7 the head, lanes 8 .. 15 the tail, an element each
    const int peel = t < head ? t : (t >= 8 && t - 8 < tail) ? head + 8 * nb + t - 8 : -1;
    const unsigned peeled = peel >= 0 ? p[peel] : 0u;
#pragma unroll
    for (int u = 0; u < SMP_VECS; ++u) {
        if (t + u * SMP_THREADS < nb) {                                             // a filled vector is no token: it is not counted
#pragma unroll
            for (int e = 0; e < 8; ++e) f((unsigned)raw[u][e], 8 * u + e, head + 8 * (t + u * SMP_THREADS) + e);
        }
    }
    if (peel >= 0) f(peeled, SMP_RUN, peel);
}

// f(bits) for every column of a part: the same walk for a caller that needs no place
template <class F>
__device__ inline void for_each_in_part(const uint16_t *p, int len, int t, F f) {
    for_each_in_part_at(p, len, t, [&](unsigned bits, int, int) { f(bits); });
}

// the elements the walk finds in front of the first 16-byte boundary of a part read at p: slot 8 u + e of lane t is column
// part_head + 8 (t + u SMP_THREADS) + e
__device__ inline int part_head(const uint16_t *p, int len) { return min(len, (int)((8u - (unsigned)((uintptr_t)p >> 1)) & 7u)); }

// The walk's columns written back: v[u][e] is the new value of the column the walk handed out as slot 8 u + e, `peeled` that of slot
// SMP_RUN, for the lane's columns of the part of `len` columns that was read at p and is written at q (q == p: in place).  Every lane
// writes exactly the columns it was handed.  Where q is congruent to p mod 16 a vector of p is a vector of q and goes out as one
// 16-byte store; otherwise its 8 elements go out one by one: the same bits either way
__device__ inline void store_part(uint16_t *q, const uint16_t *p, int len, int t, const us8 (&v)[SMP_VECS], unsigned peeled) {
    const int head = part_head(p, len);
    const int nb = (len - head) >> 3, tail = len - head - 8 * nb;
    const bool congruent = ((((uintptr_t)q ^ (uintptr_t)p) >> 1) & 7u) == 0;
#pragma unroll
    for (int u = 0; u < SMP_VECS; ++u) {
        const int at = t + u * SMP_THREADS;
        if (at < nb) {
            if (congruent) {
                *(us8 *)(q + head + 8 * at) = v[u];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) q[head + 8 * at + e] = (uint16_t)v[u][e];
            }
        }
    }
    const int peel = t < head ? t : (t >= 8 && t - 8 < tail) ? head + 8 * nb + t - 8 : -1;
    if (peel >= 0) q[peel] = (uint16_t)peeled;
}

__device__ inline u64 wave_sum(u64 x) {
#pragma unroll
    for (int off = 32; off; off >>= 1) x += (u64)__shfl_xor((long long)x, off);
    return x;
}

}  // namespace mm
