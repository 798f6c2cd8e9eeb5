// What a sampler over bf16 rows knows of a row once its threshold key is found, shared by sample.hip (mm_sample_rows) and
// spec_sample.hip (mm_spec_sample_rows): a row's parameters as the rule reads them, the kept mass of a token, the uniform number as
// the draw reads it, and the launch sequence that leaves a row's threshold key.  One copy, so that the distribution a draft is
// verified against is the one that is drawn from.  The kernels of the select live in sample.hip.
#pragma once

#include "mx_argmax_key.h"
#include "mx_row_weights.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

// what the select launches hand on, one per row
struct SampleRow {
    u64 above[256];          // level 1: the mass of bin b and every bin above it
    u64 base;                // the mass above the bin being refined
    u64 target;              // top-p: the mass the prefix has to reach
    unsigned need;           // top-k: the tokens the prefix still lacks above the bin being refined
    int bin;                 // the level-1 bin the next level-2 sweep refines; -1: the threshold is final
    int for_p;               // that sweep is top-p's (else top-k's)
    unsigned kt;             // the threshold key: a token is kept when its key is >= kt (and its weight >= min_p)
};
static_assert(sizeof(SampleRow) % 8 == 0, "the arrays behind the row states hold 64-bit words");

struct SampleParams {
    const uint16_t *logits;
    long long ld;
    int vocab;
    const int *out;          // the argmax of every row, written by argmax_rows before any kernel that reads this
    const float *temperature, *top_p, *min_p;
    const int *top_k;
    const int *cand;         // null, or per row: a value outside [0, vocab) = the row is not looked at (its `out` entry may be anything)
};

// the row is left alone: mm_spec_sample_rows' draft rows without a candidate
__device__ inline bool skipped(const SampleParams &a, int row) { return a.cand && !in_vocab(a.cand[row], a.vocab); }

// a row's parameters as the rule reads them
struct RowRule {
    float m, c, p, q;        // the maximum, log2e / T, top-p (0 for p <= 0), min-p
    int k;
    bool greedy, has_k, has_p, has_q;
};

__device__ inline RowRule row_rule(const SampleParams &a, int row) {
    RowRule r;
    const unsigned mbits = a.logits[(long long)row * a.ld + a.out[row]], mkey = argmax_key(mbits);
    const float T = a.temperature ? a.temperature[row] : 1.0f;
    r.greedy = mkey == 0u || mkey >= KEY_POS_INF || !(T > 0.0f);                    // -inf, +inf, NaN; T <= 0 or NaN
    r.m = __uint_as_float(mbits << 16);
    r.c = LOG2E / T;
    r.k = a.top_k ? a.top_k[row] : 0;
    r.has_k = r.k >= 1 && r.k < a.vocab;
    const float p = a.top_p ? a.top_p[row] : 1.0f;
    r.has_p = p < 1.0f;                                                              // NaN: off
    r.p = p > 0.0f ? p : 0.0f;
    r.q = a.min_p ? a.min_p[row] : 0.0f;
    r.has_q = r.q > 0.0f && r.q <= 1.0f;
    return r;
}

// W of a token if it is kept, else 0
__device__ inline u64 kept_mass(unsigned bits, unsigned kt, const RowRule &r) {
    const unsigned key = argmax_key(bits);
    const float w = weight(bits, key, r);
    return key >= kt && (!r.has_q || w >= r.q) ? fixed(w) : 0ull;
}

// a uniform number as the draws read it: NaN -> 0, else clamped to [0, 1 - 2^-24]
__device__ inline float clamp_u(float u) { return u > 0.0f ? fminf(u, 1.0f - 0x1p-24f) : 0.0f; }

// mm_sample_rows' place in a kept mass Z >= 2^43 (the maximum is kept): < Z, so the prefix passes it inside the row
__device__ inline u64 sample_want(float u, u64 Z) { return min((u64)((double)u * (double)Z), Z - 1); }

// one matrix of a select: its parameters, its row states and its histograms (rows * parts * 256 entries each)
struct SelectSide {
    SampleParams a;
    SampleRow *state;
    u64 *hist_mass;
    unsigned *hist_cnt;
};

// the select on `rows` rows of `parts` parts: hist / finish x 3 (sample.hip), over one matrix or -- second not null -- over two of one
// shape in the same six launches.  Afterwards state[row].kt is the threshold key of every row that is neither skipped nor greedy.
// a.out holds the rows' argmax
hipError_t launch_sample_select(const SelectSide &first, const SelectSide *second, int rows, int parts, hipStream_t stream);

}  // namespace mm
