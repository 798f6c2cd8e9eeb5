// Logits processing before a token is picked (mm_process_logits, include/micromix_logits.h): repetition, frequency and presence
// penalties over a token history, a bias list and an allowed-token bitmask, one launch, the rule stated in the header.
//
// Grid (parts, rows): a workgroup of 256 lanes owns one part of MM_ARGMAX_CHUNK columns of one row, as in verify.hip, sample.hip and
// logprob.hip, and walks it with mx_row_weights.h's for_each_in_part_at.  What the history and the bias list say about a column is
// gathered in LDS first, a word per column of the part each:
//   seen   every lane sweeps the row's history with coalesced loads; an id inside the part adds 1 (an output token) or sets bit 31 (a
//          prompt token) by an integer LDS atomic.  c_i <= ld_tok <= 2^24 stays below bit 31, so one word holds both
//   slot   the bias list the same way: atomicMax of j + 1, so the highest j wins and 0 means no entry
// Integer atomics commute: the words, and so the output, do not depend on the order in which lanes run.  The sweep is dense -- every
// part reads the whole history -- because a sparse form (visit the columns the history names) would need the parts of a row to agree
// on who writes a column twice named, which is an order; the dense form has no such question and its reads come from L2.
// A lane's vector of 8 columns lies in one mask word or two: both are loaded once and the vector's 8 bits cut out of the pair, so a
// word is read once per 32 columns of a lane's run and no LDS is spent on it.  The fp32 steps of a column are in rule(), under
// `#pragma clang fp contract(off)`: hipcc contracts a * c followed by x - . into one fma by default, which rounds once where the rule
// rounds twice (tests/test_logits_gpu.py plants inputs on which that shows after the bf16 rounding).  Instantiated per (history, bias): a call without them has neither the sweep nor its LDS.
#include "../../include/micromix_logits.h"
#include "mx_argmax_key.h"
#include "mx_kernels.h"
#include "mx_row_weights.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

constexpr unsigned LG_PROMPT = 0x80000000u;                                         // the bit a prompt token sets; the count is below it
static_assert(MM_ARGMAX_CHUNK % 32 == 0, "a part begins at a mask word");

struct LogitsParams {
    const uint16_t *logits;
    uint16_t *out;
    long long ld_in, ld_out;
    int vocab;
    const int *tokens;
    long long ld_tok;
    int n_seq;
    const int *row_seq, *prompt_len, *total_len;
    const float *repetition, *frequency, *presence;
    const int *bias_idx;
    const float *bias_val;
    int n_bias;
    const unsigned *mask;
    long long ld_mask;
};

// a row's penalties as the rule reads them: NaN is off
struct LogitsRule {
    float theta, alpha_f, alpha_p;
    bool repeat;
};

__device__ inline unsigned bf16_rne(float x) {                                      // every NaN 0x7FC0, overflow to inf
    const unsigned u = __float_as_uint(x);
    return x != x ? 0x7FC0u : (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// steps 1 - 3 of the header for one column: `word` its seen word, `bias` the value to add when has_bias.  One rounding per operation:
// the operators are written out under the pragma, which holds for the operations spelled inside this function only.  __fmul_rn and
// __fsub_rn are plain x * y and x - y in this toolchain's headers, compiled under its default contraction, and a * c through them
// came out of the compiler as one v_fma_f32 with the subtraction; the divide is the correctly rounded one (v_div_scale .. v_div_fixup)
__device__ inline float rule(float x, unsigned word, const LogitsRule &r, bool has_bias, float bias) {
#pragma clang fp contract(off)
    if (word != 0u && r.repeat) x = x < 0.0f ? x * r.theta : x / r.theta;
    const unsigned c = word & ~LG_PROMPT;
    if (c != 0u) {
        if (r.alpha_f == r.alpha_f) {
            const float fc = r.alpha_f * (float)c;
            x = x - fc;
        }
        if (r.alpha_p == r.alpha_p) x = x - r.alpha_p;
    }
    if (has_bias) x = x + bias;
    return x;
}

template <bool HIST, bool BIAS>
__global__ __launch_bounds__(SMP_THREADS) void process_logits_kernel(LogitsParams a) {
    const int t = threadIdx.x, row = blockIdx.y, lo = blockIdx.x * MM_ARGMAX_CHUNK;
    const int len = min(a.vocab - lo, MM_ARGMAX_CHUNK);
    unsigned *s_seen = nullptr, *s_slot = nullptr;
    if constexpr (HIST) {
        __shared__ unsigned seen[MM_ARGMAX_CHUNK];
        s_seen = seen;
    }
    if constexpr (BIAS) {
        __shared__ unsigned slot[MM_ARGMAX_CHUNK];
        s_slot = slot;
    }
    if constexpr (HIST || BIAS) {
        for (int i = t; i < MM_ARGMAX_CHUNK; i += SMP_THREADS) {
            if constexpr (HIST) s_seen[i] = 0u;
            if constexpr (BIAS) s_slot[i] = 0u;
        }
    }
    LogitsRule r;
    r.theta = r.alpha_f = r.alpha_p = __builtin_nanf("");
    r.repeat = false;
    if constexpr (HIST) {
        __syncthreads();                                                            // the zeroes, before the first atomic
        const int s = a.row_seq ? a.row_seq[row] : row;
        const int cap = (int)a.ld_tok;                                              // <= 2^24
        const int P = min(max(a.prompt_len[row], 0), cap), N = (unsigned)s < (unsigned)a.n_seq ? min(max(a.total_len[row], P), cap) : 0;
        const int *hist = a.tokens + (long long)((unsigned)s < (unsigned)a.n_seq ? s : 0) * a.ld_tok;
#pragma unroll 4
        for (int at = t; at < N; at += SMP_THREADS) {
            const unsigned rel = (unsigned)hist[at] - (unsigned)lo;                 // a negative id lands far above len
            if (rel < (unsigned)len) {
                if (at >= P) atomicAdd(&s_seen[rel], 1u);
                else atomicOr(&s_seen[rel], LG_PROMPT);
            }
        }
        if (a.repetition) r.theta = a.repetition[row];
        if (a.frequency) r.alpha_f = a.frequency[row];
        if (a.presence) r.alpha_p = a.presence[row];
        r.repeat = r.theta > 0.0f && r.theta < __builtin_inff();
    }
    const int *bidx = nullptr;
    const float *bval = nullptr;
    if constexpr (BIAS) {
        if constexpr (!HIST) __syncthreads();
        bidx = a.bias_idx + (long long)row * a.n_bias;
        bval = a.bias_val + (long long)row * a.n_bias;
#pragma unroll 4
        for (int j = t; j < a.n_bias; j += SMP_THREADS) {
            const unsigned rel = (unsigned)bidx[j] - (unsigned)lo;
            if (rel < (unsigned)len) atomicMax(&s_slot[rel], (unsigned)j + 1u);
        }
    }
    __syncthreads();
    const uint16_t *p = a.logits + (long long)row * a.ld_in + lo;
    // the allowed bits of the lane's vectors: columns c0 .. c0 + 7 of the part are bits (c0 & 31) .. + 7 of the pair of words c0 >> 5
    // and (c0 + 7) >> 5 (one word twice when they do not straddle: the high copy is then not reached).  A whole vector lies inside
    // the row, so both words do
    const bool masked = a.mask != nullptr;
    const unsigned *mrow = masked ? a.mask + (long long)row * a.ld_mask + (lo >> 5) : nullptr;
    unsigned allowed[SMP_VECS];
    if (masked) {
        const int head = part_head(p, len), nb = (len - head) >> 3;
#pragma unroll
        for (int u = 0; u < SMP_VECS; ++u) {
            const int at = t + u * SMP_THREADS, c0 = head + 8 * at;
            allowed[u] = at < nb ? (unsigned)((mrow[c0 >> 5] | (u64)mrow[(c0 + 7) >> 5] << 32) >> (c0 & 31)) & 0xFFu : 0u;
        }
    }
    us8 v[SMP_VECS];
    unsigned peeled = 0u;
    for_each_in_part_at(p, len, t, [&](unsigned bits, int slot, int col) {
        float x = __uint_as_float(bits << 16);
        unsigned word = 0u, j1 = 0u;
        if constexpr (HIST) word = s_seen[col];
        if constexpr (BIAS) j1 = s_slot[col];
        x = rule(x, word, r, j1 != 0u, j1 != 0u ? bval[j1 - 1u] : 0.0f);
        if (masked) {
            const int u = (slot >> 3) & (SMP_VECS - 1);                             // (the peeled column reads its own word)
            const unsigned bit = slot < SMP_RUN ? allowed[u] >> (slot & 7) : mrow[col >> 5] >> (col & 31);
            if (!(bit & 1u)) x = -__builtin_inff();
        }
        const unsigned y = bf16_rne(x);
        if (slot < SMP_RUN) v[(slot >> 3) & (SMP_VECS - 1)][slot & 7] = (unsigned short)y;
        else peeled = y;
    });
    store_part(a.out + (long long)row * a.ld_out + lo, p, len, t, v, peeled);
}

hipError_t launch_process_logits(const void *logits, int rows, int vocab, long long ld_in, void *out, long long ld_out, const int *tokens,
                                 long long ld_tok, int n_seq, const int *row_seq, const int *prompt_len, const int *total_len,
                                 const float *repetition, const float *frequency, const float *presence, const int *bias_idx,
                                 const float *bias_val, int n_bias, const int *mask, long long ld_mask, hipStream_t stream) {
    const LogitsParams a{(const uint16_t *)logits, (uint16_t *)out, ld_in, ld_out, vocab, tokens, ld_tok, n_seq, row_seq, prompt_len,
                         total_len, repetition, frequency, presence, bias_idx, bias_val, n_bias, (const unsigned *)mask, ld_mask};
    const dim3 grid(argmax_parts(vocab), rows);
    const bool hist = tokens != nullptr, bias = n_bias > 0;
    if (hist && bias) process_logits_kernel<true, true><<<grid, SMP_THREADS, 0, stream>>>(a);
    else if (hist) process_logits_kernel<true, false><<<grid, SMP_THREADS, 0, stream>>>(a);
    else if (bias) process_logits_kernel<false, true><<<grid, SMP_THREADS, 0, stream>>>(a);
    else process_logits_kernel<false, false><<<grid, SMP_THREADS, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace mm
