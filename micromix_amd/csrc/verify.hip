// Greedy verification of tree and chain drafts (mm_argmax_rows, mm_verify_greedy, include/micromix_hip.h): the vocabulary argmax of the
// verified rows, then the walk that picks the accepted path and writes the move table mm_kv_move_rows takes (kv_move.hip).
//
// The argmax order, on the bf16 bits alone: every value gets a 16-bit key that grows with it -- -inf 0x0000, the negative numbers up to
// -0 == +0 at 0x7F80, the positive ones up to +inf 0xFF00, and every NaN, of either sign, 0xFF01 -- and the answer is the lowest index
// among the largest keys.  That is a total order on (key, index), so max is associative and commutative over it: the answer cannot depend
// on how a row is divided among lanes, waves and workgroups, nor on who finishes first.  Nothing is accumulated into memory; every partial
// a finishing workgroup reads was written by a workgroup of the same call, so the workspace needs no initialisation.  The key and the
// wave reductions live in mx_argmax_key.h, which sample.hip shares.
//
// One workgroup reduces MM_ARGMAX_CHUNK columns of one row: it peels the (up to 7) elements in front of the first 16-byte boundary and
// behind the last, holds the 16-byte vectors between them in registers (4 per lane), finds the largest key without tracking an index
// (packed 16-bit min / max / sub: 4 operations an element), and only then looks for the lowest column that holds that key -- in the few
// lanes whose own maximum equals it.
#include "../../include/micromix_hip.h"
#include "mx_argmax_key.h"
#include "mx_kernels.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

constexpr int ARG_THREADS = 256, ARG_VECS = MM_ARGMAX_CHUNK / 8 / ARG_THREADS;      // lanes per workgroup; 16-byte vectors per lane
static_assert(ARG_VECS * ARG_THREADS * 8 == MM_ARGMAX_CHUNK && MM_ARGMAX_CHUNK <= 65536, "a part is a whole number of vectors per lane");

// the second matrix of a launch with gridDim.z == 2
struct ArgmaxSecond {
    const uint16_t *logits;
    long long ld;
    int *out;
    unsigned long long *partial;
    const int *cand;
};

// a partial: the key above the bitwise complement of the column, so that the larger word is the larger key, then the lower column
__device__ inline unsigned long long argmax_pack(unsigned key, unsigned col) { return ((unsigned long long)key << 32) | (0xFFFFFFFFu - col); }

// grid (parts, rows) or (parts, rows, 2).  One part: out[row] is written; several: partial[row * parts + part].  z = 1 is a second
// matrix with its own row distance and outputs (mm_spec_sample_rows' draft rows); a row of it whose cand entry names no token is
// not read and gets no answer
__global__ __launch_bounds__(ARG_THREADS) void argmax_rows_kernel(const uint16_t *__restrict__ logits, int vocab, long long ld,
                                                                  int *__restrict__ out, unsigned long long *__restrict__ partial,
                                                                  ArgmaxSecond second) {
    __shared__ unsigned s_key[ARG_THREADS / 64], s_col[ARG_THREADS / 64];
    const int t = threadIdx.x, row = blockIdx.y, lo = blockIdx.x * MM_ARGMAX_CHUNK;
    if (blockIdx.z) {
        if (!in_vocab(second.cand[row], vocab)) return;
        logits = second.logits, ld = second.ld, out = second.out, partial = second.partial;
    }
    const int len = min(vocab - lo, MM_ARGMAX_CHUNK);                               // >= 1: the grid holds ceil(vocab / CHUNK) parts
    const uint16_t *p = logits + (long long)row * ld + lo;
    const int head = min(len, (int)((8u - (unsigned)((uintptr_t)p >> 1)) & 7u));    // elements in front of the first 16-byte boundary
    const int nb = (len - head) >> 3, tail = len - head - 8 * nb;                   // whole vectors; elements behind the last
    const us8 *body = (const us8 *)(p + head);

    us8 k[ARG_VECS];
#pragma unroll
    for (int u = 0; u < ARG_VECS; ++u) {
        const int v = t + u * ARG_THREADS;
        k[u] = v < nb ? body[v] : (us8)BF16_NEG_INF;
    }
    // lanes 0 .. 7 the head, lanes 8 .. 15 the tail, an element each
    const int peel = t < head ? t : (t >= 8 && t - 8 < tail) ? head + 8 * nb + t - 8 : -1;
    const unsigned peel_key = peel >= 0 ? argmax_key(p[peel]) : 0u;
#pragma unroll
    for (int u = 0; u < ARG_VECS; ++u) k[u] = argmax_keys(k[u]);

    us8 m8 = k[0];
#pragma unroll
    for (int u = 1; u < ARG_VECS; ++u) m8 = __builtin_elementwise_max(m8, k[u]);
    unsigned mine = peel_key;
#pragma unroll
    for (int e = 0; e < 8; ++e) mine = max(mine, (unsigned)m8[e]);
    const unsigned wave_key = wave_max(mine);
    if ((t & 63) == 0) s_key[t >> 6] = wave_key;
    __syncthreads();
    unsigned best = s_key[0];
#pragma unroll
    for (int w = 1; w < ARG_THREADS / 64; ++w) best = max(best, s_key[w]);

    // the lowest column of this part that holds `best`; the filled vectors (v >= nb) and the lanes without a peeled element hold key 0,
    // which is -inf's, so they are kept out by their indices
    unsigned col = 0xFFFFFFFFu;
    if (mine == best) {
#pragma unroll
        for (int u = ARG_VECS - 1; u >= 0; --u) {
            const int v = t + u * ARG_THREADS;
            if (v < nb) {
#pragma unroll
                for (int e = 7; e >= 0; --e)
                    if (k[u][e] == best) col = (unsigned)(head + 8 * v + e);
            }
        }
        if (peel >= 0 && peel_key == best) col = min(col, (unsigned)peel);
    }
    col = wave_min(col);
    if ((t & 63) == 0) s_col[t >> 6] = col;
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < ARG_THREADS / 64; ++w) col = min(col, s_col[w]);
        col += (unsigned)lo;
        if (gridDim.x == 1) out[row] = (int)col;
        else partial[(long long)row * gridDim.x + blockIdx.x] = argmax_pack(best, col);
    }
}

// one wave per row: the largest of its `parts` partials (at most 2^20 / MM_ARGMAX_CHUNK of them).  grid rows or (rows, 2), the second
// matrix as above
__global__ __launch_bounds__(64) void argmax_finish_kernel(const unsigned long long *__restrict__ partial, int parts, int *__restrict__ out,
                                                           int vocab, ArgmaxSecond second) {
    const int row = blockIdx.x;
    if (blockIdx.y) {
        if (!in_vocab(second.cand[row], vocab)) return;
        partial = second.partial, out = second.out;
    }
    unsigned long long best = 0;                                                    // below every partial: a column never reaches 2^32 - 1
    for (int c = threadIdx.x; c < parts; c += 64) best = max(best, partial[(long long)row * parts + c]);
#pragma unroll
    for (int off = 32; off; off >>= 1) best = max(best, (unsigned long long)__shfl_xor((long long)best, off));
    if (threadIdx.x == 0) out[row] = (int)(0xFFFFFFFFu - (unsigned)best);
}

int argmax_parts(int vocab) { return (vocab + MM_ARGMAX_CHUNK - 1) / MM_ARGMAX_CHUNK; }

size_t argmax_workspace_bytes(int rows, int vocab) {
    const int parts = argmax_parts(vocab);
    return parts > 1 ? (size_t)rows * parts * sizeof(unsigned long long) : 0;
}

hipError_t launch_argmax_rows(const void *logits, int rows, int vocab, long long ld, int *out, void *ws, hipStream_t stream) {
    const int parts = argmax_parts(vocab);
    argmax_rows_kernel<<<dim3(parts, rows), ARG_THREADS, 0, stream>>>((const uint16_t *)logits, vocab, ld, out, (unsigned long long *)ws, ArgmaxSecond{});
    if (parts > 1) argmax_finish_kernel<<<rows, 64, 0, stream>>>((const unsigned long long *)ws, parts, out, vocab, ArgmaxSecond{});
    return hipGetLastError();
}

hipError_t launch_argmax_rows_pair(const void *logits, long long ld, int *out, void *ws, const void *logits2, long long ld2, int *out2, void *ws2,
                                   const int *cand, int rows, int vocab, hipStream_t stream) {
    const int parts = argmax_parts(vocab);
    const ArgmaxSecond second{(const uint16_t *)logits2, ld2, out2, (unsigned long long *)ws2, cand};
    argmax_rows_kernel<<<dim3(parts, rows, 2), ARG_THREADS, 0, stream>>>((const uint16_t *)logits, vocab, ld, out, (unsigned long long *)ws, second);
    if (parts > 1) argmax_finish_kernel<<<dim3(rows, 2), 64, 0, stream>>>((const unsigned long long *)ws, parts, out, vocab, second);
    return hipGetLastError();
}

// ---- the walk --------------------------------------------------------------------------------------------------------------------
// One wave per sequence, lane i its node i.  A node's parent is the highest bit of its word below its own: the word holds the node's
// ancestors and itself, a parent comes before its children, so every other ancestor is an ancestor of the parent and has a lower index
// still.  Each step is one ballot over "my parent is the node just taken and my token is the one wanted"; its lowest set bit is the
// node taken next.  The node taken has a higher index than the one before, so there are at most n steps.
__global__ __launch_bounds__(64) void verify_greedy_kernel(const int *__restrict__ target_tok, const int *__restrict__ draft_tok,
                                                           const int *__restrict__ root_tok, const unsigned long long *__restrict__ tree_mask,
                                                           const int *__restrict__ qo_indptr, int T, const int *__restrict__ kv_indptr,
                                                           const int *__restrict__ last_page_len, int P, int B, int *__restrict__ result,
                                                           int *__restrict__ move_src, int *__restrict__ move_dst) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int q0 = min(max(qo_indptr[b], 0), T), q1 = min(max(qo_indptr[b + 1], 0), T);
    const int n = max(q1 - q0, 0);
    // rows that belong to no sequence (a qo_indptr that does not start at 0 or end at T) still get their -1
    const int lead = b == 0 ? q0 : 0, trail = b == B - 1 ? max(q0, q1) : T;
    for (int t = lane; t < lead; t += 64) move_src[t] = move_dst[t] = -1;
    for (int t = trail + lane; t < T; t += 64) move_src[t] = move_dst[t] = -1;

    int *res = result + (long long)b * MM_VERIFY_STRIDE;
    const int root = root_tok[b];
    if (n > 64 || root < 0) {                                                       // no draft: a prompt chunk keeps all its tokens
        for (int t = q0 + lane; t < q1; t += 64) move_src[t] = move_dst[t] = -1;
        res[2 + lane] = -1;
        if (lane == 0) {
            res[0] = n;
            res[1] = n > 0 ? target_tok[q1 - 1] : -1;
        }
        return;
    }
    const int np = kv_indptr[b + 1] - kv_indptr[b];
    const int len = np > 0 ? (np - 1) * P + min(max(last_page_len[b], 0), P) : 0;   // as seq_len (mx_paged_kv.h)
    const int base = len - n;
    const bool node = lane < n;
    int parent = lane - 1, draft = -1, target = -1;
    if (node) {
        draft = draft_tok[q0 + lane];
        target = target_tok[q0 + lane];
        if (tree_mask) {
            const unsigned long long below = tree_mask[q0 + lane] & ((1ull << lane) - 1ull);
            parent = below ? 63 - __builtin_clzll(below) : -1;
        }
    }
    int cur = -1, want = root, k = 0, mine = -1;                                    // mine: path[lane]
    while (true) {
        const unsigned long long match = __ballot(node && parent == cur && draft == want);
        if (!match) break;
        cur = __builtin_ctzll(match);
        if (lane == k) mine = cur;
        want = __shfl(target, cur);
        ++k;
    }
    res[2 + lane] = mine;                                                           // -1 from k on
    if (lane == 0) {
        res[0] = k;
        res[1] = want;
    }
    if (node) {
        move_src[q0 + lane] = lane < k ? base + mine : -1;
        move_dst[q0 + lane] = lane < k ? base + lane : -1;
    }
}

hipError_t launch_verify_greedy(const int *target_tok, const int *draft_tok, const int *root_tok, const void *tree_mask, const int *qo_indptr,
                                int T, const int *kv_indptr, const int *last_page_len, int P, int B, int *result, int *move_src,
                                int *move_dst, hipStream_t stream) {
    verify_greedy_kernel<<<B, 64, 0, stream>>>(target_tok, draft_tok, root_tok, (const unsigned long long *)tree_mask, qo_indptr, T, kv_indptr,
                                                last_page_len, P, B, result, move_src, move_dst);
    return hipGetLastError();
}

}  // namespace mm
