// The token half of a decode step on the device (mm_token_step, mm_ngram_draft, include/micromix_tokens.h, which states both rules):
// commit the tokens a verified step generated into the per-sequence history under stop conditions, and draft the next chain by prompt
// lookup -- the longest n-gram of the history, at most max_n tokens, that repeats its end, the latest among equals.
//
// The search is the hot path: integer only and memory-bound.  ngram_search_kernel, grid (parts, batch): a workgroup owns MM_NGRAM_CHUNK
// end positions e of one history.  It stages them and the max_n - 1 tokens in front of them in LDS -- 16-byte loads between the (up to
// 3) elements it peels in front of the first 16-byte boundary and behind the last, since a row start is only 4-byte aligned -- holds
// the suffix h[N - 1 - i] in 16 more words, and every lane filters its positions on h[e] == h[N - 1], extending backwards only on a hit.
// A match is ONE INTEGER, m << 24 | e: the larger word is the longer match, then the later one.  max over integers is associative and
// commutative, so the answer cannot depend on how a history is divided among lanes, waves and workgroups, nor on who finishes first;
// nothing is accumulated into memory, and every workspace word the second launch reads was written by a workgroup of the same call.
// N is device data: a part without end positions writes key 0 (no match) and retires.  ngram_finish_kernel, one wave per sequence, takes
// the largest key and writes the outputs, lane i node i; with one part the search kernel's first wave does that itself.
// token_step_kernel: one wave per sequence, lane i its generated token i, the first stop position a ballot.
#include "../../include/micromix_tokens.h"
#include "mx_argmax_key.h"
#include "mx_kernels.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

constexpr int NG_THREADS = 256, NG_HALO = MM_NGRAM_MAX_N, NG_PER_LANE = MM_NGRAM_CHUNK / NG_THREADS;
constexpr int NG_VECS = ((MM_NGRAM_CHUNK + NG_HALO) / 4 + NG_THREADS - 1) / NG_THREADS;       // 16-byte vectors per lane, at most
static_assert(NG_PER_LANE * NG_THREADS == MM_NGRAM_CHUNK && NG_HALO >= MM_NGRAM_MAX_N - 1, "a part is a whole number of positions per lane");
static_assert(MM_TOKENS_MAX_LD == 1 << 24 && MM_NGRAM_MAX_N < 128, "the key is m << 24 | e in 32 bits");

__device__ inline int clamp_int(long long x, long long lo, long long hi) { return (int)(x < lo ? lo : x > hi ? hi : x); }

// the outputs of sequence b from its best key, by one wave: lane i writes node i
__device__ inline void ngram_outputs(const NgramDraft &s, int b, unsigned key, int lane) {
    int *h = s.tokens + (long long)b * s.ld_tok;
    const int N = clamp_int(s.total_len[b], 0, s.ld_tok);
    const int m = (int)(key >> 24), e = (int)(key & 0xFFFFFFu);
    const bool hit = N >= 2 && m >= s.min_n;                   // key 0, a history without a position that ends like it, has m = 0 < min_n
    const int root = N ? h[N - 1] : 0;
    const int t0 = clamp_int(s.next_indptr[b], 0, s.T), n = clamp_int(s.next_indptr[b + 1], 0, s.T) - t0;
    if (lane == 0) {
        s.root_tok[b] = N ? root : -1;
        if (s.match_len) s.match_len[b] = hit ? m : 0;
    }
    if (n < 1 || n > 64) return;
    int tok = root;                                            // node 0 is the root; node i >= 1 is d_{i - 1}
    if (hit && lane >= 1) tok = h[e + 1 + (lane - 1) % (N - 1 - e)];       // <= h[N - 1]: the continuation, periodic in p = N - 1 - e
    const int next = __shfl_down(tok, 1);
    if (lane < n) {
        s.draft_tok[t0 + lane] = tok;
        if (s.cand_tok) s.cand_tok[t0 + lane] = lane < n - 1 ? next : -1;
        if (s.row_seq) s.row_seq[t0 + lane] = b;
        if (s.row_total_len) s.row_total_len[t0 + lane] = (int)min((long long)N + lane, s.ld_tok);
        if (lane >= 1 && (long long)N + lane - 1 < s.ld_tok) h[N + lane - 1] = tok;           // the slack: past total_len, uncommitted
    }
}

__global__ __launch_bounds__(NG_THREADS) void ngram_search_kernel(const NgramDraft s) {
    __shared__ int s_h[NG_HALO + MM_NGRAM_CHUNK];              // s_h[i] = h[lo - NG_HALO + i]
    __shared__ int s_suf[MM_NGRAM_MAX_N];                      // s_suf[i] = h[N - 1 - i]
    __shared__ unsigned s_best[NG_THREADS / 64];
    const int t = threadIdx.x, b = blockIdx.y, lo = blockIdx.x * MM_NGRAM_CHUNK;
    const int *h = s.tokens + (long long)b * s.ld_tok;
    const int N = clamp_int(s.total_len[b], 0, s.ld_tok);
    const int hi = min(lo + MM_NGRAM_CHUNK, N - 1);            // this part's end positions are [lo, hi): e <= N - 2
    unsigned best = 0;
    if (hi > lo) {                                             // uniform over the workgroup
        const int a = max(lo - (s.max_n - 1), 0), len = hi - a;         // the tokens staged: h[a .. hi), nothing at or past N
        const int *p = h + a;
        int *dst = s_h + (a - lo + NG_HALO);
        const int head = min(len, (int)((4u - (unsigned)((uintptr_t)p >> 2)) & 3u));          // elements in front of the first 16-byte boundary
        const int nb = (len - head) >> 2, tail = len - head - 4 * nb;                         // whole vectors; elements behind the last
        const int4 *body = (const int4 *)(p + head);
        int4 x[NG_VECS];
#pragma unroll
        for (int u = 0; u < NG_VECS; ++u) {
            const int v = t + u * NG_THREADS;
            if (v < nb) x[u] = body[v];
        }
        // lanes 0 .. 3 the head, lanes 4 .. 7 the tail, an element each
        const int peel = t < head ? t : (t >= 4 && t - 4 < tail) ? head + 4 * nb + t - 4 : -1;
        if (peel >= 0) dst[peel] = p[peel];
        if (t < s.max_n && t < N) s_suf[t] = h[N - 1 - t];
#pragma unroll
        for (int u = 0; u < NG_VECS; ++u) {
            const int v = t + u * NG_THREADS;
            if (v < nb) {
                int *d = dst + head + 4 * v;
                d[0] = x[u].x, d[1] = x[u].y, d[2] = x[u].z, d[3] = x[u].w;
            }
        }
        __syncthreads();
        const int last = s_suf[0], max_n = s.max_n;
        for (int j = 0; j < NG_PER_LANE; ++j) {
            const int r = t + j * NG_THREADS, e = lo + r;
            if (e < hi && s_h[NG_HALO + r] == last) {
                const int lim = min(max_n, e + 1);             // cut short by the start of the history; m <= e <= N - 2 keeps s_suf[m] inside
                int m = 1;
                while (m < lim && s_h[NG_HALO + r - m] == s_suf[m]) ++m;
                best = max(best, (unsigned)m << 24 | (unsigned)e);
            }
        }
        best = wave_max(best);
        if ((t & 63) == 0) s_best[t >> 6] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NG_THREADS / 64; ++w) best = max(best, s_best[w]);
    }
    if (gridDim.x == 1) {
        if (t < 64) ngram_outputs(s, b, best, t);
    } else if (t == 0) {
        s.ws[(long long)b * gridDim.x + blockIdx.x] = best;
    }
}

// one wave per sequence: the largest of its `parts` keys (at most 2^24 / MM_NGRAM_CHUNK of them), then the outputs
__global__ __launch_bounds__(64) void ngram_finish_kernel(const NgramDraft s, int parts) {
    const int b = blockIdx.x;
    unsigned best = 0;
    for (int c = threadIdx.x; c < parts; c += 64) best = max(best, s.ws[(long long)b * parts + c]);
    ngram_outputs(s, b, wave_max(best), threadIdx.x);
}

int ngram_parts(long long ld_tok) { return (int)((ld_tok + MM_NGRAM_CHUNK - 1) / MM_NGRAM_CHUNK); }

size_t ngram_workspace_bytes(int batch, long long ld_tok) {
    const int parts = ngram_parts(ld_tok);
    return parts > 1 ? (size_t)batch * parts * sizeof(unsigned) : 0;
}

hipError_t launch_ngram_draft(const NgramDraft &s, hipStream_t stream) {
    const int parts = ngram_parts(s.ld_tok);
    ngram_search_kernel<<<dim3(parts, s.B), NG_THREADS, 0, stream>>>(s);
    if (parts > 1) ngram_finish_kernel<<<s.B, 64, 0, stream>>>(s, parts);
    return hipGetLastError();
}

// ---- the commit -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void token_step_kernel(const TokenStep s) {
    if (s.kv_state && s.kv_state[0] != 0) return;              // an earlier mm_kv_step failed: sticky, the whole call writes nothing
    const int b = blockIdx.x, lane = threadIdx.x;
    const int q0 = clamp_int(s.qo_indptr[b], 0, s.T), n = clamp_int(s.qo_indptr[b + 1], 0, s.T) - q0;
    const int *row = s.result + (long long)b * s.result_stride;
    const int k = row[0], N = s.total_len[b];
    bool live = s.finished[b] == MM_TOKENS_RUNNING && n >= 1 && n <= 64 && s.root_tok[b] >= 0 && k >= 1 && k <= n && N >= 0;
    int g = -1, m = 0;
    bool inside = true;
    if (live && lane < k) {
        const int node = row[2 + lane];
        inside = node >= 0 && node < n;
        if (inside) g = s.target_tok[q0 + node];
    }
    live = live && __all(inside);                              // a row mm_verify_greedy does not write for a draft commits nothing
    if (live) {
        const long long limit = min((long long)s.max_total[b], s.ld_tok);
        const int c = (int)min((long long)k, max(0LL, limit - N));
        bool stop = false;
        if (lane < c)
            for (int i = 0; i < s.n_stop; ++i) {
                const int st = s.stop_tok[(long long)b * s.n_stop + i];
                stop |= st >= 0 && st == g;
            }
        const unsigned long long stops = __ballot(stop);
        m = stops ? __ffsll(stops) : c;                        // through the first stop token, or all the cap admits
        if (lane < m) s.tokens[(long long)b * s.ld_tok + N + lane] = g;      // N + m <= limit <= ld_tok
        if (lane == 0) {
            s.total_len[b] = N + m;
            if (stops) s.finished[b] = MM_TOKENS_STOPPED;
            else if (N + m >= limit) s.finished[b] = MM_TOKENS_LENGTH;
        }
    }
    if (lane == 0 && s.emitted) s.emitted[b] = m;
}

hipError_t launch_token_step(const TokenStep &s, hipStream_t stream) {
    token_step_kernel<<<s.B, 64, 0, stream>>>(s);
    return hipGetLastError();
}

}  // namespace mm
