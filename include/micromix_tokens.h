/*
 * micromix_tokens.h -- the token half of a decode step on the device: commit the tokens a verified step generated into the history,
 * with stop conditions (mm_token_step), and draft the next chain by prompt lookup, the longest n-gram of that same history that
 * repeats its end (mm_ngram_draft).  With mm_process_logits -> mm_argmax_rows / mm_sample_rows / mm_spec_sample_rows ->
 * mm_verify_greedy -> mm_kv_step the host has nothing left to do between two steps: one captured graph generates several tokens per
 * sequence per replay, and the drafter needs no model (mm_spec_sample_rows' one-hot form for temperature > 0).
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The status
 * codes are micromix_hip.h's.  micromix_amd/paged.py (token_step, ngram_draft, ngram_draft_workspace_bytes) is the Python side.
 *
 * Every parameter that can differ between requests is a per-sequence DEVICE array, read by the kernels only.  Nothing is read on the
 * host and nothing is allocated: capture-safe.  There is no float arithmetic and no atomic: the outputs are a function of the inputs
 * alone, and a program over Python lists is the exact oracle (tests/token_oracle.py).
 *
 * The state, owned by the caller, in the layout mm_process_logits reads: tokens int32 [batch, ld_tok] (sequence b of the step is row
 * b), total_len[batch], finished[batch] (MM_TOKENS_RUNNING, MM_TOKENS_STOPPED: a stop token was committed, MM_TOKENS_LENGTH: the
 * length limit was reached).  The invariant the caller establishes and the steps keep: for a running sequence with total_len[b] = N
 * >= 1, tokens[b][N - 1] is the token picked after the last one in the KV cache -- the bonus, root_tok[b] of the next step.
 *
 * mm_token_step commits one verified step.  result[b * result_stride ..] is mm_verify_greedy's row (k, the bonus, the path),
 * target_tok[num_tokens] the array that went into mm_verify_greedy, qo_indptr[batch + 1] clamped to [0, num_tokens] as there,
 * root_tok[batch] that step's roots, max_total[batch] each sequence's length limit, stop_tok[batch, n_stop] its stop tokens (entries
 * < 0 are unused; may be null with n_stop == 0), kv_state (may be null) mm_kv_step's state.  The rule, for sequence b with
 * n = qo_indptr[b + 1] - qo_indptr[b] and k = result[b * result_stride]:
 *   0 kv_state given and kv_state[0] != 0: THE WHOLE CALL WRITES NOTHING, emitted included -- the sticky failure of mm_kv_step.  The
 *     call belongs after mm_verify_greedy and BEFORE this step's mm_kv_step: a step whose announce fails still commits its own
 *     verified tokens, and every later step of the graph commits none.
 *   1 The sequence is left entirely alone (emitted[b] = 0) when finished[b] != 0; when n == 0, n > 64 or root_tok[b] < 0 (a prompt
 *     chunk: prefill bookkeeping stays on the host); when k == 0; and, since all of this is device data, when the row is not one
 *     mm_verify_greedy writes for a draft (k outside [0, n], a path entry outside [0, n)) or total_len[b] < 0.
 *   2 Otherwise the step generated g_i = target_tok[qo_indptr[b] + path[i]], i < k (the last is the bonus, result[1]).
 *     limit = min(max_total[b], ld_tok); cap = max(0, limit - total_len[b]); c = min(k, cap); j = the first i < c with g_i in the
 *     stop set.  With j: m = j + 1, finished[b] = MM_TOKENS_STOPPED.  Without: m = c, and finished[b] = MM_TOKENS_LENGTH iff
 *     total_len[b] + m >= limit.  tokens[b][total_len[b] + i] = g_i for i < m, then total_len[b] += m; emitted[b] = m (may be null).
 *   No other element of tokens is written.  The cache rows of a finished sequence are whatever mm_kv_step keeps: the host truncates or
 *   frees them after it synchronised.
 *   Shape: one wave per sequence, lane i its g_i; the first stop position is a ballot.
 *
 * mm_ngram_draft proposes the next chain.  next_indptr[batch + 1] is the next step's qo_indptr / append_indptr, clamped to
 * [0, num_tokens]; sequence b gets n_b = next_indptr[b + 1] - next_indptr[b] nodes, 0 <= n_b <= 64 (a sequence outside that range
 * gets no node written).  The rule, with N = clamp(total_len[b], 0, ld_tok) and the history h = tokens[b][0 .. N):
 *   For an end position e in [0, N - 2], m_e is the largest m <= min(max_n, e + 1) with h[e - i] == h[N - 1 - i] for all i < m.
 *   Tokens are compared as plain 32-bit integers: a padding id is a value like any other.  The match is the e that maximises
 *   (m_e, e) lexicographically -- THE LONGEST N-GRAM, AND AMONG EQUALS THE LATEST -- and counts only if m_e >= min_n.
 *   With a match: p = N - 1 - e (>= 1) and d_i = h[e + 1 + (i mod p)], the continuation, repeated periodically where it runs into the
 *   end of the history (a constant history drafts that constant).  Without, or with N < 2: d_i = h[N - 1] (0 when N == 0): any token
 *   is a legal draft, and the count per step stays fixed because num_tokens sizes the captured appends.
 *   Outputs, t0 = next_indptr[b]: draft_tok[t0] = h[N - 1] (0 when N == 0), the root as node 0; draft_tok[t0 + 1 + i] = d_i for
 *   i < n_b - 1; root_tok[b] = h[N - 1], -1 when N == 0; cand_tok[t] = draft_tok[t + 1] inside the sequence and -1 on its last row
 *   (chain_candidates' values; may be null); match_len[b] = m_e, 0 without a match (may be null); row_seq[t0 + i] = b and
 *   row_total_len[t0 + i] = min(N + i, ld_tok) (each may be null): what mm_process_logits takes for the rows of the chain.
 *   The draft is laid into the history's slack so that mm_process_logits can penalise the rows of the chain as its header describes:
 *   tokens[b][N + i] = d_i for i < n_b - 1 and N + i < ld_tok.  Those slots lie past total_len, are uncommitted, and are overwritten
 *   by the next mm_token_step.  Finished sequences are drafted like any other: harmless work that keeps the shapes fixed.
 *   Nothing at or past N + n_b - 1 of a row is written, nothing at or past N is read.
 *   Shape: grid (parts, batch), parts = ceil(ld_tok / MM_NGRAM_CHUNK) from the host value ld_tok; N is device data, so a part that
 *   holds no end position retires at once.  A workgroup stages its part's end positions and a halo of max_n - 1 tokens in front in
 *   on-chip memory (16-byte loads between the peeled elements: a row start is only 4-byte aligned), every lane filters on
 *   h[e] == h[N - 1] and extends backwards only on a hit; the best (m_e, e) is ONE INTEGER KEY, m << 24 | e, reduced by wave shuffles
 *   and a few words of on-chip memory and written to workspace[b][part]; a second launch of one wave per sequence takes the largest
 *   key and writes the outputs.  With one part (ld_tok <= MM_NGRAM_CHUNK) the call is a single launch and needs no workspace.
 *   workspace: mm_ngram_draft_workspace_bytes(batch, ld_tok) bytes (0 for refused arguments and for one part), 4-byte aligned, no
 *   initialisation needed: every word read was written by the same call.
 *
 * Limits: ld_tok <= MM_TOKENS_MAX_LD = 2^24 (e fits under m in the key), batch <= MM_TOKENS_MAX_BATCH = 65535 (a grid dimension),
 * 1 <= min_n <= max_n <= MM_NGRAM_MAX_N = 16, n_stop <= MM_TOKENS_MAX_STOP = 64, at most 64 nodes per sequence as in mm_verify_greedy.
 *
 * Statuses, all without device work.  MM_ERR_BAD_ARG: batch < 0, ld_tok < 1, num_tokens < 0; mm_token_step: result_stride <
 * MM_VERIFY_STRIDE (the path is read), n_stop < 0, stop_tok null with n_stop > 0 or given with n_stop == 0; mm_ngram_draft:
 * min_n < 1 or max_n < min_n; and, with batch > 0: null tokens, total_len or indptr; mm_token_step: null finished, result, root_tok or max_total, null target_tok with
 * num_tokens > 0; mm_ngram_draft: null root_tok, null draft_tok with num_tokens > 0, a workspace that is needed and null or too
 * small; any array that is not 4-byte aligned.  MM_ERR_UNSUPPORTED, for arguments the lines above do not refuse: beyond a limit.
 * batch == 0: MM_OK.
 */
#ifndef MICROMIX_TOKENS_H
#define MICROMIX_TOKENS_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MM_NGRAM_MAX_N 16
#define MM_NGRAM_CHUNK 8192           /* end positions of a history that one workgroup searches */
#define MM_TOKENS_MAX_LD (1 << 24)
#define MM_TOKENS_MAX_BATCH 65535
#define MM_TOKENS_MAX_STOP 64
#define MM_TOKENS_RUNNING 0
#define MM_TOKENS_STOPPED 1
#define MM_TOKENS_LENGTH 2

int mm_token_step(int32_t *tokens /* [batch, ld_tok] */, long long ld_tok, int batch, int32_t *total_len /* [batch] */,
                  int32_t *finished /* [batch] */, const int32_t *result /* result[b * result_stride ..] */, int result_stride,
                  const int32_t *target_tok /* [num_tokens] */, int num_tokens, const int32_t *qo_indptr /* [batch + 1] */,
                  const int32_t *root_tok /* [batch] */, const int32_t *max_total /* [batch] */,
                  const int32_t *stop_tok /* [batch, n_stop] or null */, int n_stop,
                  const int32_t *kv_state /* mm_kv_step's state, or null */, int32_t *emitted /* [batch] or null */, mm_stream_t stream);
size_t mm_ngram_draft_workspace_bytes(int batch, long long ld_tok);
int mm_ngram_draft(int32_t *tokens /* [batch, ld_tok] */, long long ld_tok, int batch, const int32_t *total_len /* [batch] */,
                   const int32_t *next_indptr /* [batch + 1] */, int num_tokens, int min_n, int max_n,
                   int32_t *draft_tok /* [num_tokens] */, int32_t *root_tok /* [batch] */, int32_t *cand_tok /* [num_tokens] or null */,
                   int32_t *match_len /* [batch] or null */, int32_t *row_seq /* [num_tokens] or null */,
                   int32_t *row_total_len /* [num_tokens] or null */, void *workspace, size_t workspace_bytes, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
