/*
 * micromix_logprob.h -- token log-probabilities on the device: for every row of bf16 logits the log-probability and the rank of a
 * target token, the row's log-sum-exp, and its top_n tokens with their log-probabilities.  What a perplexity evaluation
 * (CrossEntropyLoss), lm-eval style scoring (log-probability, is_greedy) and a sampling API (logprobs, top_logprobs) ask of logits.
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The
 * status codes are micromix_hip.h's.  micromix_amd/paged.py (logprob_rows, cross_entropy) is the Python side.
 *
 * target, temperature and every output are DEVICE arrays, read and written by the kernels only: one captured graph serves any
 * targets and temperatures rewritten in place.  Nothing is read on the host, nothing is allocated: capture-safe.
 * The rule, for row r with logits l_i (i < vocab), key() mm_argmax_rows' 16-bit key (any NaN above +inf, +0 == -0):
 *   1 Temperature.  T' = temperature[r] if it is > 0, else 1.  A null array, T <= 0 and a NaN all give 1: the unscaled distribution
 *     is reported for a greedy request.
 *   2 Maximum and weights.  m = the row maximum in mm_argmax_rows' order.  w_i and W_i are mm_sample_rows' (the same device
 *     functions): c = fl32(fl32(log2 e) / T'), w_i = V_EXP_F32(fl32(fl32(l_i - m) * c)), l_i == m gives 1 and -inf gives 0;
 *     W_i = trunc(w_i * 2^43).  S = sum_i W_i, a 64-bit integer >= 2^43 whose value does not depend on the order of the sum.
 *   3 Values.  L = ln((double)S * 2^-43) in fp64 (the product is exact, so a row with one finite token has L = 0 exactly).
 *     lse[r] = fl32((double)m / T' + L).  The log-probability of token i is fl32(((double)l_i - (double)m) / (double)T' - L); a -inf
 *     logit in a finite row gives -inf.  The only approximation is inside S: this is the logarithm of the unfiltered distribution
 *     mm_sample_rows draws from, same W, same S.  tests/logprob_oracle.py derives the bound from tests/sample_oracle.py's.
 *   4 Degenerate rows.  m -inf, +inf or NaN: lse, logprob and every top_logprob are NaN (torch.log_softmax's answer); the integer
 *     outputs are unaffected.
 *   5 Rank.  rank[r] = #{i : key(l_i) > key(l_target)}, exact; 0 means the target is a greedy token (lm-eval's is_greedy).
 *   6 Ignored targets.  target[r] < 0 or >= vocab: logprob[r] = 0.0f, rank[r] = -1, nothing is read through the index
 *     (CrossEntropyLoss's ignore_index).
 *   7 Top-n.  top_idx[r][0 .. top_n) are the largest tokens of the row by descending key, then ascending index, so entry 0 is bit
 *     for bit mm_argmax_rows' answer; top_logprob holds their log-probabilities by 3 (4 for a degenerate row).  Entries beyond vocab
 *     hold -1 and -inf.
 *   Every element of every non-null output is written by every call.  The result is a function of the inputs alone: the same bits on
 *   every run and however a row is divided; there are no float atomics.
 *
 * logits, ld, the limits on vocab and rows and the split into parts of MM_ARGMAX_CHUNK columns: as mm_argmax_rows (2-byte alignment,
 * any ld >= vocab, nothing read outside the rows).  top_n is at most 32.  workspace: mm_logprob_rows_workspace_bytes(rows, vocab, top_n)
 * bytes (0 for arguments mm_logprob_rows refuses), 8-byte aligned, always needed, no initialisation needed: every word read was
 * written by the same call.  It holds at most 24 + 8 top_n bytes per part of every row and 8 bytes per row.
 * Launches: mm_argmax_rows' one or two, one sweep on a grid (parts, rows), one finish of a workgroup per row.
 *
 * Statuses, all without device work.  MM_ERR_BAD_ARG: rows < 0, vocab < 1, ld < vocab, top_n outside 0 .. 32; and, with rows > 0,
 * null logits, an odd logits address, any other array that is not 4-byte aligned, a target without logprob or logprob without a
 * target, rank without a target, top_n > 0 with a null top_idx or top_logprob, no output requested at all (no target, no lse,
 * top_n == 0), a workspace that is null, too small or not 8-byte aligned.  MM_ERR_UNSUPPORTED: vocab > MM_ARGMAX_MAX_VOCAB or
 * rows > MM_ARGMAX_MAX_ROWS.  rows == 0: MM_OK.
 */
#ifndef MICROMIX_LOGPROB_H
#define MICROMIX_LOGPROB_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

size_t mm_logprob_rows_workspace_bytes(int rows, int vocab, int top_n);
int mm_logprob_rows(const void *logits_bf16, int rows, int vocab, long long ld /* elements between rows, >= vocab */,
                    const int32_t *target /* [rows] or null */, const float *temperature /* [rows] or null: 1.0 */,
                    float *logprob /* [rows]; null iff target is null */, int32_t *rank /* [rows] or null */,
                    float *lse /* [rows] or null */, int top_n /* 0 .. 32 */,
                    int32_t *top_idx /* [rows, top_n] */, float *top_logprob /* [rows, top_n] */,
                    void *workspace, size_t workspace_bytes, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
