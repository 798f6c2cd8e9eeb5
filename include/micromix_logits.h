/*
 * micromix_logits.h -- what a serving request does to the logits before a token is picked, on the device: repetition, frequency and
 * presence penalties over a token history, a logit bias list (logit_bias, bad words, EOS before min_tokens) and the allowed-token
 * bitmask of grammar-constrained decoding (xgrammar's format: int32 words, bit i & 31 of word i >> 5 set = token i allowed).
 * mm_process_logits -> mm_sample_rows / mm_argmax_rows / mm_logprob_rows closes a decode step with no arithmetic on the logits elsewhere.
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The
 * status codes are micromix_hip.h's.  micromix_amd/paged.py (process_logits) is the Python side.
 *
 * Every parameter is a DEVICE array with an entry (or a row of entries) per row, read by the kernel only: one captured graph serves
 * any mix of requests rewritten in place.  Nothing is read on the host, nothing is allocated, there is no workspace, and a call is one
 * launch: capture-safe.
 * The rule, for row r with logits l_i (i < vocab); fl32() is the correctly rounded IEEE fp32 result, subnormals kept, and no two
 * operations are contracted into an fma:
 *   History.  s = row_seq ? row_seq[r] : r; s outside [0, n_seq), or null tokens, is an empty history.  P = clamp(prompt_len[r], 0,
 *     ld_tok), N = clamp(total_len[r], P, ld_tok).  The prompt is tokens[s][0 .. P), the output tokens[s][P .. N); ids outside
 *     [0, vocab) (padding such as -1) are ignored.  The lengths belong to the ROW and the buffer to the SEQUENCE: n samples of one
 *     prompt share a buffer, and the rows of a chain draft read one buffer that holds the draft under total_len = base + i + 1.
 *     seen_i: i occurs in [0, N).  c_i: the number of occurrences of i in [P, N), exact (a 32-bit integer count).
 *   With x = (float)l_i, in this order:
 *   1 Repetition.  seen_i and t = repetition_penalty[r] finite and > 0: x = x < 0 ? fl32(x * t) : fl32(x / t)
 *     (HF's RepetitionPenaltyLogitsProcessor over prompt and output).  A null array, t <= 0, inf and NaN: off.
 *   2 Frequency, then presence.  c_i > 0: x = fl32(x - fl32(a_f * (float)c_i)), then x = fl32(x - a_p), a_f = frequency_penalty[r],
 *     a_p = presence_penalty[r] (vLLM's / OpenAI's rule over the output tokens only).  A null array and a NaN: that step off.
 *   3 Bias.  Among the entries j < n_bias with bias_idx[r][j] == i the HIGHEST j wins (an integer rule: the order in which entries
 *     are visited does not matter): x = fl32(x + bias_val[r][j]).  Ids outside [0, vocab) are ignored; +-inf are legal values.
 *   4 Mask.  Bit i & 31 of allowed_mask[r][i >> 5] clear: x = -inf.  Bits at and beyond vocab are not read as tokens.
 *   5 Output.  out[r][i] = bf16 of x, round to nearest even, every NaN written as 0x7FC0.
 *   Columns >= vocab of out are never written, nothing outside the rows of logits is read.  With every optional input null the call is
 *   a copy, up to the NaN of 5.  The counts are integer atomics in on-chip memory and every fp32 operation belongs to one column, so the
 *   result is a function of the inputs alone: the same bits on every run, and a numpy float32 program is the exact oracle
 *   (tests/logits_oracle.py).
 *
 * logits and out: 2-byte aligned, ld_in / ld_out (elements between rows) >= vocab, independent of each other (a slice of a padded
 * lm_head output into a fresh tensor).  out == logits with ld_out == ld_in is the in-place form; any other overlap of the two spans
 * of (rows - 1) * ld + vocab elements is refused, decided from the addresses on the host.  16-byte accesses are used where a row's
 * source and destination are congruent mod 16 and element stores otherwise, with the same bits either way.
 * Limits: vocab <= 1048576 (2^20) and rows <= 65535, as mm_argmax_rows; ld_tok <= 16777216 (2^24), so (float)c_i is exact;
 * n_bias <= 1048576 (2^20).
 *
 * Statuses, all without device work.  MM_ERR_BAD_ARG: rows < 0, vocab < 1, ld_in < vocab, ld_out < vocab, n_bias < 0; tokens with
 * n_seq < 1 or ld_tok < 1; ld_mask < ceil(vocab / 32) with a mask; and, with rows > 0: null logits or out, an odd address of either,
 * partial overlap of the two, tokens without both lengths, a length or row_seq or a penalty array without tokens, exactly one of
 * bias_idx / bias_val, n_bias > 0 with null arrays (or arrays with n_bias == 0), any int32 / float array that is not 4-byte aligned.
 * MM_ERR_UNSUPPORTED: beyond a limit above, for arguments that are not refused: MM_ERR_BAD_ARG comes first.  rows == 0: MM_OK.
 */
#ifndef MICROMIX_LOGITS_H
#define MICROMIX_LOGITS_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int mm_process_logits(const void *logits_bf16, int rows, int vocab, long long ld_in /* elements between rows, >= vocab */,
                      void *out_bf16, long long ld_out /* >= vocab */,
                      const int32_t *tokens /* [n_seq, ld_tok] token history, or null */, long long ld_tok, int n_seq,
                      const int32_t *row_seq /* [rows] or null: row r reads sequence r */,
                      const int32_t *prompt_len, const int32_t *total_len /* [rows]; required iff tokens */,
                      const float *repetition_penalty, const float *frequency_penalty /* [rows] each, or null: off */,
                      const float *presence_penalty,
                      const int32_t *bias_idx, const float *bias_val /* [rows, n_bias] each, or both null */, int n_bias,
                      const int32_t *allowed_mask /* [rows, ld_mask] words, or null */, long long ld_mask /* >= ceil(vocab / 32) */,
                      mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
