/*
 * micromix_spec.h -- speculative sampling on the device: accept a draft token against its own odds.
 *
 * mm_sample_rows -> mm_verify_greedy keeps a draft token only when the target's independent sample happens to be the same token: the
 * output is distributed as the target model's, but a draft token x drawn from q survives with probability sum_x q(x) p(x).  The
 * speculative-sampling rule (Leviathan et al. 2023; Chen et al. 2023) accepts x with probability min(1, p(x) / q(x)) and on rejection
 * redraws from norm(max(0, p - q)): x survives with probability sum_x min(p(x), q(x)) and the output is still exactly the target's
 * distribution.  mm_spec_sample_rows is that rule as a sampler: its out_idx goes into the unchanged mm_verify_greedy as target_tok, and
 * the walk it performs is then the speculative-sampling algorithm for chain drafts -- the accepted prefix, and as the bonus token the
 * redraw at the first rejection or the plain sample after the leaf.
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The status
 * codes are micromix_hip.h's.  micromix_amd/paged.py (spec_sample_rows, chain_candidates) is the Python side.
 *
 * Scope: chains only.  Every row has at most one candidate.  For a tree draft a node has several children and the residual would have to be
 * updated child after child; that is not done here: mm_sample_rows -> mm_verify_greedy stays the recommendation for trees.
 *
 * Row r of logits is the target's logits after node r; cand_tok[r] is the token the draft proposed for the next position (the draft
 * token of node r's child in a chain: cand_tok[t] = draft_tok[t + 1] inside a sequence, -1 on its last row); row r of draft_logits is
 * the draft model's logits that token was drawn from.  u_accept, u_resample, temperature, top_k, top_p, min_p and cand_tok are DEVICE
 * arrays of `rows` entries, read by the kernels only; the library draws no random numbers.  A null temperature means 1.0, a null filter
 * array means that filter is off; both u arrays are required.  Nothing is read on the host, nothing allocated: capture-safe.
 *
 * The rule, for row r with candidate x = cand_tok[r]:
 *   P_i is mm_sample_rows' kept mass of token i of the target row under (temperature[r], top_k[r], top_p[r], min_p[r]): the integer
 *   W_i = trunc(w_i * 2^43) of a kept token and 0 of any other -- the same code finds the kept set and forms W -- and Z_p = sum_i P_i.
 *   Q_i and Z_q are the same function of the draft row under the SAME per-row parameters: the draft must have been sampled under the
 *   request's parameters.  If it was drawn by mm_sample_rows from these bits, Q is bit for bit the masses it was drawn from.
 *   U(u) = trunc(u * 2^24) with u as mm_sample_rows reads it (NaN -> 0, else clamped to [0, 1 - 2^-24]), an integer in [0, 2^24).
 *   mulshift(z, U) = floor(U * z / 2^24), computed exactly as (z >> 24) * U + (((z & (2^24 - 1)) * U) >> 24).
 *   1 Greedy target.  The target row is in mm_sample_rows' greedy case (T <= 0 or NaN, maximum NaN or infinite): out_idx[r] is
 *     mm_argmax_rows' answer bit for bit; accepted[r] = 1 if it equals the candidate, 0 if a candidate exists and differs, -1 without
 *     a candidate.
 *   2 No candidate (x < 0 or x >= vocab).  out_idx[r] is what mm_sample_rows(logits, u_resample, ...) returns for the row, bit for
 *     bit; accepted[r] = -1.  The draft row is never read.
 *   3 One-hot draft.  draft_logits null, or the draft row itself in the greedy case: Q_x = Z_q = 1 and every other Q_i = 0 (n-gram,
 *     prompt-lookup and greedy drafts: the draft proposed x with certainty).
 *   4 Accept iff mulshift(Q_x * Z_p, U(u_accept[r])) < P_x * Z_q (both products are below 2^106).  Then out_idx[r] = x, accepted[r] = 1.
 *     Q_x = 0 < P_x always accepts; P_x = 0 always rejects; and because mulshift(z, U) < t iff U * z < 2^24 * t for integers, x is
 *     accepted iff U / 2^24 < p(x) / q(x): over the 2^24 values of U the acceptance probability is min(1, p / q) rounded UP to the
 *     2^-24 grid of u.
 *   5 Reject.  R_i = max(0, P_i * Z_q - Q_i * Z_p), ZR = sum_i R_i < 2^126, summed as 128-bit integers: exact in any order.
 *     want = mulshift(ZR, U(u_resample[r])); out_idx[r] = the first index, in ascending order, whose inclusive prefix sum of R exceeds
 *     want; accepted[r] = 0.
 *   Two facts about a rejected row:
 *     R_x = 0.  For z > 0, mulshift(z, U) <= z (2^24 - 1) / 2^24 < z.  Rejected means mulshift(Q_x Z_p, U) >= P_x Z_q; with Q_x > 0 this
 *     gives Q_x Z_p > P_x Z_q, so R_x = max(0, P_x Z_q - Q_x Z_p) = 0; with Q_x = 0 it gives 0 >= P_x Z_q, so P_x = 0 and R_x = 0 again.
 *     The redraw therefore never returns x, and mm_verify_greedy's walk stops at a rejected node.
 *     ZR > 0 whenever Q_x > 0, which holds for every x that was drawn from Q (and for the one-hot form).  sum_i (P_i Z_q - Q_i Z_p) =
 *     Z_p Z_q - Z_q Z_p = 0, so the positive parts of these differences add up to what the negative parts do: ZR = sum_i max(0, Q_i Z_p -
 *     P_i Z_q) >= Q_x Z_p - P_x Z_q > 0.  Hence want < ZR and the prefix passes it inside the row.  A candidate with Q_x = 0 and P_x = 0
 *     (one the draft could not have drawn) is rejected too and may meet ZR = 0, namely when P and Q are proportional; then out_idx[r]
 *     is the target's argmax -- a token with P > 0, so still not x.
 * Every mass is an integer and every sum exact, so the result is a function of the inputs alone: the same bits on every run and however
 * a row is divided among workgroups.  tests/spec_oracle.py holds the rule in Python integers.
 *
 * logits and draft_logits: bf16, 2-byte aligned, ld / draft_ld (elements between rows) >= vocab, each independent of the other; the
 * limits on vocab and rows and the split into parts of MM_ARGMAX_CHUNK columns are mm_sample_rows'.  logits and draft_logits may be the
 * same array.  workspace: mm_spec_sample_rows_workspace_bytes(rows, vocab) bytes (0 for arguments mm_spec_sample_rows refuses), 8-byte
 * aligned, always needed, no initialisation needed: every word read was written by the same call.  accepted may be null.
 * Launches, each over both matrices: mm_argmax_rows' one or two, mm_sample_rows' six select launches unless top_k and top_p are both
 * null, then three: 4 or 5 in all without the select, 10 or 11 with it.
 *
 * Statuses, all without device work.  MM_ERR_BAD_ARG: rows < 0, vocab < 1, ld < vocab, draft_ld < vocab with draft_logits; and, with
 * rows > 0: null logits, cand_tok, u_accept, u_resample or out_idx, an odd address of logits or draft_logits, any other array that is
 * not 4-byte aligned, a workspace that is null, too small or not 8-byte aligned.  MM_ERR_UNSUPPORTED: vocab > MM_ARGMAX_MAX_VOCAB or
 * rows > MM_ARGMAX_MAX_ROWS, for arguments that are not refused by the first line.  rows == 0: MM_OK.
 */
#ifndef MICROMIX_SPEC_H
#define MICROMIX_SPEC_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

size_t mm_spec_sample_rows_workspace_bytes(int rows, int vocab);
int mm_spec_sample_rows(const void *logits_bf16, long long ld /* elements between rows, >= vocab */,
                        const void *draft_logits_bf16 /* or null: one-hot drafts */, long long draft_ld /* >= vocab */,
                        int rows, int vocab,
                        const int32_t *cand_tok /* [rows]; < 0 or >= vocab: no candidate */,
                        const float *u_accept, const float *u_resample /* [rows] each, required */,
                        const float *temperature /* [rows] or null: 1.0 */, const int32_t *top_k /* [rows] or null: off */,
                        const float *top_p /* [rows] or null: off */, const float *min_p /* [rows] or null: off */,
                        int32_t *out_idx /* [rows] */, int32_t *accepted /* [rows] or null */,
                        void *workspace, size_t workspace_bytes, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
