/*
 * micromix_random.h -- the uniform numbers of a sampled decode step on the device: a counter-based generator without state.  The numbers
 * a row of mm_sample_rows / mm_spec_sample_rows needs are a function of the REQUEST'S SEED AND THE POSITION OF THE TOKEN BEING DECIDED,
 * and of nothing else: not of the batch the request shares, not of the row it sits in, not of the calls that came before.  A request
 * with a seed then samples the same tokens on every run, alone or among others, and a captured graph of several steps (mm_ngram_draft
 * -> mm_uniform_rows -> mm_spec_sample_rows -> mm_verify_greedy -> mm_token_step) draws fresh numbers every step because the positions
 * it reads from the device have moved on.
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The status
 * codes are micromix_hip.h's.  micromix_amd/paged.py (uniform_rows) is the Python side.
 *
 * Every parameter that can differ between requests is a DEVICE array, read by the kernel only.  Nothing is read on the host and nothing
 * is allocated: capture-safe.  NO STATE, NO ATOMIC, NO WORKSPACE: the outputs are a function of the inputs alone, and a program over
 * Python integers is the exact oracle (tests/random_oracle.py).  mm_sample_rows and mm_spec_sample_rows are unchanged and still take
 * their numbers from the caller; this call is one way to make them.
 *
 * mm_uniform_rows.  seed int64 [batch] and sub int32 [batch] (null: 0) belong to the sequences, row_seq int32 [rows] (null: row r is
 * sequence r) and pos int32 [rows] to the rows; n (1 .. MM_UNIFORM_MAX_N) streams of numbers are written per row; domain is a host value.
 * The rule, for row r with s = row_seq ? row_seq[r] : r:
 *   0 s outside [0, batch): out[i][r] = 0.0f and bits[i][r] = 0 for every i < n (device data cannot be refused).
 *   1 Otherwise, for block j < ceil(n / 4): (w0, w1, w2, w3) = Philox4x32-10(counter, key) with
 *       counter = (c0, c1, c2, c3) = ((uint32)pos[r], (uint32)(sub ? sub[s] : 0), j, domain)
 *       key     = (k0, k1)         = the low and the high 32 bits of seed[s]
 *     This is Random123's Philox4x32 with 10 rounds (Salmon, Moraes, Dror, Shaw: Parallel Random Numbers: As Easy as 1, 2, 3, SC'11):
 *     M0 = 0xD2511F53, M1 = 0xCD9E8D57; one round is c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)) with
 *     hi / lo the halves of the 64-bit product; the key is bumped by (0x9E3779B9, 0xBB67AE85) between two rounds (nine times).
 *   2 Stream i = 4 j + w (i < n) gets bits[i * ld_out + r] = w_w and out[i * ld_out + r] = (float)(w_w >> 8) * 2^-24.
 *   EVERY u LIES ON THE 2^-24 GRID IN [0, 1 - 2^-24]: the set mm_sample_rows and mm_spec_sample_rows read without clamping, on which
 *   their U(u) = trunc(u * 2^24) recovers w >> 8 exactly.  The low 8 bits of a word are dropped, not rounded: u < 1 always.
 *   Layout: THE STREAMS ARE ROWS OF out, [n, ld_out] with ld_out >= rows.  out + 0 * ld_out, out + 1 * ld_out and out + 2 * ld_out are
 *   contiguous [rows] arrays: u_accept, u_resample and mm_sample_rows' u without a copy.  Elements r >= rows of a stream (the slack of
 *   ld_out) are not written.  out or bits may be null (not both): that output is not wanted.
 *   Shape: one lane per (row, block), rows fastest, so the up to four stores of a lane go to four stream rows and each is coalesced
 *   across the wave; the 32 x 32 -> 64 products are a high multiply and a 32-bit multiply.  The call is a launch and little else.
 *
 * What the arguments mean.
 *   pos[r]   THE INDEX IN THE HISTORY AT WHICH THE TOKEN THAT ROW DECIDES WILL BE COMMITTED: row_total_len as mm_ngram_draft writes it
 *            (row i of a chain decides the token at total_len + i); for a plain decode step the sequence's total_len.  Taken as a
 *            32-bit pattern: a negative value is a counter like any other.
 *   sub      separates the n samples or the beams of one prompt under one seed: same seed, same positions, other numbers.
 *   domain   separates consumers, for example the target's sampler from a draft model's sampler, which must not see the same numbers.
 *   seed     the request's.  Two requests with the same (seed, sub) draw the same numbers at the same position -- that is the point.
 *
 * Why numbers keyed by position are sound in a speculative step.  A position's token is committed exactly once.  Rows behind a
 * rejection are evaluated and thrown away; the walk stops at the rejection whatever those rows drew, so their numbers decide nothing.
 * When such a position is evaluated again in a later step, with the same numbers, its context is the committed history, which depends
 * only on the numbers of EARLIER positions and on the draft; with mm_ngram_draft the draft is a function of the history too.  So the
 * numbers that decide position p are independent of everything that formed its context, which is all that the speculative-sampling
 * rule (micromix_spec.h) asks of u_accept and u_resample: the committed token at p is distributed as the target's.  (A draft MODEL that
 * samples must draw from another domain, or its proposal for p would be correlated with the test that judges it.)
 * Sibling nodes of a tree share a position and therefore share numbers.  At most one sibling lies on the accepted path, and which one
 * is decided by the parent's row, whose position and numbers are another's: the shared numbers are used once.
 *
 * Limits: n <= MM_UNIFORM_MAX_N = 16 (four blocks), rows <= MM_UNIFORM_MAX_ROWS = 2^24.
 *
 * Statuses, all without device work.  MM_ERR_BAD_ARG: rows < 0, batch < 0, n < 1, ld_out < rows; with rows > 0: out and bits both null,
 * null pos, null seed with batch > 0; seed not 8-byte aligned, any other array not 4-byte aligned.  MM_ERR_UNSUPPORTED, for arguments
 * the lines above do not refuse: n > MM_UNIFORM_MAX_N or rows > MM_UNIFORM_MAX_ROWS.  rows == 0: MM_OK.  batch == 0 with rows > 0 is
 * served: every row is outside [0, 0) and gets zeros.
 */
#ifndef MICROMIX_RANDOM_H
#define MICROMIX_RANDOM_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MM_UNIFORM_MAX_N 16
#define MM_UNIFORM_MAX_ROWS (1 << 24)

int mm_uniform_rows(const int64_t *seed /* [batch] */, const int32_t *sub /* [batch] or null: 0 */, int batch,
                    const int32_t *row_seq /* [rows] or null: row r is sequence r */, const int32_t *pos /* [rows] */,
                    int rows, int n /* 1 .. 16 */, unsigned domain,
                    float *out /* [n, ld_out] or null */, uint32_t *bits /* [n, ld_out] or null */, long long ld_out,
                    mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
