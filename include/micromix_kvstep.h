/*
 * micromix_kvstep.h -- the device half of the paged KV cache's allocator: commit a draft and announce the next step without the host.
 *
 * Between two decode steps the page table has to change: the rejected part of a draft is dropped, its pages return to the free list,
 * the next tokens get pages, and kv_indptr / kv_indices / last_page_len / append_indptr are rewritten.  PagedKVCache does that on the
 * host (accept + extend), which costs a device-to-host copy, Python list walks and five uploads per generated token.  mm_kv_step does the
 * same bookkeeping on the device, from mm_verify_greedy's result, so that one captured graph can hold several steps; the host reads the
 * state back only when it wants to (PagedKVCache.sync).
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The status
 * codes a CALL returns are micromix_hip.h's; what a STEP found is a MM_KV_STEP_* value in the state (below).  micromix_amd/paged.py
 * (kv_step) is the Python side, micromix_amd/kvcache.py (step_launch, sync, steps_guaranteed) the cache on top.
 *
 * The state: one int32 device buffer of mm_kv_step_state_ints(batch, max_pages, pages_per_seq) entries, which the host fills with one
 * copy and reads with one copy.  With B = batch:
 *   [0] status        0, or the MM_KV_STEP_* value of the first step that failed (sticky, below)
 *   [1] steps_done    the steps performed; a failed step is not counted
 *   [2] free_count    the entries of the free stack
 *   [3] failed_step   the value steps_done had when status was set: the number, from 0, of the step that failed
 *   [MM_KV_STEP_HEADER_INTS + 0 * B ..)  seq_len[B]     the tokens of each sequence, the announced ones included
 *   [MM_KV_STEP_HEADER_INTS + 1 * B ..)  announced[B]   the tokens of the last announce: the last `announced[b]` of seq_len[b]
 *   [MM_KV_STEP_HEADER_INTS + 2 * B ..)  num_pages[B]   the entries of each sequence's page list
 *   [MM_KV_STEP_HEADER_INTS + 3 * B ..)  free[max_pages]   a stack whose top is free[free_count - 1]; entries at and past free_count mean nothing
 *   [MM_KV_STEP_HEADER_INTS + 3 * B + max_pages ..)  pages[B * pages_per_seq]   the padded master copy of the page lists: sequence b's is
 *                                       pages[b * pages_per_seq + j], j < num_pages[b]; entries past num_pages[b] mean nothing
 *
 * The rule.  P = page_size, ceil(x / P) over integers, k_b = keep ? keep[b * keep_stride] : announced[b] (mm_verify_greedy's result, whose
 * row begins with the length of the accepted path, fits with keep_stride = MM_VERIFY_STRIDE), n_b = next_new[b].
 *   1 Shorten, for b ascending: base = seq_len[b] - announced[b]; seq_len[b] = base + k_b; keep_pages = ceil(seq_len[b] / P).  The pages at
 *     list entries >= keep_pages are pushed on the stack, HIGHEST ENTRY FIRST (entry num_pages[b] - 1, then num_pages[b] - 2, ...), and
 *     num_pages[b] = keep_pages.
 *   2 After ALL sequences are shortened, for b ascending: need = ceil((seq_len[b] + n_b) / P) - num_pages[b] pages are popped from the top
 *     and appended to the list in pop order.  Then seq_len[b] += n_b and announced[b] = n_b.
 *   3 Outputs.  kv_indptr[b] = the sum of num_pages below b (kv_indptr[batch]: of all); kv_indices[kv_indptr[b] + j] = pages[b][j], entries
 *     at and past kv_indptr[batch] are not touched; last_page_len[b] = seq_len[b] - (num_pages[b] - 1) * P, 0 for an empty sequence;
 *     append_indptr[b] = the sum of n below b; token_pos[append_indptr[b] + i] = (seq_len[b] - n_b) + (depths ? depths[append_indptr[b] +
 *     i] : i) for i < n_b: the position of new token i, which is its cos / sin row for mm_rope_kv_append.  steps_done += 1.
 * This is what PagedKVCache's _keep_paths followed by extend computes on a cache that releases nothing below a window and needs no
 * copy-on-write, page numbers included: the pushes and pops land where the sequential host loops put them, because every sequence's
 * offset into the stack is a prefix sum over the sequences before it -- push t of sequence b goes to free[free_count + (pushes below b)
 * + t], pop t of sequence b takes free[top - 1 - (pops below b) - t] with top = free_count + all pushes -- and no atomic is involved.
 * THE TABLES ARE A FUNCTION OF THE INPUTS ALONE.
 *
 * No reference counts.  A dropped page lies wholly past base, so it holds only announced tokens, which only this sequence wrote into a
 * page it took from the free list for them: it is never shared, and it goes back to the stack without a count.  Pages that sequences
 * share (a forked prompt) lie below base and are never pushed.  What the caller has to see to is PagedKVCache's sole-owner rule for the
 * page that RECEIVES tokens: no sequence's partly filled last page may be shared when the first step is taken (the host extend
 * establishes that by its copy-on-write).  Steps keep it: a sequence's last page after a step is either the page it had, still its own,
 * or one popped from the stack, which no list names.
 *
 * All or nothing.  A step is evaluated completely before anything is written.  If a condition below holds, every table and the state
 * stay as they were, except status = the condition's value and failed_step = steps_done.  Conditions of a sequence come first: when any
 * sequence meets one, status is the SMALLEST value met by any sequence, and the conditions of the whole step are not looked at;
 * otherwise it is the first of those, in the order below, that holds.
 *   of a sequence:   MM_KV_STEP_BAD_STATE        seq_len or announced negative, announced > seq_len, num_pages > pages_per_seq or
 *                                                num_pages != ceil(seq_len / P): not a state this rule leaves
 *                    MM_KV_STEP_BAD_KEEP         k_b outside [0, announced[b]]
 *                    MM_KV_STEP_BAD_NEXT         n_b < 0
 *                    MM_KV_STEP_TOO_LONG         base + k_b + n_b > max_seq_len
 *                    MM_KV_STEP_SEQ_PAGES        ceil((base + k_b + n_b) / P) > pages_per_seq
 *   of the step:     MM_KV_STEP_BAD_STATE        free_count < 0 or free_count + the pushes > max_pages
 *                    MM_KV_STEP_BAD_SUM          the sum of n_b is not num_next_tokens
 *                    MM_KV_STEP_OUT_OF_PAGES     more pops than the stack holds after the pushes
 *                    MM_KV_STEP_INDICES_CAPACITY kv_indptr[batch] > kv_indices_capacity
 * status is sticky: a call that finds it non-zero does nothing at all.  A captured graph of several steps is therefore safe past a
 * failure: the later appends and attention launches of the graph run over the tables of the last good step, rewriting slots the
 * sequences already own.  The host clears status by writing the state again.
 *
 * Shape: one workgroup of up to 1024 lanes, a sequence to a lane, scans within a wave and through on-chip memory across waves, each lane
 * looping over its own pushes and pops; then a second launch over (sequence, chunk) that rebuilds kv_indices from the padded master and
 * writes token_pos.  Hence batch <= MM_KV_STEP_MAX_BATCH.  Nothing is read on the host, nothing allocated, there is no workspace
 * beyond the state: capture-safe.
 *
 * Statuses of the call, all without device work.  MM_ERR_BAD_ARG: batch < 0; max_pages, pages_per_seq, page_size or max_seq_len < 1;
 * num_next_tokens < 0; kv_indices_capacity < 0; keep with keep_stride < 1; depths without token_pos; and, with batch > 0: null state,
 * next_new, kv_indptr, kv_indices, last_page_len or append_indptr; any array that is not 4-byte aligned.  A null token_pos is allowed
 * (the positions are not wanted), also with num_next_tokens > 0.  MM_ERR_UNSUPPORTED, for arguments the first line does not refuse:
 * batch > MM_KV_STEP_MAX_BATCH, or a state of more than 2^31 - 1 entries.  batch == 0: MM_OK.
 * mm_kv_step_state_ints returns 0 for arguments mm_kv_step refuses and for batch == 0.
 */
#ifndef MICROMIX_KVSTEP_H
#define MICROMIX_KVSTEP_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MM_KV_STEP_MAX_BATCH 1024
#define MM_KV_STEP_HEADER_INTS 4

#define MM_KV_STEP_OK 0
#define MM_KV_STEP_BAD_STATE 1
#define MM_KV_STEP_BAD_KEEP 2
#define MM_KV_STEP_BAD_NEXT 3
#define MM_KV_STEP_TOO_LONG 4
#define MM_KV_STEP_SEQ_PAGES 5
#define MM_KV_STEP_BAD_SUM 6
#define MM_KV_STEP_OUT_OF_PAGES 7
#define MM_KV_STEP_INDICES_CAPACITY 8

size_t mm_kv_step_state_ints(int batch, int max_pages, int pages_per_seq);
int mm_kv_step(int32_t *state, int batch, int max_pages, int pages_per_seq, int page_size, int max_seq_len,
               const int32_t *keep /* keep[b * keep_stride], or null: all stay */, int keep_stride,
               const int32_t *next_new /* [batch] */, int num_next_tokens /* what they must sum to */,
               const int32_t *depths /* [num_next_tokens] or null */,
               int32_t *kv_indptr /* [batch + 1] */, int32_t *kv_indices, long long kv_indices_capacity, int32_t *last_page_len /* [batch] */,
               int32_t *append_indptr /* [batch + 1] */, int32_t *token_pos /* [num_next_tokens] or null */, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
