/*
 * micromix_calib.h -- calibration statistics on the device: the streaming form of the rule that produces the side inputs every
 * quantizer and GEMM of micromix_hip.h takes (the per-layer reorder_index and the p6_num / p8_num split).
 *
 * Exported from libmicromix_hip.so next to micromix_hip.h's entries and detected by symbol; mm_version() does not change.  The
 * status codes are micromix_hip.h's.  micromix_amd/calib.py (accumulate, Calibrator) is the Python side.
 *
 * One call of mm_calib_accumulate is one batch of the reference's rule (reorder_indices.py:41-51, 98-108): one hooked forward pass of
 * one linear layer, its input seen as x [rows, K] (bf16 or fp16, `ld` elements between rows, unit stride along K).  Every value
 * converts exactly to fp32; all arithmetic below is on those fp32 values.  The state of a layer is score_f32 [K] and
 * counts_i64 [2]; all zero is the empty state (the first batch's maximum with 0 is its mean, :49-51).
 *
 *   Row thresholds.  m_r = max_c |x[r][c]|, NaN when the row holds a NaN (as torch.max gives).
 *       t4_r = ((m_r * 448.0f) / 6.0f) / 1024.0f * lamda
 *       t6_r = ((m_r * 448.0f) / 28.0f) / 64.0f * lamda
 *     each operation a separately rounded round-to-nearest fp32 operation in this order, the divisions correctly rounded, no
 *     reciprocal, no contraction, subnormals kept: what torch computes on the CPU for :103-104.
 *   Counts.  counts[0] += #{(r, c): |x[r][c]| < t4_r}, counts[1] += #{(r, c): |x[r][c]| < t6_r}; strict fp32 comparisons, so a NaN
 *     threshold counts nothing, an infinite one counts every finite value and an all-zero row counts nothing.  Exact 64-bit integers.
 *   Channel scores.  mean_c = fp32(S_c / rows) with S_c = sum_r |x[r][c]|; score[c] = max(score[c], mean_c), a NaN on either side
 *     giving NaN (torch.max, :47).
 *   S_c.  R = 8.  Rows [8 s, 8 s + 8) form slice s; inside a slice |x[r][c]| is added in ascending r in fp32, starting from 0; the
 *     slice sums are added in fp64 in ascending s: the n = ceil(rows / 8) slices form 32 contiguous runs of ceil(n / 32) (the last ones
 *     shorter or empty), each run is added in ascending s starting from 0, and the runs are added in ascending order.  The division by
 *     rows is an fp64 division and its quotient is rounded to fp32.  The tree depends on (rows, K) alone: the same bits come out of
 *     every run, there are no float atomics, and the workspace needs no initialisation (every word read was stored earlier in the
 *     same call).  Relative error of mean_c against the exact mean of a finite column: at most (R + 1) * 2^-24 = 9 * 2^-24 (R - 1
 *     fp32 additions of non-negative terms, the fp64 steps, one rounding).
 *
 * Nothing beyond x[rows - 1][K - 1] is read, and the padding between rows (ld > K) is never read.
 *
 * Statuses, all without device work.  MM_ERR_BAD_ARG: negative rows or K, ld < K, lamda not finite or <= 0; and, with rows > 0, a
 * null x / score_f32 / counts_i64 / workspace, x or ld * element size not 16-byte aligned, score_f32 not 4-byte or counts_i64 not
 * 8-byte aligned, a workspace smaller than mm_calib_workspace_bytes(rows, K) or not 16-byte aligned.  MM_ERR_UNSUPPORTED: K < 128,
 * K % 128 != 0, K > 32768, rows > 2^20, a dtype other than 0 or 1.  rows == 0: MM_OK with nothing touched (the reference fails on an
 * empty batch; an unrouted MoE expert produces one).  mm_calib_workspace_bytes: ceil(rows / 8) * (4 K + 16) bytes, 0 for arguments
 * mm_calib_accumulate refuses and for rows == 0.  Two launches on `stream`, no host synchronisation, capture-safe.
 */
#ifndef MICROMIX_CALIB_H
#define MICROMIX_CALIB_H
#include "micromix_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

size_t mm_calib_workspace_bytes(int rows, int K);
int mm_calib_accumulate(const void *x, int dtype /* 0: bf16, 1: fp16 */, int rows, int K, long long ld /* elements between rows, >= K */,
                        float lamda, void *score_f32 /* [K] */, void *counts_i64 /* [2] */, void *workspace, size_t workspace_bytes,
                        mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
