// Calibration statistics of one activation batch (mm_calib_accumulate, include/micromix_calib.h): the row maxima, the two counts of
// elements below the rows' thresholds and the column sums of |x|, in one pass over x where it lies; the rule is stated in the header.
//
// Two launches:
//   calib_rows_kernel   a 256-lane workgroup takes the CAL_R = 8 consecutive rows of a slice.  A lane owns fixed 16-byte pieces of
//                       a row (piece t + 256 j), so its column sums stay in its own registers and never cross lanes.  Per batch of RB
//                       rows: the loads, the lane's maxima, one reduction over the workgroup (the maxima of a batch packed two to a
//                       word, one barrier, LDS slots taken in turns), then the lane's own registers against the two thresholds.
//                       The next batch's loads are issued before this batch is worked on.  A slice's column sums and its two
//                       counts leave by plain stores, a slice of the workspace per workgroup.
//   calib_fold_kernel   32 columns by 32 runs per workgroup: the slice sums of a column in fp64, in ascending order inside each of
//                       32 contiguous runs of slices, the runs then in ascending order; the division, and the maximum with score[c].
//                       The last workgroup adds the slices' counts (integers: any order) to counts.  One lane per element of the
//                       state, ordered against the calls before and after by the stream.
//
// |x| is taken on the bits (the sign cleared), and the maxima are maxima of those bits as unsigned 16-bit integers: below the NaN codes
// that is the order of the values, and a NaN code is larger than every other, so a row with a NaN has a NaN maximum as torch.max gives.
//
// The counts compare codes, not values: |x| < t in fp32 holds exactly when the 15-bit code of |x| is below T, the lowest code whose
// value is >= t (the codes of a format grow with their values up to infinity's; T = 0 for a NaN threshold, infinity's code for an
// infinite one, which leaves out the infinities and the NaNs above them).  Two elements are compared by one packed 16-bit subtraction,
// whose sign bits are the answers, and counted in the halves of one register (at most 8 * 16 * 4 per half and lane).
//
// Reads go through one buffer descriptor per row, [x + row * ld, + K elements): a piece beyond K, and every piece of a row beyond
// `rows` (a descriptor of 0 bytes), reads as 0 without touching memory.  A 0 adds nothing to a sum or a maximum, but 0 < t holds for a
// positive threshold: the pieces beyond K are counted out again, 8 * (256 PPT - K / 8) per row and threshold with 0 < t.
#include "../../include/micromix_calib.h"
#include "mx_buffer_ops.h"
#include "mx_kernels.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

typedef unsigned long long u64;
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
typedef short ss2 __attribute__((ext_vector_type(2)));

constexpr int CAL_THREADS = 256, CAL_R = 8;             // lanes of a workgroup; rows of a slice (R of the header)
constexpr int CAL_FOLD_COLS = 32, CAL_FOLD_RUNS = 32;    // the fold's workgroup: columns by runs of slices

struct CalibArgs {
    const uint8_t *x;
    long long row_bytes;     // ld in bytes
    int rows, K;
    float lamda;
    float *part_sum;         // [slices][K]
    u64 *part_cnt;           // [slices][2]
};

// the larger of each 16-bit half
__device__ __forceinline__ unsigned pk_max(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}

// the fp32 value of 16 bits of a bf16 / fp16
template <bool FP16>
__device__ __forceinline__ float widen(unsigned bits16) {
    if constexpr (FP16) return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
    return __uint_as_float(bits16 << 16);
}

// the lowest code of the format whose value is >= t, in both halves of a word: t >= 0 or NaN
template <bool FP16>
__device__ __forceinline__ unsigned code_at_or_above(float t) {
    unsigned code;
    if constexpr (FP16) {
        const _Float16 h = (_Float16)t;                                // to nearest; beyond the largest finite value: infinity
        code = (unsigned)__builtin_bit_cast(unsigned short, h) + ((float)h < t ? 1u : 0u);
    } else {
        const unsigned u = __float_as_uint(t);
        code = (u >> 16) + ((u & 0xFFFFu) ? 1u : 0u);
    }
    code = t != t ? 0u : code;
    return code | code << 16;
}

// counts, in the halves of c, the halves of w (15-bit codes) that are below those of T (codes up to infinity's)
__device__ __forceinline__ unsigned count_below(unsigned c, unsigned w, unsigned T) {
    const ss2 below = __builtin_bit_cast(ss2, __builtin_bit_cast(us2, w) - __builtin_bit_cast(us2, T)) >> 15;   // -1 where w < T
    return __builtin_bit_cast(unsigned, __builtin_bit_cast(us2, c) - __builtin_bit_cast(us2, below));
}

// PPT: pieces of a row per lane (256 PPT * 8 >= K); RB: rows per batch
template <int PPT, int RB, bool FP16>
__global__ __launch_bounds__(CAL_THREADS) void calib_rows_kernel(CalibArgs a) {
    constexpr int NB = CAL_R / RB, NP = (RB + 1) / 2;                 // batches of a slice; words of packed maxima per batch
    constexpr bool AHEAD = NB > 1 && PPT <= 8;                         // the next batch's loads in flight under this batch's work
    static_assert(NB * RB == CAL_R && (NB == 1 || NB % 2 == 0), "a slice is whole batches, taken in pairs");
    __shared__ unsigned s_max[2][NP][CAL_THREADS / 64];
    __shared__ unsigned s_cnt[CAL_THREADS / 64][2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int row0 = blockIdx.x * CAL_R;
    const unsigned row_len = (unsigned)a.K * 2u;

    float sum[PPT][8];
#pragma unroll
    for (int j = 0; j < PPT; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) sum[j][e] = 0.0f;
    unsigned c4 = 0, c6 = 0;          // elements below the thresholds, this lane's, a count in each half
    unsigned pos4 = 0, pos6 = 0;      // rows with 0 < t4, 0 < t6

    auto load = [&](v4i (&raw)[RB][PPT], int b) {
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int row = row0 + b * RB + i;
            const __amdgpu_buffer_rsrc_t rsrc = make_brsrc(a.x + (size_t)min(row, a.rows - 1) * (size_t)a.row_bytes, row < a.rows ? row_len : 0u);
#pragma unroll
            for (int j = 0; j < PPT; ++j) raw[i][j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (t + CAL_THREADS * j) * 16, 0, 0);
        }
    };

    auto work = [&](v4i (&raw)[RB][PPT], int b) {
        if (row0 + b * RB >= a.rows) return;                           // the whole workgroup alike
        unsigned pk[NP];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            unsigned m = 0;
#pragma unroll
            for (int j = 0; j < PPT; ++j)
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    raw[i][j][d] &= 0x7FFF7FFF;                        // |x|
                    m = pk_max(m, (unsigned)raw[i][j][d]);
                }
            m = max(m & 0xFFFFu, m >> 16);
            if (i & 1) pk[i >> 1] |= m << 16;
            else pk[i >> 1] = m;
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
            for (int off = 32; off; off >>= 1) pk[p] = pk_max(pk[p], (unsigned)__shfl_xor((int)pk[p], off));
            if (lane == 0) s_max[b & 1][p][wave] = pk[p];
        }
        // one barrier per batch: batch b + 2 writes these slots again only after every lane has passed batch b + 1's barrier, behind
        // which nobody reads batch b's
        __syncthreads();
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            pk[p] = s_max[b & 1][p][0];
#pragma unroll
            for (int w = 1; w < CAL_THREADS / 64; ++w) pk[p] = pk_max(pk[p], s_max[b & 1][p][w]);
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const float m = widen<FP16>((pk[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
            const float t4 = __fmul_rn(__fdiv_rn(__fdiv_rn(__fmul_rn(m, 448.0f), 6.0f), 1024.0f), a.lamda);
            const float t6 = __fmul_rn(__fdiv_rn(__fdiv_rn(__fmul_rn(m, 448.0f), 28.0f), 64.0f), a.lamda);
            const unsigned T4 = code_at_or_above<FP16>(t4), T6 = code_at_or_above<FP16>(t6);
            pos4 += T4 != 0u;
            pos6 += T6 != 0u;
#pragma unroll
            for (int j = 0; j < PPT; ++j)
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const unsigned w = (unsigned)raw[i][j][d];
                    sum[j][2 * d] += widen<FP16>(w & 0xFFFFu);
                    sum[j][2 * d + 1] += widen<FP16>(w >> 16);
                    c4 = count_below(c4, w, T4);
                    c6 = count_below(c6, w, T6);
                }
        }
    };

    v4i A[RB][PPT];
    if constexpr (NB == 1) {
        load(A, 0);
        work(A, 0);
    } else if constexpr (AHEAD) {
        v4i B[RB][PPT];
        load(A, 0);
#pragma unroll 1
        for (int b = 0; b < NB; b += 2) {
            load(B, b + 1);
            work(A, b);
            if (b + 2 < NB) load(A, b + 2);
            work(B, b + 1);
        }
    } else {
#pragma unroll 1
        for (int b = 0; b < NB; ++b) {
            load(A, b);
            work(A, b);
        }
    }

    const int pieces = a.K >> 3;
    float *out = a.part_sum + (size_t)blockIdx.x * (size_t)a.K;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int piece = t + CAL_THREADS * j;
        if (piece < pieces) {
            v4f *o = (v4f *)(out + (size_t)piece * 8);
            o[0] = v4f{sum[j][0], sum[j][1], sum[j][2], sum[j][3]};
            o[1] = v4f{sum[j][4], sum[j][5], sum[j][6], sum[j][7]};
        }
    }
    c4 = (c4 & 0xFFFFu) + (c4 >> 16);
    c6 = (c6 & 0xFFFFu) + (c6 >> 16);
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        c4 += (unsigned)__shfl_xor((int)c4, off);
        c6 += (unsigned)__shfl_xor((int)c6, off);
    }
    if (lane == 0) {
        s_cnt[wave][0] = c4;
        s_cnt[wave][1] = c6;
    }
    __syncthreads();
    if (t < 2) {
        unsigned c = 0;
#pragma unroll
        for (int w = 0; w < CAL_THREADS / 64; ++w) c += s_cnt[w][t];
        const unsigned beyond = 8u * (unsigned)(CAL_THREADS * PPT - pieces);   // the zeros read beyond K, per row
        a.part_cnt[(size_t)blockIdx.x * 2 + t] = (u64)(c - beyond * (t ? pos6 : pos4));
    }
}

// grid K / 32 + 1
__global__ __launch_bounds__(CAL_FOLD_COLS *CAL_FOLD_RUNS) void calib_fold_kernel(const float *__restrict__ part_sum,
                                                                                   const u64 *__restrict__ part_cnt, int slices, int rows,
                                                                                   int K, float *score, long long *counts) {
    constexpr int THREADS = CAL_FOLD_COLS * CAL_FOLD_RUNS;
    const int t = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {
        __shared__ u64 s_c[THREADS];
        const int which = t & 1;
        u64 c = 0;
        for (int s = t >> 1; s < slices; s += THREADS / 2) c += part_cnt[(size_t)s * 2 + which];
        s_c[t] = c;
        __syncthreads();
        for (int off = THREADS / 2; off >= 2; off >>= 1) {
            if (t < off) s_c[t] += s_c[t + off];
            __syncthreads();
        }
        if (t < 2) counts[t] += (long long)s_c[t];
        return;
    }
    __shared__ double s_run[CAL_FOLD_RUNS][CAL_FOLD_COLS];
    const int col = blockIdx.x * CAL_FOLD_COLS + (t & (CAL_FOLD_COLS - 1)), run = t / CAL_FOLD_COLS;
    const int per = (slices + CAL_FOLD_RUNS - 1) / CAL_FOLD_RUNS, end = min(slices, (run + 1) * per);
    const float *p = part_sum + col;
    double acc = 0.0;
    int s = run * per;
    for (; s + 8 <= end; s += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(s + u) * (size_t)K];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (double)v[u];
    }
    for (; s < end; ++s) acc += (double)p[(size_t)s * (size_t)K];
    s_run[run][t & (CAL_FOLD_COLS - 1)] = acc;
    __syncthreads();
    if (run == 0) {
#pragma unroll
        for (int r = 1; r < CAL_FOLD_RUNS; ++r) acc += s_run[r][t];
        const float mean = (float)(acc / (double)rows), old = score[col];
        score[col] = mean != mean ? mean : old != old ? old : fmaxf(old, mean);
    }
}

size_t calib_workspace_bytes(int rows, int K) {
    const size_t slices = ((size_t)rows + CAL_R - 1) / CAL_R;
    return slices * ((size_t)K * sizeof(float) + 2 * sizeof(u64));
}

template <bool FP16>
static void launch_rows(const CalibArgs &a, int slices, hipStream_t stream) {
    const int ppt = (a.K / 8 + CAL_THREADS - 1) / CAL_THREADS;
    if (ppt <= 1) calib_rows_kernel<1, 8, FP16><<<slices, CAL_THREADS, 0, stream>>>(a);
    else if (ppt <= 2) calib_rows_kernel<2, 4, FP16><<<slices, CAL_THREADS, 0, stream>>>(a);
    else if (ppt <= 4) calib_rows_kernel<4, 2, FP16><<<slices, CAL_THREADS, 0, stream>>>(a);
    else if (ppt <= 8) calib_rows_kernel<8, 1, FP16><<<slices, CAL_THREADS, 0, stream>>>(a);
    else calib_rows_kernel<16, 1, FP16><<<slices, CAL_THREADS, 0, stream>>>(a);
}

hipError_t launch_calib_accumulate(const void *x, bool fp16, int rows, int K, long long ld, float lamda, float *score, long long *counts,
                                   void *ws, hipStream_t stream) {
    const int slices = (rows + CAL_R - 1) / CAL_R;
    CalibArgs a{(const uint8_t *)x, ld * 2, rows, K, lamda, (float *)ws, (u64 *)((char *)ws + (size_t)slices * (size_t)K * sizeof(float))};
    if (fp16) launch_rows<true>(a, slices, stream);
    else launch_rows<false>(a, slices, stream);
    calib_fold_kernel<<<K / CAL_FOLD_COLS + 1, CAL_FOLD_COLS * CAL_FOLD_RUNS, 0, stream>>>(a.part_sum, a.part_cnt, slices, rows, K, score, counts);
    return hipGetLastError();
}

}  // namespace mm
