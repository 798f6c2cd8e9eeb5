// Sampling a token per row of bf16 logits (mm_sample_rows, include/micromix_hip.h): temperature, top-k, top-p and min-p with per-row
// parameters read on the device, the rule stated in the header.
//
// A bf16 row holds at most 65 281 distinct values and mx_argmax_key.h maps each to a 16-bit key that grows with it, so the three
// filters -- each a prefix of the classes (equal values) in descending order -- are one threshold key `kt`, found by a radix select:
// a 256-bin histogram over the key's high byte, then one over the low byte inside the bin where the count (top-k) or the mass (top-p)
// crosses.  No sort, no scratch array of the row, no loop of unknown length.
//
// Masses are integers.  A weight w = exp2((l - m) * (log2e / T)), fp32 in [0, 1], becomes W = trunc(w * 2^43), a 64-bit integer:
// 2^20 of them cannot overflow, integer addition is associative, and so every histogram bin, every part sum, the kept mass Z and the
// prefix sums of the draw are the same numbers however a row is divided among lanes, waves and workgroups and whoever finishes first.
// The histograms are built with integer LDS atomics (order-free for that reason); there are no float atomics and no tickets.  Every
// workspace word a kernel reads was stored by an earlier kernel of the same call, so the workspace needs no initialisation.
//
// The launches of one call, each on the whole batch, a row's workgroups leaving at once where the row has nothing to do there:
//   argmax_rows (verify.hip)     out[r] = the row's argmax: the greedy answer, and m = logits[r][out[r]] for every kernel below
//   hist 1, finish 1             level-1 histogram of counts and masses per part; summed over the parts, suffix sums from the top,
//                                the bin where top-k (or, without top-k, top-p) crosses
//   hist 2, finish 2             level-2 histogram inside that bin: top-k's threshold key and Z_k, then top-p's bin; the same bin: done
//   hist 2, finish 3             level-2 histogram inside top-p's bin, when it lies above top-k's
//   mass                         the kept mass of every part: key >= kt and w >= min_p
//   draw                         Z, the part that holds u * Z, and the column inside it
// The six select launches are left out when top_k and top_p are both null; a row with neither filter on leaves them at once.
// What spec_sample.hip (mm_spec_sample_rows) shares -- the row's rule, the kept mass of a token, the select as launch_sample_select --
// is declared in mx_sample_select.h; a row whose SampleParams::cand entry names no token leaves the select at once, unread.
#include "../../include/micromix_hip.h"
#include "mx_argmax_key.h"
#include "mx_kernels.h"
#include "mx_row_weights.h"
#include "mx_sample_select.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

// grid (parts, rows) or (parts, rows, 2): z names the side.  level 1: bins are the key's high byte; level 2: its low byte, for the keys
// whose high byte is state[row].bin
__global__ __launch_bounds__(SMP_THREADS) void sample_hist_kernel(SelectSide first, SelectSide second, int level) {
    __shared__ u64 s_mass[256];
    __shared__ unsigned s_cnt[256];
    const int t = threadIdx.x, row = blockIdx.y, lo = blockIdx.x * MM_ARGMAX_CHUNK;
    const SelectSide &side = blockIdx.z ? second : first;
    const SampleParams &a = side.a;
    const SampleRow *state = side.state;
    u64 *hist_mass = side.hist_mass;
    unsigned *hist_cnt = side.hist_cnt;
    if (skipped(a, row)) return;
    const RowRule r = row_rule(a, row);
    if (r.greedy || !(r.has_k || r.has_p)) return;
    const int bin = level == 1 ? -1 : state[row].bin;
    if (level == 2 && bin < 0) return;
    s_mass[t] = 0;
    s_cnt[t] = 0;
    __syncthreads();
    for_each_in_part(a.logits + (long long)row * a.ld + lo, min(a.vocab - lo, MM_ARGMAX_CHUNK), t, [&](unsigned bits) {
        const unsigned key = argmax_key(bits);
        if (level == 1 || (int)(key >> 8) == bin) {
            const unsigned b = level == 1 ? key >> 8 : key & 255u;
            atomicAdd(&s_cnt[b], 1u);
            const u64 W = fixed(weight(bits, key, r));
            if (W) atomicAdd(&s_mass[b], W);
        }
    });
    __syncthreads();
    const long long at = ((long long)row * gridDim.x + blockIdx.x) * 256 + t;
    hist_mass[at] = s_mass[t];
    hist_cnt[at] = s_cnt[t];
}

// the largest bin b with f(b) >= x, where f does not grow with b and f(0) >= x >= 1: lane b tests itself against f(b + 1)
#define SMP_CROSSES(f_here, f_next, x) ((f_here) >= (x) && (f_next) < (x))

// grid rows or (rows, 2): y names the side; 256 lanes, lane b the bin b.  stage 1 follows the level-1 sweep, stages 2 and 3 a level-2
// sweep each
__global__ __launch_bounds__(256) void sample_finish_kernel(SelectSide first, SelectSide second, int stage, int parts) {
    __shared__ u64 s_m[257];
    __shared__ unsigned s_c[257];
    __shared__ u64 s_zk;
    __shared__ int s_bin;
    const int t = threadIdx.x, row = blockIdx.x;
    const SelectSide &side = blockIdx.y ? second : first;
    const SampleParams &a = side.a;
    SampleRow *state = side.state;
    const u64 *hist_mass = side.hist_mass;
    const unsigned *hist_cnt = side.hist_cnt;
    if (skipped(a, row)) return;
    const RowRule r = row_rule(a, row);
    if (r.greedy) return;
    SampleRow &st = state[row];
    if (!(r.has_k || r.has_p)) {
        if (stage == 1 && t == 0) {
            st.kt = 0;
            st.bin = -1;
        }
        return;
    }
    // everything this stage reads of the row's state, before any lane writes to it
    const int bin = stage == 1 ? -1 : st.bin, for_p = stage == 1 ? 0 : st.for_p;
    if (stage > 1 && bin < 0) return;
    const u64 base = stage == 1 ? 0 : st.base, target = stage == 1 ? 0 : st.target;
    const unsigned need = stage == 1 ? 0 : st.need;
    const u64 above_here = stage == 1 ? 0 : st.above[t], above_next = stage == 1 || t == 255 ? 0 : st.above[t + 1];

    u64 mass = 0;
    unsigned cnt = 0;
    for (int c = 0; c < parts; ++c) {
        const long long at = ((long long)row * parts + c) * 256 + t;
        mass += hist_mass[at];
        cnt += hist_cnt[at];
    }
    // suffix sums: bin t and every bin above it
    s_m[t] = mass;
    s_c[t] = cnt;
    if (t == 0) {
        s_m[256] = 0;
        s_c[256] = 0;
        s_bin = -1;
    }
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const u64 m2 = t + off < 256 ? s_m[t + off] : 0;
        const unsigned c2 = t + off < 256 ? s_c[t + off] : 0;
        __syncthreads();
        s_m[t] += m2;
        s_c[t] += c2;
        __syncthreads();
    }
    const u64 sm = s_m[t], sm_next = s_m[t + 1];
    const unsigned sc = s_c[t], sc_next = s_c[t + 1];

    if (stage == 1) {
        st.above[t] = sm;
        if (r.has_k) {
            if (SMP_CROSSES(sc, sc_next, (unsigned)r.k)) {
                st.bin = t;
                st.for_p = 0;
                st.need = (unsigned)r.k - sc_next;
                st.base = sm_next;
            }
        } else {                                                                    // top-p alone: Z_k is the whole row
            const u64 tgt = max((u64)((double)r.p * (double)s_m[0]), 1ull);
            if (SMP_CROSSES(sm, sm_next, tgt)) {
                st.bin = t;
                st.for_p = 1;
                st.base = sm_next;
                st.target = tgt;
            }
        }
        return;
    }
    if (for_p) {                                                                    // top-p's own bin: the threshold is final
        if (SMP_CROSSES(base + sm, base + sm_next, target)) {
            st.kt = (unsigned)bin << 8 | (unsigned)t;
            st.bin = -1;
        }
        return;
    }
    // top-k's bin: its threshold key and Z_k
    if (SMP_CROSSES(sc, sc_next, need)) {
        s_zk = base + sm;
        if (!r.has_p) {
            st.kt = (unsigned)bin << 8 | (unsigned)t;
            st.bin = -1;
        }
    }
    if (!r.has_p) return;
    __syncthreads();
    // top-p over the classes top-k kept.  above[bin] >= Z_k >= the target, so its bin is top-k's or a higher one
    const u64 tgt = max((u64)((double)r.p * (double)s_zk), 1ull);
    if (SMP_CROSSES(above_here, above_next, tgt)) s_bin = t;
    __syncthreads();
    const int pbin = s_bin;
    if (pbin != bin) {                                                              // a higher bin: one more level-2 sweep
        if (t == 0) {
            st.bin = pbin;
            st.for_p = 1;
            st.base = pbin == 255 ? 0 : st.above[pbin + 1];
            st.target = tgt;
        }
    } else if (SMP_CROSSES(base + sm, base + sm_next, tgt)) {                       // the same bin: at top-k's low byte the mass is Z_k
        st.kt = (unsigned)bin << 8 | (unsigned)t;
        st.bin = -1;
    }
}

// grid (parts, rows): the kept mass of a part
__global__ __launch_bounds__(SMP_THREADS) void sample_mass_kernel(SampleParams a, const SampleRow *__restrict__ state,
                                                                  u64 *__restrict__ part_mass) {
    __shared__ u64 s_sum[SMP_THREADS / 64];
    const int t = threadIdx.x, row = blockIdx.y, lo = blockIdx.x * MM_ARGMAX_CHUNK;
    const RowRule r = row_rule(a, row);
    if (r.greedy) return;
    const unsigned kt = state ? state[row].kt : 0u;
    u64 sum = 0;
    for_each_in_part(a.logits + (long long)row * a.ld + lo, min(a.vocab - lo, MM_ARGMAX_CHUNK), t,
                     [&](unsigned bits) { sum += kept_mass(bits, kt, r); });
    sum = wave_sum(sum);
    if ((t & 63) == 0) s_sum[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < SMP_THREADS / 64; ++w) sum += s_sum[w];
        part_mass[(long long)row * gridDim.x + blockIdx.x] = sum;
    }
}

// grid rows: Z, the part in which the prefix passes u * Z, and the column inside it.  A lane takes SMP_RUN consecutive columns
__global__ __launch_bounds__(SMP_THREADS) void sample_draw_kernel(SampleParams a, const float *__restrict__ u, int parts,
                                                                  const SampleRow *__restrict__ state, const u64 *__restrict__ part_mass,
                                                                  int *out /* == a.out */) {
    __shared__ u64 s_scan[SMP_THREADS];
    const int t = threadIdx.x, row = blockIdx.x;
    const RowRule r = row_rule(a, row);
    if (r.greedy) return;                                                           // out[row] holds the argmax already
    const unsigned kt = state ? state[row].kt : 0u;
    const float ur = clamp_u(u[row]);                                               // NaN -> 0
    u64 Z = 0;
    for (int c = 0; c < parts; ++c) Z += part_mass[(long long)row * parts + c];
    u64 want = sample_want(ur, Z);                                                  // < Z: the prefix passes it inside the row
    int part = 0;
    for (int c = 0; c < parts; ++c) {
        const u64 s = part_mass[(long long)row * parts + c];
        if (want < s) {
            part = c;
            break;
        }
        want -= s;
    }
    const int lo = part * MM_ARGMAX_CHUNK + t * SMP_RUN;
    const uint16_t *p = a.logits + (long long)row * a.ld;
    u64 W[SMP_RUN], sum = 0;
#pragma unroll
    for (int j = 0; j < SMP_RUN; ++j) {
        W[j] = lo + j < a.vocab ? kept_mass(p[lo + j], kt, r) : 0ull;
        sum += W[j];
    }
    s_scan[t] = sum;
    __syncthreads();
    for (int off = 1; off < SMP_THREADS; off <<= 1) {                               // inclusive prefix sums over the lanes
        const u64 below = t >= off ? s_scan[t - off] : 0;
        __syncthreads();
        s_scan[t] += below;
        __syncthreads();
    }
    u64 run = s_scan[t] - sum;
    if (run <= want && want < s_scan[t]) {                                          // one lane: the prefix passes `want` in its columns
#pragma unroll
        for (int j = 0; j < SMP_RUN; ++j) {
            const bool before = run <= want;
            run += W[j];
            if (before && want < run) out[row] = lo + j;
        }
    }
}

struct SampleWorkspace {
    size_t argmax, part_mass, state, hist_mass, hist_cnt, total;
};

static SampleWorkspace sample_layout(int rows, int vocab) {
    const size_t parts = (size_t)argmax_parts(vocab), n = (size_t)rows * parts;
    SampleWorkspace w;
    w.argmax = 0;
    w.part_mass = w.argmax + n * sizeof(u64);
    w.state = w.part_mass + n * sizeof(u64);
    w.hist_mass = w.state + (size_t)rows * sizeof(SampleRow);
    w.hist_cnt = w.hist_mass + n * 256 * sizeof(u64);
    w.total = w.hist_cnt + n * 256 * sizeof(unsigned);
    return w;
}

size_t sample_workspace_bytes(int rows, int vocab) { return sample_layout(rows, vocab).total; }

hipError_t launch_sample_select(const SelectSide &first, const SelectSide *second, int rows, int parts, hipStream_t stream) {
    const int sides = second ? 2 : 1;
    const SelectSide &other = second ? *second : first;
    for (int stage = 1; stage <= 3; ++stage) {
        sample_hist_kernel<<<dim3(parts, rows, sides), SMP_THREADS, 0, stream>>>(first, other, stage == 1 ? 1 : 2);
        sample_finish_kernel<<<dim3(rows, sides), 256, 0, stream>>>(first, other, stage, parts);
    }
    return hipGetLastError();
}

hipError_t launch_sample_rows(const void *logits, int rows, int vocab, long long ld, const float *u, const float *temperature,
                              const int *top_k, const float *top_p, const float *min_p, int *out, void *ws, hipStream_t stream) {
    const int parts = argmax_parts(vocab);
    const SampleWorkspace w = sample_layout(rows, vocab);
    char *base = (char *)ws;
    u64 *part_mass = (u64 *)(base + w.part_mass), *hist_mass = (u64 *)(base + w.hist_mass);
    unsigned *hist_cnt = (unsigned *)(base + w.hist_cnt);
    SampleRow *state = top_k || top_p ? (SampleRow *)(base + w.state) : nullptr;
    hipError_t e = launch_argmax_rows(logits, rows, vocab, ld, out, base + w.argmax, stream);
    if (e != hipSuccess) return e;
    const SampleParams a{(const uint16_t *)logits, ld, vocab, out, temperature, top_p, min_p, top_k, nullptr};
    const dim3 grid(parts, rows);
    if (state) {
        e = launch_sample_select(SelectSide{a, state, hist_mass, hist_cnt}, nullptr, rows, parts, stream);
        if (e != hipSuccess) return e;
    }
    sample_mass_kernel<<<grid, SMP_THREADS, 0, stream>>>(a, state, part_mass);
    sample_draw_kernel<<<rows, SMP_THREADS, 0, stream>>>(a, u, parts, state, part_mass, out);
    return hipGetLastError();
}

}  // namespace mm
