// Speculative sampling of chain drafts (mm_spec_sample_rows, include/micromix_spec.h): per row, accept the draft's candidate token x
// against its own odds, min(1, p(x) / q(x)), or redraw from norm(max(0, p - q)) -- with p and q the kept distributions mm_sample_rows
// draws from, as integer masses P_i / Z_p and Q_i / Z_q (mx_row_weights.h, mx_sample_select.h).  The accept test and the residual
// R_i = max(0, P_i Z_q - Q_i Z_p) are formed exactly, in 128-bit integers (mx_spec_rule.h): every sum is the same number in any order, so
// the result is a function of the inputs alone.  There are no float atomics and no tickets, and every workspace word a kernel reads was
// stored by an earlier kernel of the same call.
//
// The launches of one call, each on the whole batch, a row's workgroups leaving at once where the row has nothing to do there.  A draft
// row without a candidate is never read:
//   argmax_rows (verify.hip)   both matrices in one launch (two when a row has several parts): out[r] = the target row's argmax -- the
//                              greedy answer, the fallback, and m for every kernel below -- and the draft row's, in the workspace
//   select (sample.hip)        the threshold keys of the target rows and of the draft rows, both matrices in the same hist / finish x 3;
//                              left out when top_k and top_p are both null
//   mass                       the kept mass of every part of both matrices
//   residual                   every workgroup of a row decides for itself -- Z_p, Z_q, P_x, Q_x, the greedy answer, the accept test:
//                              the same integers, so the same decision -- and the row's first one records it; a rejected row's
//                              workgroups then sum the residual mass of their part, two 64-bit words
//   draw                       accepted rows: out[r] = x.  Rejected rows: ZR, the part that holds mulshift(ZR, U_r) and the column
//                              inside it.  Rows without a candidate: mm_sample_rows' draw from P with its own 64-bit place
// out[] is written by the first launches and by the last only: in between it is the target's argmax for every reader.
#include "../../include/micromix_spec.h"
#include "mx_argmax_key.h"
#include "mx_kernels.h"
#include "mx_row_weights.h"
#include "mx_sample_select.h"
#include "mx_spec_rule.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

enum : int { SPEC_GREEDY = 0, SPEC_ACCEPT = 1, SPEC_PLAIN = 2, SPEC_RESIDUAL = 3, SPEC_RESIDUAL_ONE_HOT = 4 };

// a row's decision
struct SpecRow {
    u64 Zp, Zq;              // the kept masses of the target and the draft row (one-hot: Zq = 1)
    int mode;                // SPEC_GREEDY: out[r] holds the answer; SPEC_ACCEPT: it is x; SPEC_PLAIN: draw from P; SPEC_RESIDUAL*: from R
    int x;                   // the candidate
    int accepted;            // what accepted[r] reports
    int pad;
};
static_assert(sizeof(SpecRow) % 8 == 0, "the arrays behind the row states hold 64-bit words");

struct SpecParams {
    SampleParams p, q;       // the target rows and the draft rows (q.logits null: one-hot drafts); q.cand is cand
    const SampleRow *state_p, *state_q;   // null without top_k and top_p: every key is kept
    const int *cand;
    const u64 *mass_p, *mass_q;           // the kept mass of every part, by the mass kernel
    int parts;
};

__device__ inline u128 wave_sum128(u128 x) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const u64 lo = (u64)__shfl_xor((long long)(u64)x, off), hi = (u64)__shfl_xor((long long)(u64)(x >> 64), off);
        x += (u128)hi << 64 | lo;
    }
    return x;
}

// grid (parts, rows, 1 or 2): the kept mass of a part of the target row (z = 0) or of the draft row (z = 1)
__global__ __launch_bounds__(SMP_THREADS) void spec_mass_kernel(SpecParams a, u64 *__restrict__ mass_p, u64 *__restrict__ mass_q) {
    __shared__ u64 s_sum[SMP_THREADS / 64];
    const int t = threadIdx.x, row = blockIdx.y, lo = blockIdx.x * MM_ARGMAX_CHUNK;
    const bool draft = blockIdx.z != 0;
    const SampleParams &m = draft ? a.q : a.p;
    if (skipped(m, row)) return;
    const RowRule r = row_rule(m, row);
    if (r.greedy) return;
    const SampleRow *state = draft ? a.state_q : a.state_p;
    const unsigned kt = state ? state[row].kt : 0u;
    u64 sum = 0;
    for_each_in_part(m.logits + (long long)row * m.ld + lo, min(m.vocab - lo, MM_ARGMAX_CHUNK), t,
                     [&](unsigned bits) { sum += kept_mass(bits, kt, r); });
    sum = wave_sum(sum);
    if ((t & 63) == 0) s_sum[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < SMP_THREADS / 64; ++w) sum += s_sum[w];
        (draft ? mass_q : mass_p)[(long long)row * gridDim.x + blockIdx.x] = sum;
    }
}

// The decision of a row, by a whole wave (every lane returns it): the sums, the two masses of the candidate, the accept test.  It reads
// what earlier launches wrote and nothing this launch writes, so every wave of every workgroup of the row arrives at the same one
__device__ inline SpecRow spec_decide(const SpecParams &a, int row, const float *__restrict__ u_accept) {
    const int lane = threadIdx.x & 63;
    SpecRow d;
    d.x = a.cand[row];
    d.Zp = 0, d.Zq = 1, d.pad = 0;
    const bool valid = in_vocab(d.x, a.p.vocab);
    const RowRule rp = row_rule(a.p, row);
    if (rp.greedy) {                                                                // out[row] holds the argmax
        d.mode = SPEC_GREEDY;
        d.accepted = valid ? (a.p.out[row] == d.x ? 1 : 0) : -1;
        return d;
    }
    for (int c = lane; c < a.parts; c += 64) d.Zp += a.mass_p[(long long)row * a.parts + c];
    d.Zp = wave_sum(d.Zp);
    if (!valid) {                                                                   // the draft row is never read
        d.mode = SPEC_PLAIN;
        d.accepted = -1;
        return d;
    }
    const u64 Px = kept_mass(a.p.logits[(long long)row * a.p.ld + d.x], a.state_p ? a.state_p[row].kt : 0u, rp);
    bool one_hot = a.q.logits == nullptr;
    u64 Qx = 1;
    if (!one_hot) {
        const RowRule rq = row_rule(a.q, row);
        one_hot = rq.greedy;
        if (!one_hot) {
            d.Zq = 0;
            for (int c = lane; c < a.parts; c += 64) d.Zq += a.mass_q[(long long)row * a.parts + c];
            d.Zq = wave_sum(d.Zq);
            Qx = kept_mass(a.q.logits[(long long)row * a.q.ld + d.x], a.state_q ? a.state_q[row].kt : 0u, rq);
        }
    }
    const bool take = spec_accept(Px, d.Zp, Qx, d.Zq, spec_u24(u_accept[row]));
    d.mode = take ? SPEC_ACCEPT : one_hot ? SPEC_RESIDUAL_ONE_HOT : SPEC_RESIDUAL;
    d.accepted = take ? 1 : 0;
    return d;
}

// the masses of a rejected (or candidate-less) row as the residual and the draw kernel read them: R_i, or P_i for SPEC_PLAIN
struct SpecMasses {
    const uint16_t *p, *q;
    RowRule rp, rq;
    unsigned ktp, ktq;
    u64 Zp, Zq;
    int mode, x;

    __device__ inline SpecMasses(const SpecParams &a, const SpecRow &d, int row) : Zp(d.Zp), Zq(d.Zq), mode(d.mode), x(d.x) {
        p = a.p.logits + (long long)row * a.p.ld;
        rp = row_rule(a.p, row);
        ktp = a.state_p ? a.state_p[row].kt : 0u;
        q = nullptr, ktq = 0u, rq = RowRule{};
        if (mode == SPEC_RESIDUAL) {                                                // only here is the draft's argmax a written word
            q = a.q.logits + (long long)row * a.q.ld;
            rq = row_rule(a.q, row);
            ktq = a.state_q ? a.state_q[row].kt : 0u;
        }
    }
    __device__ inline u128 at(int col) const {
        const u64 Pi = kept_mass(p[col], ktp, rp);
        if (mode == SPEC_PLAIN) return (u128)Pi;
        const u64 Qi = mode == SPEC_RESIDUAL ? kept_mass(q[col], ktq, rq) : (col == x ? 1ull : 0ull);
        return spec_residual(Pi, Zp, Qi, Zq);
    }
};

// grid (parts, rows): the row's decision, recorded by its first workgroup, and the residual mass of a part of a rejected row.  Lane t
// takes the columns t, t + 256, ... of the part
__global__ __launch_bounds__(SMP_THREADS) void spec_residual_kernel(SpecParams a, const float *__restrict__ u_accept, SpecRow *__restrict__ rowst,
                                                                    int *__restrict__ accepted, u64 *__restrict__ res) {
    __shared__ u64 s_lo[SMP_THREADS / 64], s_hi[SMP_THREADS / 64];
    const int t = threadIdx.x, row = blockIdx.y, lo = blockIdx.x * MM_ARGMAX_CHUNK;
    const SpecRow d = spec_decide(a, row, u_accept);
    if (blockIdx.x == 0 && t == 0) {
        rowst[row] = d;
        if (accepted) accepted[row] = d.accepted;
    }
    if (d.mode != SPEC_RESIDUAL && d.mode != SPEC_RESIDUAL_ONE_HOT) return;
    const SpecMasses ms(a, d, row);
    const int len = min(a.p.vocab - lo, MM_ARGMAX_CHUNK);
    u128 sum = 0;
    for (int c = t; c < len; c += SMP_THREADS) sum += ms.at(lo + c);
    sum = wave_sum128(sum);
    if ((t & 63) == 0) {
        s_lo[t >> 6] = (u64)sum;
        s_hi[t >> 6] = (u64)(sum >> 64);
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < SMP_THREADS / 64; ++w) sum += (u128)s_hi[w] << 64 | s_lo[w];
        const long long at = ((long long)row * gridDim.x + blockIdx.x) * 2;
        res[at] = (u64)sum;
        res[at + 1] = (u64)(sum >> 64);
    }
}

// grid rows: the place in the row's mass, the part that holds it, and the column inside it.  A lane takes SMP_RUN consecutive columns
__global__ __launch_bounds__(SMP_THREADS) void spec_draw_kernel(SpecParams a, const float *__restrict__ u_resample,
                                                                const SpecRow *__restrict__ rowst, const u64 *__restrict__ res,
                                                                int *out /* == a.p.out */) {
    __shared__ u64 s_lo[SMP_THREADS], s_hi[SMP_THREADS];
    __shared__ int s_owner;
    const int t = threadIdx.x, row = blockIdx.x;
    const SpecRow d = rowst[row];
    if (d.mode == SPEC_GREEDY) return;
    if (d.mode == SPEC_ACCEPT) {
        if (t == 0) out[row] = d.x;
        return;
    }
    const SpecMasses ms(a, d, row);
    const bool plain = d.mode == SPEC_PLAIN;
    const long long first = (long long)row * a.parts;
    auto part_mass = [&](int c) -> u128 { return plain ? (u128)a.mass_p[first + c] : (u128)res[2 * (first + c) + 1] << 64 | res[2 * (first + c)]; };
    u128 want;
    if (plain) {
        want = sample_want(clamp_u(u_resample[row]), d.Zp);
    } else {
        u128 ZR = 0;
        for (int c = 0; c < a.parts; ++c) ZR += part_mass(c);
        if (ZR == 0) return;                                                        // P is Q and Q_x = 0: out[row] holds the target's argmax
        want = spec_mulshift(ZR, spec_u24(u_resample[row]));                        // < ZR: the prefix passes it inside the row
    }
    int part = 0;
    for (int c = 0; c < a.parts; ++c) {
        const u128 s = part_mass(c);
        if (want < s) {
            part = c;
            break;
        }
        want -= s;
    }
    const int lo = part * MM_ARGMAX_CHUNK + t * SMP_RUN;
    u128 sum = 0;
#pragma unroll 4
    for (int j = 0; j < SMP_RUN; ++j)
        if (lo + j < a.p.vocab) sum += ms.at(lo + j);
    if (t == 0) s_owner = 0;
    s_lo[t] = (u64)sum;
    s_hi[t] = (u64)(sum >> 64);
    __syncthreads();
    for (int off = 1; off < SMP_THREADS; off <<= 1) {                               // inclusive prefix sums over the lanes
        const u128 below = t >= off ? (u128)s_hi[t - off] << 64 | s_lo[t - off] : (u128)0;
        __syncthreads();
        const u128 mine = ((u128)s_hi[t] << 64 | s_lo[t]) + below;
        s_lo[t] = (u64)mine;
        s_hi[t] = (u64)(mine >> 64);
        __syncthreads();
    }
    const u128 upto = (u128)s_hi[t] << 64 | s_lo[t];
    if (upto - sum <= want && want < upto) s_owner = t;                             // one lane: the prefix passes `want` in its columns
    __syncthreads();
    // ... which the first wave walks, a column a lane, instead of that lane alone: an inclusive scan over the wave
    if (t >= 64) return;
    const int owner = s_owner, col = part * MM_ARGMAX_CHUNK + owner * SMP_RUN + t;
    const u128 mine = t < SMP_RUN && col < a.p.vocab ? ms.at(col) : (u128)0;
    u128 run = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 l = (u64)__shfl_up((long long)(u64)run, off), h = (u64)__shfl_up((long long)(u64)(run >> 64), off);
        if (t >= off) run += (u128)h << 64 | l;
    }
    if (owner > 0) run += (u128)s_hi[owner - 1] << 64 | s_lo[owner - 1];
    if (run - mine <= want && want < run) out[row] = col;
}

struct SpecWorkspace {
    size_t argmax_p, argmax_q, mass_p, mass_q, res, state_p, state_q, hist_mass_p, hist_mass_q, hist_cnt_p, hist_cnt_q, row, draft_arg, total;
};

static SpecWorkspace spec_layout(int rows, int vocab) {
    const size_t parts = (size_t)argmax_parts(vocab), n = (size_t)rows * parts;
    SpecWorkspace w;
    w.argmax_p = 0;
    w.argmax_q = w.argmax_p + n * sizeof(u64);
    w.mass_p = w.argmax_q + n * sizeof(u64);
    w.mass_q = w.mass_p + n * sizeof(u64);
    w.res = w.mass_q + n * sizeof(u64);
    w.state_p = w.res + 2 * n * sizeof(u64);
    w.state_q = w.state_p + (size_t)rows * sizeof(SampleRow);
    w.hist_mass_p = w.state_q + (size_t)rows * sizeof(SampleRow);
    w.hist_mass_q = w.hist_mass_p + n * 256 * sizeof(u64);
    w.hist_cnt_p = w.hist_mass_q + n * 256 * sizeof(u64);
    w.hist_cnt_q = w.hist_cnt_p + n * 256 * sizeof(unsigned);
    w.row = w.hist_cnt_q + n * 256 * sizeof(unsigned);
    w.draft_arg = w.row + (size_t)rows * sizeof(SpecRow);
    w.total = w.draft_arg + (((size_t)rows * sizeof(int) + 7) & ~(size_t)7);
    return w;
}

size_t spec_sample_workspace_bytes(int rows, int vocab) { return spec_layout(rows, vocab).total; }

hipError_t launch_spec_sample_rows(const void *logits, long long ld, const void *draft_logits, long long draft_ld, int rows, int vocab,
                                   const int *cand_tok, const float *u_accept, const float *u_resample, const float *temperature,
                                   const int *top_k, const float *top_p, const float *min_p, int *out, int *accepted, void *ws,
                                   hipStream_t stream) {
    const int parts = argmax_parts(vocab);
    const SpecWorkspace w = spec_layout(rows, vocab);
    char *base = (char *)ws;
    u64 *mass_p = (u64 *)(base + w.mass_p), *mass_q = (u64 *)(base + w.mass_q), *res = (u64 *)(base + w.res);
    SpecRow *rowst = (SpecRow *)(base + w.row);
    int *draft_arg = (int *)(base + w.draft_arg);
    const bool select = top_k || top_p, draft = draft_logits != nullptr;
    SpecParams a;
    a.p = SampleParams{(const uint16_t *)logits, ld, vocab, out, temperature, top_p, min_p, top_k, nullptr};
    a.q = SampleParams{(const uint16_t *)draft_logits, draft_ld, vocab, draft_arg, temperature, top_p, min_p, top_k, cand_tok};
    a.state_p = select ? (SampleRow *)(base + w.state_p) : nullptr;
    a.state_q = select && draft ? (SampleRow *)(base + w.state_q) : nullptr;
    a.cand = cand_tok;
    a.mass_p = mass_p;
    a.mass_q = mass_q;
    a.parts = parts;

    hipError_t e = draft ? launch_argmax_rows_pair(logits, ld, out, base + w.argmax_p, draft_logits, draft_ld, draft_arg, base + w.argmax_q, cand_tok,
                                                   rows, vocab, stream)
                         : launch_argmax_rows(logits, rows, vocab, ld, out, base + w.argmax_p, stream);
    if (e != hipSuccess) return e;
    if (select) {
        const SelectSide target{a.p, (SampleRow *)(base + w.state_p), (u64 *)(base + w.hist_mass_p), (unsigned *)(base + w.hist_cnt_p)};
        const SelectSide drafts{a.q, (SampleRow *)(base + w.state_q), (u64 *)(base + w.hist_mass_q), (unsigned *)(base + w.hist_cnt_q)};
        e = launch_sample_select(target, draft ? &drafts : nullptr, rows, parts, stream);
        if (e != hipSuccess) return e;
    }
    spec_mass_kernel<<<dim3(parts, rows, draft ? 2 : 1), SMP_THREADS, 0, stream>>>(a, mass_p, mass_q);
    spec_residual_kernel<<<dim3(parts, rows), SMP_THREADS, 0, stream>>>(a, u_accept, rowst, accepted, res);
    spec_draw_kernel<<<rows, SMP_THREADS, 0, stream>>>(a, u_resample, rowst, res, out);
    return hipGetLastError();
}

}  // namespace mm
