// One step of the paged KV cache's allocator on the device (mm_kv_step, include/micromix_kvstep.h, which states the rule and the layout of
// the state): every sequence is shortened behind the tokens it keeps, the pages past them go back to the free stack, the next tokens get
// pages from it, and the page table is rewritten in place -- what PagedKVCache's accept + extend do on the host, page numbers included.
//
// kv_step_kernel is ONE workgroup with a sequence to a lane.  The host loops are sequential -- sequence b's pushes land above those of
// the sequences before it, its pops take what they left -- so a sequence's place in the stack is an exclusive prefix sum over the lanes
// (within a wave by shuffles, across the waves through 16 words of LDS per scan), and each lane then loops over its own pushes and pops: no atomic
// places a page, the same tables on every run (the one atomic is an integer OR in LDS that collects which conditions were met).  The whole step is evaluated first; a condition of the header ends it with status set and nothing else
// written.  All pushes are stored before a barrier and all pops read after it, since a pop may take a page pushed in the same step.
// kv_step_tables_kernel, over (sequence, chunk), copies the padded master lists into kv_indices at their new offsets and writes token_pos;
// it does nothing unless the step succeeded (status is then still 0).
#include "mx_kernels.h"
#include "../../include/micromix_kvstep.h"

namespace mm {

constexpr int STEP_WAVES = MM_KV_STEP_MAX_BATCH / 64, STEP_HDR = MM_KV_STEP_HEADER_INTS, TABLE_THREADS = 256, TABLE_CHUNKS = 8;

__device__ inline int ceil_div_nonneg(long long x, int P) { return (int)(x / P) + (x % P != 0); }

// the exclusive prefix sum of v over the lanes of the workgroup (a multiple of 64 of them) and, in *total, the sum of all: two barriers
template <typename T>
__device__ inline T block_scan(T v, T *lds, T *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T below = __shfl_up(inc, d);
        if (lane >= d) inc += below;
    }
    __syncthreads();                                          // the words are free: every lane has read the previous scan's
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    T before = 0, all = 0;
    for (int w = 0; w < waves; ++w) {
        const T t = lds[w];
        before += w < wave ? t : 0;
        all += t;
    }
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(MM_KV_STEP_MAX_BATCH) void kv_step_kernel(const KVStep s) {
    __shared__ int lds[STEP_WAVES];                           // the wave totals of a scan: one array for each type scanned
    __shared__ long long lds_tokens[STEP_WAVES];
    __shared__ int met_lds;
    int *st = s.state;
    const int status = st[0], steps = st[1], fc = st[2];
    if (status != 0) return;                                  // sticky: uniform, before any barrier
    const int B = s.B, P = s.P, b = threadIdx.x;
    const bool live = b < B;
    int *seq_len = st + STEP_HDR, *announced = seq_len + B, *num_pages = announced + B, *stack = num_pages + B;
    int *pg = stack + s.max_pages + (live ? (long long)b * s.pps : 0);

    int sl = 0, an = 0, np = 0, nn = 0, k = 0, err = 0, kept = 0, keep_pages = 0, fin_pages = 0;
    long long fin = 0;
    if (live) {
        sl = seq_len[b], an = announced[b], np = num_pages[b], nn = s.next_new[b];
        k = s.keep ? s.keep[(long long)b * s.keep_stride] : an;
        if (sl < 0 || an < 0 || an > sl || np > s.pps || np != ceil_div_nonneg(sl, P)) err = MM_KV_STEP_BAD_STATE;
        else if (k < 0 || k > an) err = MM_KV_STEP_BAD_KEEP;
        else if (nn < 0) err = MM_KV_STEP_BAD_NEXT;
        else {
            kept = sl - an + k;
            keep_pages = ceil_div_nonneg(kept, P);
            fin = (long long)kept + nn;
            if (fin > s.max_seq_len) err = MM_KV_STEP_TOO_LONG;
            else if ((fin_pages = ceil_div_nonneg(fin, P)) > s.pps) err = MM_KV_STEP_SEQ_PAGES;
        }
    }
    // the conditions of a sequence: the smallest value any of them met (__syncthreads_or would only say that one was met).  An integer
    // OR in LDS: whatever the order, the same word
    if (b == 0) met_lds = 0;
    __syncthreads();
    if (err) atomicOr(&met_lds, 1 << err);
    __syncthreads();
    const int met = met_lds;
    if (met) {
        if (b == 0) st[0] = __ffs(met) - 1, st[3] = steps;
        return;
    }
    const int push = live ? np - keep_pages : 0, need = live ? fin_pages - keep_pages : 0;      // both >= 0: keep_pages <= np, kept <= fin
    int pushes, pops, entries;
    long long tokens;
    const int push_at = block_scan<int>(push, lds, &pushes);
    const int pop_at = block_scan<int>(need, lds, &pops);
    const int first = block_scan<int>(fin_pages, lds, &entries);
    const long long tok_at = block_scan<long long>(nn, lds_tokens, &tokens);

    int bad = 0;                                              // the conditions of the step, uniform
    if (fc < 0 || (long long)fc + pushes > s.max_pages) bad = MM_KV_STEP_BAD_STATE;
    else if (tokens != s.T) bad = MM_KV_STEP_BAD_SUM;
    else if (pops > fc + pushes) bad = MM_KV_STEP_OUT_OF_PAGES;
    else if (entries > s.capacity) bad = MM_KV_STEP_INDICES_CAPACITY;
    if (bad) {
        if (b == 0) st[0] = bad, st[3] = steps;
        return;
    }

    for (int t = 0; t < push; ++t) stack[fc + push_at + t] = pg[np - 1 - t];       // the highest entry first
    __syncthreads();                                          // every push is in the stack before the first pop reads it
    const int top = fc + pushes;
    if (live) {
        for (int t = 0; t < need; ++t) pg[keep_pages + t] = stack[top - 1 - pop_at - t];
        seq_len[b] = (int)fin, announced[b] = nn, num_pages[b] = fin_pages;
        s.kv_indptr[b] = first;
        s.last_page_len[b] = fin ? (int)(fin - (long long)(fin_pages - 1) * P) : 0;
        s.append_indptr[b] = (int)tok_at;
        if (b == B - 1) s.kv_indptr[B] = entries, s.append_indptr[B] = (int)tokens;
    }
    if (b == 0) st[1] = steps + 1, st[2] = top - pops;
}

__global__ __launch_bounds__(TABLE_THREADS) void kv_step_tables_kernel(const KVStep s) {
    const int *st = s.state;
    if (st[0] != 0) return;                                   // this step, or an earlier one, failed: the tables stay
    const int B = s.B, b = blockIdx.x, at = blockIdx.y * TABLE_THREADS + threadIdx.x, stride = gridDim.y * TABLE_THREADS;
    const int *seq_len = st + STEP_HDR, *announced = seq_len + B, *num_pages = announced + B;
    const int *pg = num_pages + B + s.max_pages + (long long)b * s.pps;
    const int np = num_pages[b], first = s.kv_indptr[b];
    for (int j = at; j < np; j += stride) s.kv_indices[first + j] = pg[j];
    if (s.token_pos) {
        const int n = announced[b], t0 = s.append_indptr[b], base = seq_len[b] - n;
        for (int i = at; i < n; i += stride) s.token_pos[t0 + i] = base + (s.depths ? s.depths[t0 + i] : i);
    }
}

hipError_t launch_kv_step(const KVStep &s, hipStream_t stream) {
    kv_step_kernel<<<1, (s.B + 63) / 64 * 64, 0, stream>>>(s);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const int widest = s.pps > s.T ? s.pps : s.T;
    int chunks = (widest + TABLE_THREADS - 1) / TABLE_THREADS;
    chunks = chunks < 1 ? 1 : chunks > TABLE_CHUNKS ? TABLE_CHUNKS : chunks;
    kv_step_tables_kernel<<<dim3(s.B, chunks), TABLE_THREADS, 0, stream>>>(s);
    return hipGetLastError();
}

}  // namespace mm
