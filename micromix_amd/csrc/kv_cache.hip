// Paged KV cache: append (int4 or fp8 quantize, or bf16 copy) and GQA split-KV decode attention (include/micromix_hip.h, mm_kv_append /
// mm_paged_decode).  Layout and parameter convention of the reference's vendored FlashInfer cache (flashinfer/page.cuh:15,75-103,
// quantization.cuh:60-80); the quantization rule is quantize_int_group(x, 4, 128) (model/qLlamaLayer.py:13-23) with fp16 parameters.
//
//   kv_data  int4: uint8 [max_pages, L, 2, Hkv, P, 64]  (byte j = element 2j low nibble | element 2j+1 high nibble)
//            bf16: bf16  [max_pages, L, 2, Hkv, P, 128]
//            fp8:  uint8 [max_pages, L, 2, Hkv, P, 128] (OCP e4m3fn codes, element j in byte j)
//   kv_param int4 and fp8: fp16 [max_pages, L, 2, Hkv, P, 2] = (scale, zero);  value = decode(code) * scale - zero
//            (fp8: scale = 2^e, the smallest e in [-14, 15] with amax <= 448 * 2^e, and zero = +0.0)
//
// Decode: one workgroup (4 waves) per (sequence, kv head, chunk of tokens) handles all g = Hq / Hkv query heads of that kv head, so every
// cache byte is read once.  Each wave walks 32-token tiles of the chunk:
//   scores  one v_mfma_f32_16x16x32_bf16 chain per 16 tokens: A = q (16 head rows, g used), B = the K codes as bf16 (16 + code, exact),
//           so q.k = s * (q.(16 + c)) - (16 s + z) * sum(q);  for the bf16 cache B is the K row itself;  fp8: B = the codes widened to
//           bf16 (exact, one v_cvt_scalef32_pk_bf16_fp8 per two), q.k = s * (q.code): the power-of-two s moves no rounding
//   softmax online, in the log2 domain, the max across the tile's 16 token lanes, l and sum(p z) as per-lane partials
//   p.V     VALU, fp32: a lane owns 8 dims of 8 tokens of the tile, acc[h][8] += (p s_v)[h] * code  (minus sum(p z_v) once at the end;
//           fp8: the codes by v_cvt_pk_f32_fp8, no z)
// The waves merge through LDS; with one chunk the workgroup writes o, otherwise (m, l, o) partials that mm_paged_decode's merge kernel
// combines.
// Sliding window (mm_paged_decode_window, the WINDOW kernels): the walk starts at token max(0, len - W) instead of at token 0 and the
// chunks are laid over the W tokens from there, so a long sequence costs its window; the un-windowed kernels are the WINDOW = false
// instantiations, instruction for instruction what they were.
// Shared prefix (mm_paged_decode_shared, the prefix / tail kernels): sequences that hold their leading pages in common (PagedKVCache.fork)
// put their queries into one A operand -- row c is member c / g, head c % g of a slab of floor(16 / g) members -- and one walk over the
// shared tokens serves them all; each sequence's own tail is walked as before, from its shared count on; both always leave partials and
// the merge kernel combines the ncA + ncB of a (sequence, query head).  All four walks are one tile loop, kv_decode_tiles.inc.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

#include "mx_kernels.h"
#include "mx_kv_shared_host.h"
#include "mx_paged_kv.h"

namespace {

using namespace mm::kv;       // the page-table walk, the append rule, the int4 decoding and the chunk merge
using mm::PagedKV;

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int DEC_WAVES = 4;
constexpr int TILE = 32;           // tokens per wave iteration

// One workgroup per appended token and kv head; wave 0 writes K, wave 1 writes V (the slot and the int4 rule: mx_paged_kv.h).
template <int KIND>
__global__ __launch_bounds__(128) void kv_append_kernel(const PagedKV kv, const uint16_t *__restrict__ k, const uint16_t *__restrict__ v,
                                                        const int *__restrict__ append_indptr) {
    const int i = blockIdx.x, h = blockIdx.y, which = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = append_row(kv, append_indptr, i, which, h);
    if (row < 0) return;
    const uint32_t two = ((const uint32_t *)((which ? v : k) + ((int64_t)i * kv.Hkv + h) * HD))[lane];   // elements 2 lane, 2 lane + 1
    store_row<KIND>(kv, row, lane, two);
}

struct DecodeArgs {
    PagedKV kv;
    const uint16_t *q;
    float *ws;                 // partials: o [B, Hkv, nc, g, 128], then (m, l) [B, Hkv, nc, g, 2]
    uint16_t *o;
    int Hq, g, nc, chunk;
    float scale_log2;          // sm_scale * log2(e)
    int window;                // WINDOW kernels: the query attends its last `window` >= 1 tokens (itself included)
};

// mm_paged_decode_shared: d is what the tile loop and the merge kernel take, with d.nc = ncA + ncB, the partials of a (sequence, query
// head) -- prefix chunks first, then tail chunks, one stride; d.chunk and d.window are unused
struct SharedArgs {
    DecodeArgs d;
    const int *group_indptr, *group_members, *shared_len;
    int ncA, chunkA, ncB, chunkB;
};

// What a workgroup walks, and for whom:
//   WALK_ALL     sequence b = blockIdx.z, tokens [0, len_b), its g heads
//   WALK_WINDOW  sequence b, tokens [lo_b, len_b), lo_b = max(0, len_b - window), chunk c from lo_b + c * chunk on.  The tiles start at
//                lo_b itself -- a lane addresses its token's row on its own, so a tile need not start on a multiple of 32 -- and no token
//                below the window is ever looked at: no compare, no page-table read, the span exactly min(len_b, window) tokens
//   WALK_PREFIX  slot s = blockIdx.z of group_members: live when it is the first of a slab, i.e. a multiple of per = 16 / g positions
//                into its group; the slab is the group's members from s on, at most per.  Row c of the A operand is member c / g,
//                head c % g; the walk is [0, min(shared_len, len)) of the slab's first member, over that member's page list.  Always
//                partials, every row's to its own (sequence, query head, chunk).  A dead slot returns having read the group table only
//   WALK_SUFFIX  sequence b, tokens [min(shared_len[b], len_b), len_b), the WINDOW shape with the begin read from shared_len.  Always
//                partials, behind the ncA prefix chunks
// A member index outside [0, B) is a row without a query and without an output; a bad first member makes the slab's walk empty.
enum { WALK_ALL = 0, WALK_WINDOW = 1, WALK_PREFIX = 2, WALK_SUFFIX = 3 };

template <int KIND, int GP, bool WINDOW>
__global__ __launch_bounds__(256) void paged_decode_kernel(const DecodeArgs a) {
    constexpr int WALK = WINDOW ? WALK_WINDOW : WALK_ALL;
    const SharedArgs sh = {};                          // no shared walk here: the branches that read it are discarded
#include "kv_decode_tiles.inc"
}

// the prefix walk always runs the 16-row accumulator set: its rows are the slab's members, not one sequence's heads
template <int KIND>
__global__ __launch_bounds__(256) void paged_decode_prefix_kernel(const SharedArgs sh) {
    constexpr int WALK = WALK_PREFIX, GP = 16;
    const DecodeArgs &a = sh.d;
#include "kv_decode_tiles.inc"
}

template <int KIND, int GP>
__global__ __launch_bounds__(256) void paged_decode_suffix_kernel(const SharedArgs sh) {
    constexpr int WALK = WALK_SUFFIX;
    const DecodeArgs &a = sh.d;
#include "kv_decode_tiles.inc"
}

// combines the nc chunk partials of one (sequence, query head)
__global__ __launch_bounds__(64) void paged_decode_merge_kernel(const DecodeArgs a) {
    const int hq = blockIdx.x, b = blockIdx.y, kvh = hq / a.g, h = hq % a.g, d = 2 * threadIdx.x;
    const int64_t first = (((int64_t)b * a.kv.Hkv + kvh) * a.nc) * a.g + h;      // part index of chunk 0; chunk stride g
    float o[2];
    merge_chunks<2>(a.ws + (int64_t)a.kv.B * a.Hq * a.nc * HD, a.ws + d, first, a.g, a.nc, o);
    *(uint32_t *)(a.o + ((int64_t)b * a.Hq + hq) * HD + d) = pack_bf(o[0], o[1]);
}

template <int KIND, bool WINDOW>
hipError_t launch_decode_g(const DecodeArgs &a, hipStream_t stream) {
    const dim3 grid(a.nc, a.kv.Hkv, a.kv.B);
    if (a.g <= 4) paged_decode_kernel<KIND, 4, WINDOW><<<grid, 256, 0, stream>>>(a);
    else if (a.g <= 8) paged_decode_kernel<KIND, 8, WINDOW><<<grid, 256, 0, stream>>>(a);
    else paged_decode_kernel<KIND, 16, WINDOW><<<grid, 256, 0, stream>>>(a);
    return hipGetLastError();
}

template <int KIND>
hipError_t launch_shared_g(const SharedArgs &s, hipStream_t stream) {
    const PagedKV &kv = s.d.kv;
    paged_decode_prefix_kernel<KIND><<<dim3(s.ncA, kv.Hkv, kv.B), 256, 0, stream>>>(s);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const dim3 grid(s.ncB, kv.Hkv, kv.B);
    if (s.d.g <= 4) paged_decode_suffix_kernel<KIND, 4><<<grid, 256, 0, stream>>>(s);
    else if (s.d.g <= 8) paged_decode_suffix_kernel<KIND, 8><<<grid, 256, 0, stream>>>(s);
    else paged_decode_suffix_kernel<KIND, 16><<<grid, 256, 0, stream>>>(s);
    return hipGetLastError();
}

}  // namespace

namespace mm {

void kv_chunks(long long work, int target_workgroups, int max_seq_len, int round_to, int *nc, int *chunk) {
    if (work < 1) work = 1;
    const long long want = (target_workgroups + work - 1) / work;
    const int most = (max_seq_len + 255) / 256;
    int n = want < most ? (int)want : most;
    if (n < 1) n = 1;
    int cl = (max_seq_len + n - 1) / n;
    cl = (cl + round_to - 1) / round_to * round_to;
    if (cl < round_to) cl = round_to;
    *chunk = cl;
    *nc = max_seq_len > 0 ? (max_seq_len + cl - 1) / cl : 1;
}

int kv_window_span(int max_seq_len, int window, int slack) {
    return window > 0 && (long long)window + slack < max_seq_len ? window + slack : max_seq_len;
}

void kv_decode_split(int B, int Hkv, int max_seq_len, int window, int *nc, int *chunk) {
    // two workgroups per CU of the 256 on an MI355X; a chunk gives every wave whole tiles.  A window's range is the window: no slack
    kv_chunks((long long)B * Hkv, 512, kv_window_span(max_seq_len, window, 0), TILE * DEC_WAVES, nc, chunk);
}

size_t kv_decode_workspace_bytes(int B, int Hq, int Hkv, int max_seq_len, int window) {
    int nc, chunk;
    kv_decode_split(B, Hkv, max_seq_len, window, &nc, &chunk);
    return nc > 1 ? (size_t)B * Hq * nc * (HD + 2) * sizeof(float) : 0;     // DecodeArgs::ws
}

hipError_t launch_kv_append(const PagedKV &kv, const void *k, const void *v, const int *append_indptr, int T, hipStream_t stream) {
    const dim3 grid(T, kv.Hkv);
    if (kv.kind == KV_INT4) kv_append_kernel<KV_INT4><<<grid, 128, 0, stream>>>(kv, (const uint16_t *)k, (const uint16_t *)v, append_indptr);
    else if (kv.kind == KV_FP8) kv_append_kernel<KV_FP8><<<grid, 128, 0, stream>>>(kv, (const uint16_t *)k, (const uint16_t *)v, append_indptr);
    else kv_append_kernel<KV_BF16><<<grid, 128, 0, stream>>>(kv, (const uint16_t *)k, (const uint16_t *)v, append_indptr);
    return hipGetLastError();
}

hipError_t launch_paged_decode(const PagedKV &kv, const void *q, int Hq, int max_seq_len, int window, float sm_scale, void *ws, void *o,
                               hipStream_t stream) {
    DecodeArgs a;
    a.kv = kv;
    a.q = (const uint16_t *)q;
    a.ws = (float *)ws;
    a.o = (uint16_t *)o;
    a.Hq = Hq;
    a.g = Hq / kv.Hkv;
    kv_decode_split(kv.B, kv.Hkv, max_seq_len, window, &a.nc, &a.chunk);
    a.scale_log2 = kv_scale_log2(sm_scale);
    a.window = window;
    hipError_t e;
    if (kv.kind == KV_INT4) e = window > 0 ? launch_decode_g<KV_INT4, true>(a, stream) : launch_decode_g<KV_INT4, false>(a, stream);
    else if (kv.kind == KV_FP8) e = window > 0 ? launch_decode_g<KV_FP8, true>(a, stream) : launch_decode_g<KV_FP8, false>(a, stream);
    else e = window > 0 ? launch_decode_g<KV_BF16, true>(a, stream) : launch_decode_g<KV_BF16, false>(a, stream);
    if (e != hipSuccess || a.nc == 1) return e;
    paged_decode_merge_kernel<<<dim3(Hq, kv.B), 64, 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t launch_paged_decode_shared(const PagedKV &kv, const void *q, int Hq, const int *group_indptr, const int *group_members,
                                      const int *shared_len, int max_shared_len, int max_suffix_len, float sm_scale, void *ws, void *o,
                                      hipStream_t stream) {
    const KvSharedSplit sp = kv_shared_split(kv.B, Hq, kv.Hkv, max_shared_len, max_suffix_len);
    SharedArgs s;
    s.d.kv = kv;
    s.d.q = (const uint16_t *)q;
    s.d.ws = (float *)ws;
    s.d.o = (uint16_t *)o;
    s.d.Hq = Hq;
    s.d.g = Hq / kv.Hkv;
    s.d.nc = sp.ncA + sp.ncB;
    s.d.chunk = 0;
    s.d.scale_log2 = kv_scale_log2(sm_scale);
    s.d.window = 0;
    s.group_indptr = group_indptr;
    s.group_members = group_members;
    s.shared_len = shared_len;
    s.ncA = sp.ncA;
    s.chunkA = sp.chunkA;
    s.ncB = sp.ncB;
    s.chunkB = sp.chunkB;
    hipError_t e;
    if (kv.kind == KV_INT4) e = launch_shared_g<KV_INT4>(s, stream);
    else if (kv.kind == KV_FP8) e = launch_shared_g<KV_FP8>(s, stream);
    else e = launch_shared_g<KV_BF16>(s, stream);
    if (e != hipSuccess) return e;
    paged_decode_merge_kernel<<<dim3(Hq, kv.B), 64, 0, stream>>>(s.d);
    return hipGetLastError();
}

}  // namespace mm
