// Host-side launch interface between capi.hip and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "mx_launch_shape.h"

namespace mm {

// Per-device launcher state.  One process may drive several GPUs (the reference's --multi_gpu mode places the layers of ONE
// process on several devices, model/parallel_utils.py:135-156): a kernel's dynamic-LDS limit and the CU count belong to the
// device that is current at the launch, so both are cached per device id, never per process.
constexpr int MM_MAX_DEVICES = 64;
inline int current_device() {
    int d = 0;
    return (hipGetDevice(&d) == hipSuccess && d >= 0 && d < MM_MAX_DEVICES) ? d : 0;
}
inline int device_cus() {
    static std::atomic<int> cus[MM_MAX_DEVICES];
    const int dev = current_device();
    int c = cus[dev].load(std::memory_order_relaxed);
    if (c == 0) {
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
        cus[dev].store(c, std::memory_order_relaxed);
    }
    return c;
}
// raises a kernel's dynamic shared memory limit once per device (calling it twice is harmless, so no lock)
struct DynamicLdsOnce {
    std::atomic<bool> done[MM_MAX_DEVICES];
    hipError_t ensure(const void *kernel, int bytes) {
        const int dev = current_device();
        if (done[dev].load(std::memory_order_acquire)) return hipSuccess;
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess) done[dev].store(true, std::memory_order_release);
        return e;
    }
};

// Measurement hook (mm_diag_set_kernel_events): the calling thread's pair of events, both null unless registered.  The launches that
// hand them to launch_kernel -- the quantizers' and, from GemmArgs::ev_start / ev_stop, the GEMMs' -- attach them to their dispatch, so
// that their elapsed time is the kernel's own duration -- what rocprofv3's kernel trace reports -- without the launch gap that events
// around a call include.
struct DiagEvents { hipEvent_t start, stop; };
DiagEvents &diag_events();     // thread-local, defined in capi.hip

// The one launch of a kernel that keeps state per kernel: `args` are the kernel's arguments, `ev` the diagnostics events (both null:
// none).  With l.raise_to the kernel's dynamic-LDS limit is raised to it once per device before the first such launch; that state
// belongs to the kernel -- a static of this instantiation -- so no call site can pair a kernel with another kernel's flag.
template <auto Kern, class... Args>
hipError_t launch_kernel(const LaunchShape &l, hipStream_t stream, DiagEvents ev, const Args &...args) {
    static DynamicLdsOnce once;
    if (l.raise_to) {
        if (hipError_t e = once.ensure(reinterpret_cast<const void *>(Kern), l.raise_to); e != hipSuccess) return e;
    }
    if (ev.start != nullptr && ev.stop != nullptr)
        hipExtLaunchKernelGGL(Kern, dim3(l.grid_x, l.grid_y), dim3(l.threads), l.lds_bytes, stream, ev.start, ev.stop, 0, args...);
    else
        hipLaunchKernelGGL(Kern, dim3(l.grid_x, l.grid_y), dim3(l.threads), l.lds_bytes, stream, args...);
    return hipGetLastError();
}

// a kernel as a value that a generic lambda can take: decltype(k)::value is the kernel
template <auto Kern> using kernel_c = std::integral_constant<decltype(Kern), Kern>;

// resident workgroups per CU of Kern at (threads, dynamic LDS): the occupancy query costs ~1 us of host time per launch, so the last
// answer is kept per calling thread and kernel -- a static of this instantiation (a layer stack alternates between a handful of shapes)
template <auto Kern>
int resident_per_cu(int threads, size_t lds) {
    struct Entry { int dev, threads; size_t lds; int per_cu; };
    static thread_local Entry last = {};
    const int dev = current_device();
    if (last.dev == dev && last.threads == threads && last.lds == lds && last.per_cu > 0) return last.per_cu;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(Kern), threads, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    last = Entry{dev, threads, lds, per_cu};
    return per_cu;
}

constexpr int MM_MAX_SPLITS = 16;   // in-kernel split-K: splits per tile

struct GemmArgs {
    const uint8_t *X[3];    // activation segments  (AN, AS, AO)
    const uint8_t *W[3];    // weight segments      (BN, BS, BO)
    const uint8_t *SFX[3];  // activation scales
    const uint8_t *SFW[3];  // weight scales
    int K[3];
    int M, N;
    int sfx_row_tiles;      // allocated 128-row tiles in the activation SF tensors
    int sfw_row_tiles;
    int round_per_segment;
    const uint16_t *bias;   // optional [N] bf16
    uint16_t *D;            // [M, N] bf16 (out_f32 = 0)
    int out_f32;            // MM_OUT_F32: D is [M, N] fp32 instead -- the accumulator as it is, no rounding (tensor-parallel partial sums)
    float *ws;              // split-K workspace (NULL: never split), see mm_matmul_ws
    size_t ws_bytes;
    int force_split;        // MM_SPLIT_K_ALWAYS
    int n_tile0, n_tiles;   // launcher: this launch covers 256-feature tile columns [n_tile0, n_tile0 + n_tiles) (0, 0 = all)
    int splits;             // filled in by the launcher when it splits K
    int split_first[4];     // splits [split_first[i], split_first[i+1]) work on segment i
    unsigned short split_cut[MM_MAX_SPLITS + 1];   // in-kernel split-K: split q walks 128-deep K units [split_cut[q], split_cut[q+1]) of N | S | O
    unsigned short split_slot[MM_MAX_SPLITS + 1];  // ... and leaves its partial sums in slots split_slot[q] ... of its tile; [splits] = slots per tile
    unsigned long long slot_seg;    // ... two bits per slot: the segment (0 N, 1 S, 2 O) whose partial sum the slot holds
    unsigned *tickets;              // in-kernel split-K (4-wave tiles): one counter per tile at the head of the workspace, zero between launches
    int tickets_zeroed;             // MM_WS_TICKETS_ZEROED: the caller vouches for that
    // Fused gate / up epilogue (mm_gate_up_activate; launch_mx_gemm_act): W holds 2 * I rows, 128 gate features alternating with
    // the 128 up features of the same index, and a 256-feature tile quantizes silu(gate) * up of its 128 intermediate features as
    // activate_quantize_x does -- into act_o / act_sf, the operand tensors of the consumer GEMM whose K split is act_K -- instead of
    // writing D.
    int act;
    int act_K[3];
    uint8_t *act_o[3];
    uint8_t *act_sf[3];
    hipEvent_t ev_start, ev_stop;   // diagnostics only (mm_diag_set_kernel_events): recorded at the GEMM dispatch itself
    unsigned long long *clock_out;  // diagnostics only (mm_diag_set_clock_buffer): per workgroup {shader cycles, 100 MHz ticks}
};

constexpr int MM_MAX_GROUPS = 8;   // argument blocks of one grouped launch travel in the kernel arguments (8 x ~230 B)
struct GroupedGemmArgs {
    GemmArgs g[MM_MAX_GROUPS];
    int ngroups;
};

struct GroupedTileArgs {
    GemmArgs g[MM_MAX_GROUPS];
    int first_block[MM_MAX_GROUPS + 1];   // prefix sum of the groups' tile counts
    int ngroups;
};
hipError_t launch_mx_gemm256_grouped(GroupedTileArgs &ga, bool w4, hipStream_t stream);   // fills first_block[]

struct QuantArgs {
    const uint16_t *src;   // [rows, K] bf16
    const int16_t *idx;    // [KN + KS + KO]
    uint8_t *o[3];         // packed segments
    uint8_t *sf[3];        // scale tensors
    int rows;
};
struct GroupedQuantArgs {
    QuantArgs g[MM_MAX_GROUPS];
    int ngroups, K, KN, KS, KO;
};
hipError_t launch_reorder_quantize_grouped(const GroupedQuantArgs &ga, int max_rows, bool w4, hipStream_t stream);


// Device-sized grouped launches (mm_moe_quantize / mm_moe_matmul, include/micromix_hip.h): the groups are the experts of a sparse MoE
// block, their rows the slots [offsets[e], offsets[e + 1]) of buffers that hold all experts' rows in slot order.  What differs from
// expert to expert and is known on the host sits in a device table (one MoeExpert = one mm_moe_expert, 64 bytes); the row counts are
// read from `offsets` by every workgroup, so nothing is read back to the host and the grids depend on host values only.
struct MoeExpert {
    const int16_t *idx;        // reorder index (mm_moe_quantize)
    const uint8_t *W[3];       // packed weights BN, BS, BO (mm_moe_matmul)
    const uint8_t *SFW[3];     // their scales
    const uint16_t *bias;      // optional [N] bf16
};
struct MoeGroups {
    const int *offsets;        // [E + 1], device
    const MoeExpert *table;    // [E], device
    int E, n, max_rows;        // n: rows of the packed buffers; a group with more than max_rows rows is skipped
};
// first 128-row scale tile of expert e's run in a packed scale tensor: a function of offsets[e] alone (runs are disjoint because
// floor(lo / 128) + ceil(M / 128) <= floor(hi / 128) + 1, and all lie inside n / 128 + E tiles)
__host__ __device__ inline int moe_sf_tile(int lo, int e) { return (lo >> 7) + e; }
inline size_t moe_sf_bytes(int n, int E, int Kseg) { return (size_t)(n / 128 + E) * 128u * (size_t)(Kseg / 32); }
#if defined(__HIPCC__)
// the argument block of expert e in a launch whose `a` carries the packed buffers (X, SFX, D) and what all experts share
// ACT (mm_moe_gate_up_activate): `a` also carries the packed outputs of the fused gate / up epilogue, act_o / act_sf, which advance to
// the expert's rows and to its run of scale tiles by the rule of X / SFX -- the layout mm_moe_quantize writes and mm_moe_matmul reads
template <bool ACT = false>
__device__ __forceinline__ void moe_group_args(GemmArgs &a, const MoeGroups &mg, int e, int lo, int M) {
    const MoeExpert &x = mg.table[e];
    const size_t tile = (size_t)moe_sf_tile(lo, e);
    a.X[0] += (size_t)lo * (size_t)(a.K[0] >> 1);
    a.X[1] += (size_t)lo * (size_t)((a.K[1] >> 2) * 3);
    a.X[2] += (size_t)lo * (size_t)a.K[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a.SFX[i] += tile * (size_t)(a.K[i] << 2);      // a 128-row tile of a segment's scales: 128 * Kseg / 32 bytes
        a.W[i] = x.W[i];
        a.SFW[i] = x.SFW[i];
    }
    a.bias = x.bias;
    a.D += (size_t)lo * (size_t)a.N;
    a.M = M;
    a.sfx_row_tiles = (M + 127) >> 7;
    if constexpr (ACT) {
        a.act_o[0] += (size_t)lo * (size_t)(a.act_K[0] >> 1);
        a.act_o[1] += (size_t)lo * (size_t)((a.act_K[1] >> 2) * 3);
        a.act_o[2] += (size_t)lo * (size_t)a.act_K[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) a.act_sf[i] += tile * (size_t)(a.act_K[i] << 2);
    }
}
#endif
hipError_t launch_moe_quantize(const void *src, const int *row_of_slot, const MoeGroups &mg, int src_rows, int K, int KN, int KS, int KO,
                               bool w4, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, hipStream_t stream);
// a, b bf16 [n, K] in slot order; h_out bf16 [n, K] or nullptr; mixed mode only
hipError_t launch_moe_activate_quantize(const void *a, const void *b, void *h_out, const MoeGroups &mg, int K, int KN, int KS, int KO, uint8_t *oN,
                                        uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, hipStream_t stream);
bool mx_gemm_stream_moe_supported(int max_m, const int K[3]);
// `a`: X / SFX / D the packed buffers, K, N, round_per_segment, sfw_row_tiles filled in; groups of 1 .. min(max_rows, 64) rows
hipError_t launch_mx_gemm_stream_moe(const GemmArgs &a, const MoeGroups &mg, bool w4, hipStream_t stream);
// ... groups of 65 .. max_rows rows on the tiled kernels
hipError_t launch_mx_gemm256_moe(const GemmArgs &a, const MoeGroups &mg, bool w4, hipStream_t stream);
// ... every group of 1 .. max_rows rows on the 256-feature tiles with the fused gate / up epilogue (mm_moe_gate_up_activate): fp4 weights
// of N = 2 I interleaved rows, `a` as above plus act_K / act_o / act_sf (the packed buffers of the consumer's operand); no D
hipError_t launch_mx_gemm256_moe_act(const GemmArgs &a, const MoeGroups &mg, hipStream_t stream);
const char *describe_mx_gemm256_moe_act(int E, int n, int N);
hipError_t launch_moe_zero_rows(void *D, const int *offsets, int E, int n, int N, hipStream_t stream);

hipError_t set_quant_clock_buffer(unsigned long long *buf);   // -DMM_INSTRUMENT only
hipError_t launch_reorder_quantize(const void *src, int rows, int K, const int16_t *idx, int KN, int KS, int KO, bool w4,
                                   uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO,
                                   hipStream_t stream);
// mode: 0 silu(A) * B, 1 A (mixed), 2 A (all fp4), 3 = 0 with A | B interleaved per 128 columns in one [rows, 2 K] matrix
hipError_t launch_direct_quantize(const void *A, const void *B, int rows, int KN, int KS, int KO, int mode, uint8_t *oN,
                                  uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, hipStream_t stream);
hipError_t launch_rmsnorm_quantize(const void *src, const void *weight, float eps, int rows, int K, const int16_t *idx, int KN,
                                   int KS, int KO, bool integer_round, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN,
                                   uint8_t *sfS, uint8_t *sfO, hipStream_t stream);
// ... of s = src + res (bf16, one rounding), which is also written to s_out (mm_add_rmsnorm_quantize)
hipError_t launch_add_rmsnorm_quantize(const void *src, const void *res, void *s_out, const void *weight, float eps, int rows, int K,
                                       const int16_t *idx, int KN, int KS, int KO, bool integer_round, uint8_t *oN, uint8_t *oS, uint8_t *oO,
                                       uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, hipStream_t stream);
// RMSNorm in front of the quantization of the decode launches (mm_rmsnorm_qlinear_decode): weight == nullptr means no norm
// res / s_out (both or neither; with weight only): the residual add in front of the norm -- the rows are X + res, and one workgroup
// of the launch writes them to s_out (mm_add_rmsnorm_qlinear_decode)
struct NormArgs { const void *weight; float eps; int int_round; const void *res; void *s_out; };
constexpr NormArgs NO_NORM = {nullptr, 0.0f, 1, nullptr, nullptr};
int qlinear_decode_supported(int M, int N, const int K[3], bool rms = false, bool w4 = false);
hipError_t launch_qlinear_decode(const void *X, const int16_t *idx, const uint8_t *const W[3], const uint8_t *const SFW[3],
                                 int M, int N, const int K[3], bool w4, int round_per_segment, const void *bias, void *D,
                                 hipStream_t stream, const NormArgs &norm = NO_NORM);
hipError_t launch_mx_gemm(const GemmArgs &a, bool w4, hipStream_t stream);
hipError_t launch_mx_gemm256(const GemmArgs &a, bool w4, hipStream_t stream);
bool mx_gemm_act_supported(int M, int N);                                 // the tiled kernels with the fused gate / up epilogue take this shape
hipError_t launch_mx_gemm_act(const GemmArgs &a, hipStream_t stream);    // fp4 weights only
const char *describe_mx_gemm_act(int M, int N);
hipError_t launch_mx_gemm_skinny(const GemmArgs &a, bool w4, hipStream_t stream);
// second-generation weight-streaming kernel (mx_gemm_stream.hip): M <= 64 (one to four 16-token tiles)
bool mx_gemm_stream_supported(int M, int N, const int K[3], bool w4);
hipError_t launch_mx_gemm_stream(const GemmArgs &a, bool w4, hipStream_t stream);
bool mx_gemm_stream_grouped_supported(int max_m, int ngroups, int N, const int K[3]);
hipError_t launch_mx_gemm_stream_grouped(const GroupedGemmArgs &ga, int max_m, bool w4, hipStream_t stream);
// ... with silu(gate) * up + its quantization inside every workgroup (mm_down_activate_decode)
bool down_activate_stream_supported(int M, int N, const int K[3], bool w4 = false);   // w4: the ring / reduction tail of fp4 weights is 48 KB, not 64
hipError_t launch_down_activate_stream(const void *GU, const uint8_t *const W[3], const uint8_t *const SFW[3], int M, int N, const int K[3],
                                       bool w4, int round_per_segment, const void *bias, void *D, hipStream_t stream);
// ... with the quantization of the M <= 8 activation rows inside every workgroup (mm_qlinear_decode)
bool qlinear_stream_supported(int M, int N, const int K[3], bool rms = false, bool w4 = false);
hipError_t launch_qlinear_stream(const void *X, const int16_t *idx, const uint8_t *const W[3], const uint8_t *const SFW[3], int M, int N,
                                 const int K[3], bool w4, int round_per_segment, const void *bias, void *D, hipStream_t stream,
                                 const NormArgs &norm = NO_NORM);
// ... the fused gate | up weight (fp4) with silu(gate) * up and the quantization for the consumer inside the launch (a.act_K / act_o / act_sf;
// round 6): from the quantized activations (M <= 16) or, `X` / `idx` / `norm`, from the bf16 rows (M <= 4)
bool gate_up_act_stream_supported(int M, int N, const int K[3], bool from_bf16, bool rms);
hipError_t launch_gate_up_act_stream(const GemmArgs &a, hipStream_t stream);
hipError_t launch_gate_up_act_stream_decode(const void *X, const int16_t *idx, const GemmArgs &a, hipStream_t stream, const NormArgs &norm = NO_NORM);
hipError_t launch_mx_gemm_skinny_grouped(const GroupedGemmArgs &ga, int max_m, bool w4, hipStream_t stream);
size_t mx_gemm_workspace_bytes(int M, int N, const int K[3], bool w4, bool force, bool tickets_zeroed);
bool mx_gemm_small_m_uses_tiles(int M, int N, const int K[3], bool w4, size_t ws_bytes, bool force_split);
const char *describe_mx_gemm256(int M, int N, const int K[3], bool w4, size_t ws_bytes, bool force_split, bool tickets_zeroed, bool out_f32 = false);   // thread-local buffer  // 0 when mm_matmul would not split K for this shape

// paged KV cache: one layer of a cache and the page table of its B sequences (layout: kv_cache.hip; device side: mx_paged_kv.h)
constexpr int KV_INT4 = 0, KV_BF16 = 1, KV_FP8 = 3;      // the codes of enum mm_kv_dtype (include/micromix_hip.h); 2 is unassigned
struct PagedKV {
    uint8_t *data;
    uint16_t *param;           // int4 and fp8: fp16 (scale, zero) per row
    const int *indptr, *indices, *last_page_len;
    int max_pages, L, layer, Hkv, P, B;
    int kind;                  // KV_INT4, KV_BF16 or KV_FP8
};
constexpr float KV_DEFAULT_SM_SCALE = 0.08838834764831845f;                // 1 / sqrt(128)
inline float kv_scale_log2(float sm_scale) { return (sm_scale > 0.0f ? sm_scale : KV_DEFAULT_SM_SCALE) * 1.4426950408889634f; }
// split-KV chunks, from host-known values only, so a captured graph stays valid while the sequences grow up to max_seq_len: enough
// chunks of `work` items to reach target_workgroups, of at least 256 tokens each, the chunk length a multiple of round_to
void kv_chunks(long long work, int target_workgroups, int max_seq_len, int round_to, int *nc, int *chunk);
// Sliding window (window >= 1; 0: none): a query attends its last `window` positions, itself included.  The kernels walk only the
// tiles that hold them, and the chunks are laid over that span -- at most window + slack tokens, slack being what a kernel's range
// gains by starting on a tile edge and by the query tile's rows (prefill; decode starts at the window itself: none) -- so the grid
// still depends on host values only, and a window that reaches max_seq_len gives the split of no window
int kv_window_span(int max_seq_len, int window, int slack);
// append and single-token attention (kv_cache.hip)
void kv_decode_split(int B, int Hkv, int max_seq_len, int window, int *nc, int *chunk);
size_t kv_decode_workspace_bytes(int B, int Hq, int Hkv, int max_seq_len, int window);
hipError_t launch_kv_append(const PagedKV &kv, const void *k, const void *v, const int *append_indptr, int T, hipStream_t stream);
hipError_t launch_paged_decode(const PagedKV &kv, const void *q, int Hq, int max_seq_len, int window, float sm_scale, void *ws, void *o,
                               hipStream_t stream);
// decode over sequences that share leading pages (kv_cache.hip; the host rules and the split: mx_kv_shared_host.h); ws always used
hipError_t launch_paged_decode_shared(const PagedKV &kv, const void *q, int Hq, const int *group_indptr, const int *group_members,
                                      const int *shared_len, int max_shared_len, int max_suffix_len, float sm_scale, void *ws, void *o,
                                      hipStream_t stream);
// RoPE + append in one launch (rope_append.hip): q | k | v share the token stride qkv_stride, cos | sin the stride cs_stride (elements)
hipError_t launch_rope_kv_append(const PagedKV &kv, const void *q, const void *k, const void *v, int64_t qkv_stride, int Hq, const void *cos,
                                 const void *sin, int64_t cs_stride, const int *append_indptr, int T, void *q_out, hipStream_t stream);
// rows [0, rows[i]) of page src_pages[i] -> page dst_pages[i], every layer, K and V, every head (kv_copy.hip); kv.layer is 0
hipError_t launch_kv_copy_pages(const PagedKV &kv, const int *src_pages, const int *dst_pages, const int *rows, int num_pairs,
                                hipStream_t stream);
// within sequence b, for moves m in [move_indptr[b], move_indptr[b + 1]): the token row at position src_pos[m] -> position dst_pos[m],
// every layer, K and V, every head, all sources read before any destination is written (kv_move.hip); kv.layer is 0
hipError_t launch_kv_move_rows(const PagedKV &kv, const int *move_indptr, const int *src_pos, const int *dst_pos, int num_moves,
                               hipStream_t stream);
// greedy verification of drafts (verify.hip): the argmax of bf16 rows (ws: argmax_workspace_bytes, 0 when a row is one part), and the walk
// that picks each sequence's accepted path and writes the move table launch_kv_move_rows takes with move_indptr = qo_indptr
int argmax_parts(int vocab);                              // workgroups a row is divided among: ceil(vocab / MM_ARGMAX_CHUNK)
size_t argmax_workspace_bytes(int rows, int vocab);
hipError_t launch_argmax_rows(const void *logits, int rows, int vocab, long long ld, int *out, void *ws, hipStream_t stream);
// ... of two matrices of one shape in the same launches, each with its row distance, answers and workspace; a row of the second whose
// cand entry (device, `rows` entries) is outside [0, vocab) is not read and gets no answer
hipError_t launch_argmax_rows_pair(const void *logits, long long ld, int *out, void *ws, const void *logits2, long long ld2, int *out2, void *ws2,
                                   const int *cand, int rows, int vocab, hipStream_t stream);
hipError_t launch_verify_greedy(const int *target_tok, const int *draft_tok, const int *root_tok, const void *tree_mask, const int *qo_indptr,
                                int T, const int *kv_indptr, const int *last_page_len, int P, int B, int *result, int *move_src,
                                int *move_dst, hipStream_t stream);
// sampling over bf16 rows (sample.hip): temperature, top-k, top-p, min-p, each a device array of `rows` entries or null; ws:
// sample_workspace_bytes, uninitialised
size_t sample_workspace_bytes(int rows, int vocab);
hipError_t launch_sample_rows(const void *logits, int rows, int vocab, long long ld, const float *u, const float *temperature,
                              const int *top_k, const float *top_p, const float *min_p, int *out, void *ws, hipStream_t stream);
// speculative sampling of chain drafts over bf16 rows (spec_sample.hip, include/micromix_spec.h): draft_logits null = one-hot drafts,
// accepted null when not wanted, the per-row parameters as launch_sample_rows takes them; ws: spec_sample_workspace_bytes, uninitialised
size_t spec_sample_workspace_bytes(int rows, int vocab);
hipError_t launch_spec_sample_rows(const void *logits, long long ld, const void *draft_logits, long long draft_ld, int rows, int vocab,
                                   const int *cand_tok, const float *u_accept, const float *u_resample, const float *temperature,
                                   const int *top_k, const float *top_p, const float *min_p, int *out, int *accepted, void *ws,
                                   hipStream_t stream);
// one step of the device allocator (kv_step.hip, include/micromix_kvstep.h): the step kernel, one workgroup, then the launch that rebuilds
// kv_indices and writes token_pos; keep, depths and token_pos null when absent
struct KVStep {
    int *state;
    int B, max_pages, pps, P, max_seq_len;
    const int *keep;
    int keep_stride;
    const int *next_new;
    int T;
    const int *depths;
    int *kv_indptr, *kv_indices;
    long long capacity;
    int *last_page_len, *append_indptr, *token_pos;
};
hipError_t launch_kv_step(const KVStep &s, hipStream_t stream);
// the token half of a step (token_step.hip, include/micromix_tokens.h): commit a verified step into the history; draft the next chain
// by n-gram lookup over it.  Optional arrays null when absent; ws: ngram_workspace_bytes, uninitialised
struct TokenStep {
    int *tokens;
    long long ld_tok;
    int B;
    int *total_len, *finished;
    const int *result;
    int result_stride;
    const int *target_tok;
    int T;
    const int *qo_indptr, *root_tok, *max_total, *stop_tok;
    int n_stop;
    const int *kv_state;
    int *emitted;
};
hipError_t launch_token_step(const TokenStep &s, hipStream_t stream);
struct NgramDraft {
    int *tokens;
    long long ld_tok;
    int B;
    const int *total_len, *next_indptr;
    int T, min_n, max_n;
    int *draft_tok, *root_tok, *cand_tok, *match_len, *row_seq, *row_total_len;
    unsigned *ws;
};
int ngram_parts(long long ld_tok);
size_t ngram_workspace_bytes(int batch, long long ld_tok);
hipError_t launch_ngram_draft(const NgramDraft &s, hipStream_t stream);
// uniform numbers keyed by seed and position (random.hip, include/micromix_random.h): sub and row_seq null when absent, out or bits
// null when not wanted; no state, no workspace
struct UniformRows {
    const long long *seed;
    const int *sub;
    int B;
    const int *row_seq, *pos;
    int rows, n;
    unsigned domain;
    float *out;
    unsigned *bits;
    long long ld_out;
};
hipError_t launch_uniform_rows(const UniformRows &s, hipStream_t stream);
// token log-probabilities over bf16 rows (logprob.hip, include/micromix_logprob.h): target and temperature device arrays of `rows`
// entries or null, every output null when not wanted, top_n 0 .. 32; ws: logprob_workspace_bytes, uninitialised
size_t logprob_workspace_bytes(int rows, int vocab, int top_n);
hipError_t launch_logprob_rows(const void *logits, int rows, int vocab, long long ld, const int *target, const float *temperature,
                               float *logprob, int *rank, float *lse, int top_n, int *top_idx, float *top_logprob, void *ws,
                               hipStream_t stream);
// penalties, bias and mask over bf16 rows (logits_process.hip, include/micromix_logits.h): every optional array null when off, one launch,
// no workspace
hipError_t launch_process_logits(const void *logits, int rows, int vocab, long long ld_in, void *out, long long ld_out, const int *tokens,
                                 long long ld_tok, int n_seq, const int *row_seq, const int *prompt_len, const int *total_len,
                                 const float *repetition, const float *frequency, const float *presence, const int *bias_idx,
                                 const float *bias_val, int n_bias, const int *mask, long long ld_mask, hipStream_t stream);
// calibration statistics of one batch (calib_stats.hip, include/micromix_calib.h): x [rows, K] bf16 or fp16, K a multiple of 128 up to
// 32768, rows >= 1; ws: calib_workspace_bytes, uninitialised
size_t calib_workspace_bytes(int rows, int K);
hipError_t launch_calib_accumulate(const void *x, bool fp16, int rows, int K, long long ld, float lamda, float *score, long long *counts,
                                   void *ws, hipStream_t stream);
// sparse MoE block around the grouped GEMMs (moe.hip): n = T * top_k pairs, H a multiple of 8, rows 16-byte aligned
hipError_t launch_moe_route(const void *logits, int T, int E, int top_k, int *ids, void *w, hipStream_t stream);
hipError_t launch_moe_plan(const int *ids, int n, int E, int top_k, int *offsets, int *sorted_token, int *slot_of, hipStream_t stream);
hipError_t launch_moe_gather(const void *x, const int *sorted_token, int T, int n_rows, int H, void *x_sorted, hipStream_t stream);
hipError_t launch_moe_combine(const void *y, const int *ids, const void *w, const int *slot_of, int T, int top_k, int H, void *out,
                              hipStream_t stream);
// causal multi-token attention over the paged cache (kv_prefill.hip)
void kv_prefill_split(int T, int B, int Hq, int Hkv, int max_seq_len, int window, int *tiles, int *nc, int *chunk);
size_t kv_prefill_workspace_bytes(int T, int B, int Hq, int Hkv, int max_seq_len, int window);
// tree_mask: null, or the [T] words of mm_paged_prefill_tree (then window is 0)
hipError_t launch_paged_prefill(const PagedKV &kv, const void *q, const int *qo_indptr, int T, int Hq, int max_seq_len, int window,
                                const void *tree_mask, float sm_scale, void *ws, void *o, hipStream_t stream);

}  // namespace mm
