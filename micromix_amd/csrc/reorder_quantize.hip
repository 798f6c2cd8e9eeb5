// Fused column-reorder + per-32-group absmax + UE8M0 scale + MXFP4/MXFP6/MXFP8
// quantize + pack for gfx950.
//
// What it computes is the reference's reorder_quantize_mixed_kernel
// (mgemm/src/reorder.cu:94-269) and reorder_quantize_mxfp4_kernel (:271-432):
// for every row and every 32-wide group g of *reordered* columns,
//   v[i] = row[idx[32g+i]];  amax = max|v|;  e = ceil(log2(amax/FMAX)) (amax==0 -> -1);
//   q[i] = RNE_fmt(v[i] * 2^-e);  SF byte = e + 127 at sf_offset(row, g - seg_start/32).
//
// How it is laid out for MI355X (HBM-bound: 2*K bytes in, ~K/2..K bytes out per row):
//  * one workgroup owns a strided set of rows; thread t owns group t for every one
//    of those rows, so its 32 reorder indices live in 16 VGPRs for the whole launch
//    (the reference re-reads each index from global memory per element);
//  * the row is staged in LDS with 16-byte coalesced loads; the next row's loads are
//    issued before the current row's gather so HBM latency hides under the LDS work;
//  * all scale arithmetic is integer/exponent arithmetic (no log2/ceil/ldexp/divide); the element conversion is
//    one hardware MX-converter instruction per 2 (fp4/fp8) or 32 (fp6) elements.
#include "mx_common.h"
#include "mx_direct_convert.h"
#include "mx_group_convert.h"
#include "mx_instrument.h"
#include "mx_kernels.h"
#include "mx_quant_plan.h"

namespace mm {

#if MM_CLOCKS
// instrumented variant only: per workgroup {start, row staged, group quantized and stored, end} in 100 MHz ticks (tools/quant_clock.py)
__device__ unsigned long long *g_quant_clock = nullptr;
#endif

// How a row reaches its LDS image, 16 bytes (eight bf16) per lane and step.  load() issues the global loads of chunk c of row r (grow:
// that row of src; zeros past the row's end) into a Regs, of which the body keeps four in flight; chunk() turns a Regs into the eight
// bf16 to stage; keep() runs once the row's chunks are in LDS, for a hook that also stores what it staged.  chunk() and keep() are
// called only for chunks of the row.  StageLoad, the plain load, is what every quantizer but moe_activate_quantize_kernel stages with.
struct StageLoad {
    typedef uint4 Regs;
    __device__ __forceinline__ Regs load(const uint4 *__restrict__ grow, int, int, int c, bool in_row) const {
        uint4 t = make_uint4(0u, 0u, 0u, 0u);
        if (in_row) t = grow[c];
        return t;
    }
    __device__ __forceinline__ uint4 chunk(Regs &t, int, int, int) const { return t; }
    __device__ __forceinline__ void keep(const Regs &, int, int, int) const {}
};
// The staged row is computed: src is a, and h = bf16(bf16(silu(a)) * b) from the same row of b (silu_mul_bf16, mx_direct_convert.h),
// 4 + 4 loads in flight per lane; with h_out the eight bf16 are also stored, unreordered -- after all four chunks are computed, so
// that no chunk's arithmetic waits behind a store.
struct StageSiluMul {
    struct Regs { uint4 a, b; };
    const uint16_t *__restrict__ b;     // [rows, K]
    uint16_t *__restrict__ h_out;       // [rows, K] or nullptr
    __device__ __forceinline__ Regs load(const uint4 *__restrict__ grow, int r, int K, int c, bool in_row) const {
        Regs t = {make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
        if (in_row) {
            t.a = grow[c];
            t.b = reinterpret_cast<const uint4 *>(b + (size_t)r * K)[c];
        }
        return t;
    }
    __device__ __forceinline__ uint4 chunk(Regs &t, int, int, int) const {
        float x[8], y[8];
        unpack8(t.a, x);
        unpack8(t.b, y);
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = silu_mul_bf16(x[2 * k], y[2 * k]) | (silu_mul_bf16(x[2 * k + 1], y[2 * k + 1]) << 16);
        return t.a = make_uint4(w[0], w[1], w[2], w[3]);
    }
    __device__ __forceinline__ void keep(const Regs &t, int r, int K, int c) const {
        if (h_out != nullptr) reinterpret_cast<uint4 *>(h_out + (size_t)r * K)[c] = t.a;
    }
};

// rows first_row, first_row + row_stride, ... of one [rows, K] matrix (one workgroup's share); sf_row0: the row of the scale tensors
// that row 0 of the matrix is (0 everywhere but in the moe kernels, whose pointers are those of ONE row)
template <bool W4, class Stage = StageLoad>
__device__ __forceinline__ void reorder_quantize_body(const uint16_t *__restrict__ src, int rows, int K, const int16_t *__restrict__ idx,
                                                      int KN, int KS, int KO, uint8_t *__restrict__ oN, uint8_t *__restrict__ oS,
                                                      uint8_t *__restrict__ oO, uint8_t *__restrict__ sfN, uint8_t *__restrict__ sfS,
                                                      uint8_t *__restrict__ sfO, int first_row, int row_stride, int sf_row0 = 0,
                                                      const Stage hook = Stage()) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int G = (KN + KS + KO) >> 5;  // groups produced; K is the input row length (>= 32 * G)
    const int g = threadIdx.x;
    const bool active = g < G;
    const int nchunk = K >> 3;  // 16-byte chunks per row
    // fp6 / fp8 codes go through an image of the row's [S | O] codes behind the staged row (store_code_image, mx_group_convert.h): 11.3 -> 9.3 us
    const int bytesS = KS / 4 * 3, bytesO = KO;
    uint8_t *image = smem + (size_t)K * 2;

    uint32_t ix[16];
    if (active) {
        const uint4 *p = reinterpret_cast<const uint4 *>(idx + (size_t)g * 32);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 q = p[i];
            // keep BYTE offsets (index << 1; indices are < 32768 so each half stays within 16 bits)
            ix[4 * i] = swizzle_offsets((q.x << 1) & 0xFFFEFFFEu);
            ix[4 * i + 1] = swizzle_offsets((q.y << 1) & 0xFFFEFFFEu);
            ix[4 * i + 2] = swizzle_offsets((q.z << 1) & 0xFFFEFFFEu);
            ix[4 * i + 3] = swizzle_offsets((q.w << 1) & 0xFFFEFFFEu);
        }
    }
    // Which segment this thread's group falls in (positions in reordered order).
    const int gN = KN >> 5, gS = KS >> 5;
    int seg, j, kseg;
    if (g < gN) { seg = 0; j = g; kseg = KN; }
    else if (g < gN + gS) { seg = 1; j = g - gN; kseg = KS; }
    else { seg = 2; j = g - gN - gS; kseg = KO; }

#if MM_CLOCKS
    unsigned long long *ck = g_quant_clock != nullptr ? g_quant_clock + 4 * (size_t)blockIdx.x : nullptr;
    if (ck != nullptr && threadIdx.x == 0) ck[0] = __builtin_amdgcn_s_memrealtime();
#endif
    typename Stage::Regs stage[4];
    int r = first_row;
    if (r < rows) {
        const uint4 *grow = reinterpret_cast<const uint4 *>(src + (size_t)r * K);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = threadIdx.x + i * blockDim.x;
            stage[i] = hook.load(grow, r, K, c, c < nchunk);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = threadIdx.x + i * blockDim.x;
            if (c < nchunk) reinterpret_cast<uint4 *>(smem)[swizzle_chunk(c)] = hook.chunk(stage[i], r, K, c);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = threadIdx.x + i * blockDim.x;
            if (c < nchunk) hook.keep(stage[i], r, K, c);
        }
    }
    __syncthreads();
#if MM_CLOCKS
    if (ck != nullptr && threadIdx.x == 0) ck[1] = __builtin_amdgcn_s_memrealtime();
#endif
    for (; r < rows; r += row_stride) {
        const int rn = r + row_stride;
        if (rn < rows) {
            const uint4 *grow = reinterpret_cast<const uint4 *>(src + (size_t)rn * K);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = threadIdx.x + i * blockDim.x;
                stage[i] = hook.load(grow, rn, K, c, c < nchunk);
            }
        }
        if (active) {
            const uint8_t *row = smem;
            uint32_t byte;
            uint8_t *sf;
            uint32_t v[16];
            const uint32_t amax = gather_group(row, ix, v);   // once per wave, whatever segments its lanes are in
            if (seg == 0) {
                byte = finish_group<EL_FP4, true>(v, amax, oN + (size_t)r * (KN >> 1) + j * 16);
                sf = sfN;
            } else if (seg == 1) {
                if constexpr (W4) byte = finish_group<EL_FP4, true>(v, amax, oS + (size_t)r * (KS >> 1) + j * 16);
                else byte = finish_group<EL_FP6>(v, amax, image + j * 24);                 // into the LDS image (see above)
                sf = sfS;
            } else {
                if constexpr (W4) byte = finish_group<EL_FP4, true>(v, amax, oO + (size_t)r * (KO >> 1) + j * 16);
                else byte = finish_group<EL_FP8>(v, amax, image + bytesS + j * 32);
                sf = sfO;
            }
            // the 4 block scales of one row and one 128-column slab are 4 consecutive bytes of the SF layout: gather them
            // from the lane quad (segment widths are multiples of 128, so a quad never straddles segments) and store a dword
            const uint32_t b1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0x55, 0xF, 0xF, false);
            const uint32_t b2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0xAA, 0xF, 0xF, false);
            const uint32_t b3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0xFF, 0xF, 0xF, false);
            if ((g & 3) == 0)
                store_scale_dword(sf + sf_offset(r + sf_row0, j, kseg), byte | (b1 << 8) | (b2 << 16) | (b3 << 24));
        }
#if MM_CLOCKS
        if (ck != nullptr && threadIdx.x == 0 && r == first_row) ck[2] = __builtin_amdgcn_s_memrealtime();
#endif
        __syncthreads();
        if constexpr (!W4) store_code_image(image, bytesS, bytesO, oS, oO, r);
        if (rn < rows) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = threadIdx.x + i * blockDim.x;
                if (c < nchunk) reinterpret_cast<uint4 *>(smem)[swizzle_chunk(c)] = hook.chunk(stage[i], rn, K, c);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = threadIdx.x + i * blockDim.x;
                if (c < nchunk) hook.keep(stage[i], rn, K, c);
            }
        }
        __syncthreads();
    }
#if MM_CLOCKS
    if (ck != nullptr && threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ck[3] = __builtin_amdgcn_s_memrealtime();
    }
#endif
}

template <bool W4, int MAXT>
__global__ void __launch_bounds__(MAXT)
reorder_quantize_kernel(const uint16_t *__restrict__ src, int rows, int K, const int16_t *__restrict__ idx, int KN,
                        int KS, int KO, uint8_t *__restrict__ oN, uint8_t *__restrict__ oS, uint8_t *__restrict__ oO,
                        uint8_t *__restrict__ sfN, uint8_t *__restrict__ sfS, uint8_t *__restrict__ sfO) {
    reorder_quantize_body<W4>(src, rows, K, idx, KN, KS, KO, oN, oS, oO, sfN, sfS, sfO, blockIdx.x, gridDim.x);
}

// Grouped launch (MoE experts: every expert quantizes its own token rows with its own reorder index; reference: the
// per-expert reorder_quantize_x calls of qMixtralLayer.py:507-519): blockIdx.y picks one of up to MM_MAX_GROUPS argument blocks.
template <bool W4, int MAXT>
__global__ void __launch_bounds__(MAXT) reorder_quantize_grouped_kernel(GroupedQuantArgs ga) {
    const QuantArgs &q = ga.g[blockIdx.y];
    if ((int)blockIdx.x < q.rows)
        reorder_quantize_body<W4>(q.src, q.rows, ga.K, q.idx, ga.KN, ga.KS, ga.KO, q.o[0], q.o[1], q.o[2], q.sf[0], q.sf[1], q.sf[2],
                                  blockIdx.x, gridDim.x);
}

// Device-sized grouped launch (mm_moe_quantize): one workgroup per slot s of the packed buffers.  It finds the expert that owns the
// slot among the <= 65 offsets (the number of offsets[i] <= s, i < E, less one: an empty expert shares its offset with the next one, and
// the last of them is the owner), takes the row to read from row_of_slot (the gather of the MoE dispatch, folded in) or s itself, and
// quantizes it with that expert's reorder index into packed row s and the expert's run of scale tiles (moe_sf_tile).  A slot that no
// expert owns, offsets that are not those of a plan, or a source row outside [0, src_rows) leave the slot's outputs untouched; the
// scale tile written is at most s / 128 + E - 1 whatever the offsets hold.
template <bool W4, int MAXT>
__global__ void __launch_bounds__(MAXT)
moe_quantize_kernel(const uint16_t *__restrict__ src, const int *__restrict__ row_of_slot, MoeGroups mg, int src_rows, int K, int KN, int KS,
                    int KO, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO) {
    const int s = blockIdx.x;
    int e = -1;
    for (int i = 0; i < mg.E; ++i) e += mg.offsets[i] <= s ? 1 : 0;
    if (e < 0) return;
    const int lo = mg.offsets[e], hi = mg.offsets[e + 1];
    if (lo < 0 || lo > s || s >= hi || hi > mg.n) return;
    const int t = row_of_slot != nullptr ? row_of_slot[s] : s;
    if (t < 0 || t >= src_rows) return;
    const int r = s - lo;                                     // the row inside the expert's own [M_e, K] matrix
    const size_t tile = (size_t)moe_sf_tile(lo, e) + (size_t)(r >> 7);
    reorder_quantize_body<W4>(src + (size_t)t * K, 1, K, mg.table[e].idx, KN, KS, KO, oN + (size_t)s * (KN >> 1),
                              oS + (size_t)s * (W4 ? KS >> 1 : (KS >> 2) * 3), oO + (size_t)s * (W4 ? KO >> 1 : KO),
                              sfN + tile * (size_t)(KN << 2), sfS + tile * (size_t)(KS << 2), sfO + tile * (size_t)(KO << 2), 0, 1, r & 127);
}

// mm_moe_activate_quantize: moe_quantize_kernel<false> on a row that is computed while it is staged -- slot s of a and b gives
// h = bf16(bf16(silu(a)) * b), which goes to h_out (when given) and through the expert's reorder index into packed row s and the
// expert's run of scale tiles.  The same walk over the offsets and the same guards: a slot no expert owns is left untouched, h_out too.
template <int MAXT>
__global__ void __launch_bounds__(MAXT)
moe_activate_quantize_kernel(const uint16_t *__restrict__ a, const uint16_t *__restrict__ b, uint16_t *__restrict__ h_out, MoeGroups mg, int K,
                             int KN, int KS, int KO, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO) {
    const int s = blockIdx.x;
    int e = -1;
    for (int i = 0; i < mg.E; ++i) e += mg.offsets[i] <= s ? 1 : 0;
    if (e < 0) return;
    const int lo = mg.offsets[e], hi = mg.offsets[e + 1];
    if (lo < 0 || lo > s || s >= hi || hi > mg.n) return;
    const int r = s - lo;
    const size_t tile = (size_t)moe_sf_tile(lo, e) + (size_t)(r >> 7), row = (size_t)s * K;
    reorder_quantize_body<false>(a + row, 1, K, mg.table[e].idx, KN, KS, KO, oN + (size_t)s * (KN >> 1), oS + (size_t)s * ((KS >> 2) * 3),
                                 oO + (size_t)s * KO, sfN + tile * (size_t)(KN << 2), sfS + tile * (size_t)(KS << 2), sfO + tile * (size_t)(KO << 2),
                                 0, 1, r & 127, StageSiluMul{b + row, h_out != nullptr ? h_out + row : nullptr});
}

#if MM_CLOCKS
hipError_t set_quant_clock_buffer(unsigned long long *buf) { return hipMemcpyToSymbol(HIP_SYMBOL(g_quant_clock), &buf, sizeof(buf)); }
#endif

// ---- the host side: the plan is mx_quant_plan.h's; what follows picks the instantiation and launches ----
// The one place that turns a plan into template arguments: fn(fp4 weights, the kernel's launch bound)
template <class Fn>
static hipError_t for_variant(bool w4, const quant::ReorderPlan &p, Fn &&fn) {
    using std::bool_constant, std::integral_constant;
    if (p.max_threads == 256) return w4 ? fn(bool_constant<true>{}, integral_constant<int, 256>{}) : fn(bool_constant<false>{}, integral_constant<int, 256>{});
    return w4 ? fn(bool_constant<true>{}, integral_constant<int, 1024>{}) : fn(bool_constant<false>{}, integral_constant<int, 1024>{});
}

hipError_t launch_reorder_quantize(const void *src, int rows, int K, const int16_t *idx, int KN, int KS, int KO, bool w4,
                                   uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO,
                                   hipStream_t stream) {
    if (rows == 0) return hipSuccess;
    const quant::ReorderPlan p = quant::plan_reorder_quantize(K, KN, KS, KO, w4);
    return for_variant(w4, p, [&](auto w4_, auto maxt_) {
        constexpr auto kern = reorder_quantize_kernel<decltype(w4_)::value, decltype(maxt_)::value>;
        // one resident wave of workgroups (no tail), each striding over the rows
        // (fewer, fatter workgroups that keep their reorder indices for 2 / 4 / 8 rows were measured: 11.1 -> 11.7 / 15.6 / 23.9 us;
        // one row per workgroup with the occupancy limited to 12 / 8 / 4 workgroups per CU, so that rounds of workgroups overlap
        // their load / gather / store phases: 11.3 / 11.4 / 13.7 us)
        const int blocks = quant::resident_grid(rows, device_cus(), resident_per_cu<kern>(p.threads, p.lds_bytes));
        return launch_kernel<kern>(p.shape(blocks), stream, diag_events(), (const uint16_t *)src, rows, K, idx, KN, KS, KO, oN, oS, oO, sfN, sfS, sfO);
    });
}

hipError_t launch_reorder_quantize_grouped(const GroupedQuantArgs &ga, int max_rows, bool w4, hipStream_t stream) {
    if (ga.ngroups < 1 || ga.ngroups > MM_MAX_GROUPS || max_rows < 1) return hipErrorInvalidValue;
    const quant::ReorderPlan p = quant::plan_reorder_quantize(ga.K, ga.KN, ga.KS, ga.KO, w4);
    return for_variant(w4, p, [&](auto w4_, auto maxt_) {
        constexpr auto kern = reorder_quantize_grouped_kernel<decltype(w4_)::value, decltype(maxt_)::value>;
        // one resident wave of workgroups shared by the groups
        const int bx = quant::resident_grid(max_rows, device_cus(), resident_per_cu<kern>(p.threads, p.lds_bytes), ga.ngroups);
        return launch_kernel<kern>(p.shape(bx, ga.ngroups), stream, DiagEvents{}, ga);
    });
}

hipError_t launch_moe_quantize(const void *src, const int *row_of_slot, const MoeGroups &mg, int src_rows, int K, int KN, int KS, int KO,
                               bool w4, uint8_t *oN, uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, hipStream_t stream) {
    if (mg.n == 0) return hipSuccess;
    const quant::ReorderPlan p = quant::plan_reorder_quantize(K, KN, KS, KO, w4);
    return for_variant(w4, p, [&](auto w4_, auto maxt_) {
        constexpr auto kern = moe_quantize_kernel<decltype(w4_)::value, decltype(maxt_)::value>;
        return launch_kernel<kern>(p.shape(mg.n), stream, DiagEvents{}, (const uint16_t *)src, row_of_slot, mg, src_rows, K, KN, KS, KO, oN, oS, oO, sfN,
                                   sfS, sfO);
    });
}

hipError_t launch_moe_activate_quantize(const void *a, const void *b, void *h_out, const MoeGroups &mg, int K, int KN, int KS, int KO, uint8_t *oN,
                                        uint8_t *oS, uint8_t *oO, uint8_t *sfN, uint8_t *sfS, uint8_t *sfO, hipStream_t stream) {
    if (mg.n == 0) return hipSuccess;
    const quant::ReorderPlan p = quant::plan_reorder_quantize(K, KN, KS, KO, false);
    auto launch = [&](auto maxt_) {
        constexpr auto kern = moe_activate_quantize_kernel<decltype(maxt_)::value>;
        return launch_kernel<kern>(p.shape(mg.n), stream, DiagEvents{}, (const uint16_t *)a, (const uint16_t *)b, (uint16_t *)h_out, mg, K, KN, KS, KO, oN,
                                   oS, oO, sfN, sfS, sfO);
    };
    return p.max_threads == 256 ? launch(std::integral_constant<int, 256>{}) : launch(std::integral_constant<int, 1024>{});
}

}  // namespace mm
