// Body of the large-M fused MX GEMM kernel, included several times by mx_gemm256.hip (MM_WM x 2 waves, each TM x TN MFMA tiles):
//   MM_NS = g256, MM_WM = 4, MM_TM = 2, MM_TN = 4 : 256 x 256 tile (8 waves x 64 x 128)  -- enough tiles to fill the chip
//   MM_NS = g128, MM_WM = 4, MM_TM = 1, MM_TN = 4 : 128 x 256 tile (8 waves x 32 x 128)  -- medium M, when 256-row tiles would leave CUs idle
//   MM_NS = g64,  MM_WM = 4, MM_TM = 1, MM_TN = 2 : 128 x 128 tile (8 waves x 32 x 64)   -- when even those fill at most half of the CUs
//   MM_NS = g32,  MM_WM = 2, MM_TM = 1, MM_TN = 2 : 64 x 128 tile (4 waves x 32 x 64)    -- 64 < M <= ~512: several workgroups per CU
//   MM_NS = g32n, MM_WM = 2, MM_TM = 1, MM_TN = 1 : 64 x 64 tile (4 waves x 32 x 32)
//   MM_NS = g16,  MM_WM = 1, MM_TM = 1, MM_TN = 1 : 32 x 64 tile (2 compute + 2 loader waves): launches whose 64 x 64 tiles would leave
//                                                   half of the CUs without a workgroup (q/o at M <= 128)
// MM_LDS_BUDGET = bytes of LDS one workgroup may claim; MM_ACC = clobber list naming the accumulator registers a[0 : 16*TM*TN-1] (mx_acc_regs.h).
// See mx_gemm256.hip for the design notes.
// MM_SMALL: the loader / compute tiles (WM <= 2, compiler-owned accumulators)
#define MM_SMALL (MM_WM <= 2)
namespace MM_NS {

__device__ __forceinline__ int mm_tid() { return (int)threadIdx.x; }
constexpr int WM = MM_WM, TM = MM_TM, TN = MM_TN;  // WM x 2 waves; MFMA tiles per wave: TM*32 tokens x TN*32 features
constexpr int BM = WM * TM * 32, BN = 2 * TN * 32, NT = WM * 2 * 64;
// threads of a workgroup: the loader / compute tiles (WM <= 2: SMALL) run NT compute threads plus NT loader threads (run_slabs_small)
constexpr bool SMALL = MM_SMALL;
constexpr int NTHREADS = SMALL ? 2 * NT : NT;
constexpr int NACC = 16 * TM * TN; // accumulator registers per lane: a[0 : NACC-1]
// The 8-wave tiles keep their accumulators in AGPRs that only inline asm names (see mx_gemm256.hip); the 4-wave tiles have 16-32 of
// them and leave them to the compiler (MFMA builtin), which then sees no asm-owned AGPRs and gives the kernel the whole
// 256-register budget of a 512-thread workgroup -- and cannot allocate a temporary on top of an accumulator it does not know
// about (it did, see tools/check_acc_regs.py).
struct Acc {
#if MM_SMALL
    v16f t[TM * TN];
#endif
};
constexpr int X_TILE = BM * 128;   // bytes, sized for fp8 / padded fp6
constexpr int SF_BYTES = 1024;     // two 512-byte SF atoms (256 rows x 4 blocks); only the first is used when BM = 128

// LDS that one workgroup may claim.  A CU has 160 KiB and a single workgroup may declare all of it (MI355X_MICROARCH.md): the
// 8-wave tiles take as many stages (up to MM_MAX_STAGES = 3) as fit; the 4-wave tiles always use three (42-84 KB).
constexpr int LDS_BUDGET = MM_LDS_BUDGET;

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
#if !(MM_DBG & 2048)   // ablation 2048: no waits for the DMA
    mm::wait_vmcnt<N>();
#endif
}
// workgroup barrier that does NOT drain the DMA queue (a __syncthreads() would add vmcnt(0))
__device__ __forceinline__ void barrier_lds_only() {
#if (MM_DBG & 1024)
    MM_DEVICE_ONLY(asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");)   // ablation: no workgroup barrier (results are garbage)
#else
    MM_DEVICE_ONLY(asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");)
#endif
}

// ---------------------------------------------------------------------------------------------------------
// Operand geometry.  KD = K depth of one pipeline slab: 128 everywhere except the fp4 x fp4 segment, whose slabs are 256 deep.
// Why: an LDS-DMA instruction costs the memory pipeline per 128-byte cache line it touches, not per byte (measured: the DMA-only
// loop of the fp4 x fp4 segment took 2050 cycles per 128-deep slab of 34 KB, the fp8 x fp4 one 1700 cycles for 50 KB -- both
// touch 72 lines per wave).  A 128-deep slab of an fp4 operand is 64 bytes per row, i.e. HALF a line per row and slab, fetched
// again by the next slab; a 256-deep slab takes whole lines (128 B per row), halving the line requests of that segment.
// ---------------------------------------------------------------------------------------------------------
template <int EL, int KD> struct Op;
template <> struct Op<EL_FP8, 128> { static constexpr int PITCH = 128, G128 = 128; };   // PITCH: LDS row pitch; G128: global bytes per row and 128 K
template <> struct Op<EL_FP6, 128> { static constexpr int PITCH = 128, G128 = 96; };
template <> struct Op<EL_FP4, 128> { static constexpr int PITCH = 64, G128 = 64; };
template <> struct Op<EL_FP4, 256> { static constexpr int PITCH = 128, G128 = 64; };

// fragment types: the register tuple handed to the MFMA has exactly the width the format needs
template <int EL> struct Frag;
template <> struct Frag<EL_FP8> { typedef int type __attribute__((ext_vector_type(8))); };
template <> struct Frag<EL_FP6> { typedef int type __attribute__((ext_vector_type(6))); };
template <> struct Frag<EL_FP4> { typedef int type __attribute__((ext_vector_type(4))); };

// Per-lane byte offsets (inside an operand tile) of the pieces of a fragment, for MFMA tile 0 of the wave and K
// step h (64 deep) of the slab.  Tile t adds the compile-time constant t * 32 * PITCH (the swizzle term only depends on row & 31).
// Layouts (measured, tests/test_hw_gpu.py): fp4/fp6 lanes hold the 32 consecutive elements of K block 2h + kb;
// fp8 lanes hold K = 64h + 16kb + [0,16) in registers 0-3 and K = 64h + 32 + 16kb + [0,16) in registers 4-7.
// 128-byte rows are XOR-swizzled in 16-byte chunks with (row >> 1) & 7, 64-byte rows with (row >> 2) & 3: every ds_read_b128
// of a fragment is bank-conflict free (the DMA applies the same permutation on the SOURCE address).
template <int EL, int KD> struct FragOfs;
template <> struct FragOfs<EL_FP8, 128> {
    int o[2][2];
    __device__ __forceinline__ void init(int row, int kb) {
        const int sw = (row >> 1) & 7, rb = row * 128;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            o[h][0] = rb + (((4 * h + kb) ^ sw) << 4);
            o[h][1] = rb + (((4 * h + 2 + kb) ^ sw) << 4);
        }
    }
};
template <> struct FragOfs<EL_FP4, 128> {
    int o[2][1];
    __device__ __forceinline__ void init(int row, int kb) {
        const int sw = (row >> 2) & 3, rb = row * 64;
#pragma unroll
        for (int h = 0; h < 2; ++h) o[h][0] = rb + (((2 * h + kb) ^ sw) << 4);
    }
};
template <> struct FragOfs<EL_FP4, 256> {
    int o[4][1];
    __device__ __forceinline__ void init(int row, int kb) {
        const int sw = (row >> 1) & 7, rb = row * 128;
#pragma unroll
        for (int h = 0; h < 4; ++h) o[h][0] = rb + (((2 * h + kb) ^ sw) << 4);
    }
};
template <> struct FragOfs<EL_FP6, 128> {
    int o[2][3];
    __device__ __forceinline__ void init(int row, int kb) {
        const int sw = (row >> 1) & 7, rb = row * 128;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int u = 3 * (2 * h + kb) + i;  // 8-byte unit of the 96-byte row
                o[h][i] = rb + (((u >> 1) ^ sw) << 4) + ((u & 1) << 3);
            }
    }
};

template <int EL, int KD, int H>
__device__ __forceinline__ typename Frag<EL>::type load_frag(const uint8_t *tile, const FragOfs<EL, KD> &fo, int t) {
    const uint8_t *p = tile + t * 32 * Op<EL, KD>::PITCH;
    typename Frag<EL>::type r;
    if constexpr (EL == EL_FP8) {
        const uint4 lo = *reinterpret_cast<const uint4 *>(p + fo.o[H][0]);
        const uint4 hi = *reinterpret_cast<const uint4 *>(p + fo.o[H][1]);
        r = typename Frag<EL>::type{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
    } else if constexpr (EL == EL_FP4) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p + fo.o[H][0]);
        r = typename Frag<EL>::type{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
    } else {
        const uint2 t0 = *reinterpret_cast<const uint2 *>(p + fo.o[H][0]);
        const uint2 t1 = *reinterpret_cast<const uint2 *>(p + fo.o[H][1]);
        const uint2 t2 = *reinterpret_cast<const uint2 *>(p + fo.o[H][2]);
        r = typename Frag<EL>::type{(int)t0.x, (int)t0.y, (int)t1.x, (int)t1.y, (int)t2.x, (int)t2.y};
    }
    return r;
}

// Compact offsets of an fp8 operand (round 6; the fp8 x fp8 segment of the matching-precision mode, whose 256-row kernel has no VGPR
// to spare: two full fragment sets of 8-register fragments are 96 VGPRs).  The swizzle is an XOR on chunk bits that the K step h
// (bit 2 of the chunk index) and the fragment half i (bit 1) do not share with the row term, so
//     o[h][i] = o[0][0] ^ (h << 6 | i << 5),
// and because every operand tile starts at a multiple of 128 bytes of LDS (the workgroup's dynamic LDS starts at 0: the kernels have no
// static LDS -- the build guard checks group_segment_fixed_size == 0 -- and stages, operand offsets and MFMA row tiles are multiples of
// 128) the XOR commutes with adding the tile's base:  address(h, i) = (tile + o[0][0]) ^ (h << 6 | i << 5).
// ONE register per operand instead of four; per K step one v_add and one to two v_xor per operand where there were two v_add.  (The sum
// changes with the stage, so LLVM cannot hoist the XORs out of the K loop as it does with `o[0][0] ^ constant`.)
template <int EL, int KD> struct FragOfsC;
template <> struct FragOfsC<EL_FP8, 128> {
    int o00;
    __device__ __forceinline__ void init(int row, int kb) { o00 = row * 128 + ((kb ^ ((row >> 1) & 7)) << 4); }
};
template <int EL, int KD, int H>
__device__ __forceinline__ typename Frag<EL>::type load_frag(const uint8_t *tile, const FragOfsC<EL, KD> &fo, int t) {
    static_assert(EL == EL_FP8 && KD == 128, "compact offsets exist for 128-byte fp8 rows");
    typedef unsigned u4_t __attribute__((ext_vector_type(4)));          // (a builtin vector: HIP's uint4 class cannot be read through address space 3)
    typedef const u4_t __attribute__((address_space(3))) *lds_u4;
    const unsigned a00 = (unsigned)(unsigned long long)tile + (unsigned)fo.o00;   // (the LDS address: the low half of the flat pointer)
    const unsigned a0 = (a00 ^ (unsigned)(H << 6)) + (unsigned)(t * 32 * 128), a1 = (a00 ^ (unsigned)((H << 6) | 32)) + (unsigned)(t * 32 * 128);
    const u4_t lo = *(lds_u4)(unsigned long)a0;
    const u4_t hi = *(lds_u4)(unsigned long)a1;
    return typename Frag<EL>::type{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}
// the offsets type of an operand inside segment geometry G
template <class G, int EL> using FragOfsOf = std::conditional_t<G::XEL == EL_FP8 && G::WEL == EL_FP8 && !MM_SMALL, FragOfsC<EL, G::KD>, FragOfs<EL, G::KD>>;

// ---------------------------------------------------------------------------------------------------------
// accumulators in a[0:NACC-1]: tile (tm, tn) = a[16 * (tn * TM + tm) .. + 15]
// ---------------------------------------------------------------------------------------------------------
// FENCE: the statement also carries a "memory" clobber, so hipcc cannot hoist the LDS reads that follow it in the source
// above it (used on the first MFMAs after a barrier: the matrix pipe gets work before the wave spends ~100 cycles
// issuing the next fragments' ds_reads).  HSEL = op_sel_hi of both scale operands: the scale bytes 0/1 (HSEL = 0) or 2/3
// (HSEL = 1) of the lane's scale dword, already shifted by 8 * kb, i.e. K block 2 * HSEL + kb of the 128-deep scale atom.
// ZC: the tile's FIRST K step (the ping-pong kernel, which never zeroes its accumulators): srcC is the inline constant 0 and the
// accumulator is only written.  0 + x in the matrix pipe is what accumulating onto a zeroed register gives, bit for bit.
template <int T, int XEL, int WEL, int HSEL, bool FENCE = false, bool ZC = false>
__device__ __forceinline__ void mfma_tile(const typename Frag<XEL>::type &x, const typename Frag<WEL>::type &w, int sx,
                                          int sw) {
    // s_nop 1: two wait states between a just-written source VGPR (a compiler v_mov assembling the tuple, the
    // scale shift) and the MFMA that reads it -- hipcc pads nothing inside or in front of an asm statement.
#if !(MM_DBG & 1)
    if constexpr (ZC) {   // (always a fence: these are the first MFMAs behind a barrier)
        MM_DEVICE_ONLY(asm volatile("s_nop 1\n\tv_mfma_scale_f32_32x32x64_f8f6f4 a[%c7:%c8], %0, %1, 0, %2, %3 "
                                    "op_sel_hi:[%c4,%c4,0] cbsz:%c5 blgp:%c6"
                                    :
                                    : "v"(x), "v"(w), "v"(sx), "v"(sw), "i"(HSEL), "i"(ElemTraits<XEL>::HW),
                                      "i"(ElemTraits<WEL>::HW), "i"(16 * T), "i"(16 * T + 15)
                                    : MM_ACC, "memory");)
    } else if constexpr (FENCE) {
        MM_DEVICE_ONLY(asm volatile("s_nop 1\n\tv_mfma_scale_f32_32x32x64_f8f6f4 a[%c7:%c8], %0, %1, a[%c7:%c8], %2, %3 "
                                    "op_sel_hi:[%c4,%c4,0] cbsz:%c5 blgp:%c6"
                                    :
                                    : "v"(x), "v"(w), "v"(sx), "v"(sw), "i"(HSEL), "i"(ElemTraits<XEL>::HW),
                                      "i"(ElemTraits<WEL>::HW), "i"(16 * T), "i"(16 * T + 15)
                                    : MM_ACC, "memory");)
    } else {
        MM_DEVICE_ONLY(asm volatile("s_nop 1\n\tv_mfma_scale_f32_32x32x64_f8f6f4 a[%c7:%c8], %0, %1, a[%c7:%c8], %2, %3 "
                                    "op_sel_hi:[%c4,%c4,0] cbsz:%c5 blgp:%c6"
                                    :
                                    : "v"(x), "v"(w), "v"(sx), "v"(sw), "i"(HSEL), "i"(ElemTraits<XEL>::HW),
                                      "i"(ElemTraits<WEL>::HW), "i"(16 * T), "i"(16 * T + 15)
                                    : MM_ACC);)
    }
#else
    MM_DEVICE_ONLY(asm volatile("" ::"v"(x), "v"(w), "v"(sx), "v"(sw));)
#endif
}

template <int I>
__device__ __forceinline__ float acc_read() {
    float v = 0.0f;
    MM_DEVICE_ONLY(asm volatile("v_accvgpr_read_b32 %0, a[%c1]" : "=v"(v) : "i"(I) : MM_ACC);)
    return v;
}
template <int I>
__device__ __forceinline__ void acc_write(float v) {
    MM_DEVICE_ONLY(asm volatile("v_accvgpr_write_b32 a[%c1], %0" : : "v"(v), "i"(I) : MM_ACC);)
}
// an MFMA result may be read by a VALU instruction only 18+ wait states after the MFMA issued (16-pass XDL op)
__device__ __forceinline__ void acc_settle() { MM_DEVICE_ONLY(asm volatile("s_nop 15\n\ts_nop 7" ::: MM_ACC);) }

template <int I, int N>
struct AccLoop {
    static __device__ __forceinline__ void zero() {
        acc_write<I>(0.0f);
        AccLoop<I + 1, N>::zero();
    }
    // D = bf16(acc) of the reference's chained kernels, in place, eight accumulators per statement: v_cvt_pk_bf16_f32 (RNE, a
    // NaN stays a NaN) rounds two at a time, a shift / a mask put each back into the high half of a dword.  3.5 instructions
    // per value (the integer formulation took ~10), and the four pairs of a statement are interleaved so that no instruction
    // waits for the one before it (a dependent chain per pair ran at VALU latency: ~3 k cycles per segment boundary).
    static __device__ __forceinline__ void round_bf16() {
        static_assert(I % 8 == 0 && N % 8 == 0, "accumulators are rounded eight at a time");
        MM_DEVICE_ONLY(unsigned r0, r1, r2, r3, r4, r5, r6, r7, p0, p1, p2, p3;
                       asm volatile("v_accvgpr_read_b32 %0, a[%c12]\n\tv_accvgpr_read_b32 %1, a[%c13]\n\t"
                                    "v_accvgpr_read_b32 %2, a[%c14]\n\tv_accvgpr_read_b32 %3, a[%c15]\n\t"
                                    "v_accvgpr_read_b32 %4, a[%c16]\n\tv_accvgpr_read_b32 %5, a[%c17]\n\t"
                                    "v_accvgpr_read_b32 %6, a[%c18]\n\tv_accvgpr_read_b32 %7, a[%c19]\n\t"
                                    "v_cvt_pk_bf16_f32 %8, %0, %1\n\tv_cvt_pk_bf16_f32 %9, %2, %3\n\t"
                                    "v_cvt_pk_bf16_f32 %10, %4, %5\n\tv_cvt_pk_bf16_f32 %11, %6, %7\n\t"
                                    "v_lshlrev_b32 %0, 16, %8\n\tv_and_b32 %1, 0xffff0000, %8\n\t"
                                    "v_lshlrev_b32 %2, 16, %9\n\tv_and_b32 %3, 0xffff0000, %9\n\t"
                                    "v_lshlrev_b32 %4, 16, %10\n\tv_and_b32 %5, 0xffff0000, %10\n\t"
                                    "v_lshlrev_b32 %6, 16, %11\n\tv_and_b32 %7, 0xffff0000, %11\n\t"
                                    "v_accvgpr_write_b32 a[%c12], %0\n\tv_accvgpr_write_b32 a[%c13], %1\n\t"
                                    "v_accvgpr_write_b32 a[%c14], %2\n\tv_accvgpr_write_b32 a[%c15], %3\n\t"
                                    "v_accvgpr_write_b32 a[%c16], %4\n\tv_accvgpr_write_b32 a[%c17], %5\n\t"
                                    "v_accvgpr_write_b32 a[%c18], %6\n\tv_accvgpr_write_b32 a[%c19], %7"
                                    : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7),
                                      "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3)
                                    : "i"(I), "i"(I + 1), "i"(I + 2), "i"(I + 3), "i"(I + 4), "i"(I + 5), "i"(I + 6), "i"(I + 7)
                                    : MM_ACC);)
        AccLoop<I + 8, N>::round_bf16();
    }
    // split-K partial sums: registers I .. I+3 of every lane -> 16 bytes at p[(I / 4) * NT * 4] (p already includes 4 * the thread
    // index): a wave instruction writes 1 KB side by side, write-through (the reader is another launch).  down_proj
    // (12288,1024,1024) at M = 128 / 256 / 512 through the C ABI: plain 4-byte stores of one register each 21.0 / 26.1 / 39.5 us,
    // the same write-through 20.2 / 24.7 / 39.1, 16 bytes write-through 20.2 / 24.8 / 39.0 (profiles/notes_r03.md section 19).
    static __device__ __forceinline__ void store(float *p) {
        static_assert(I % 4 == 0 && N % 4 == 0, "four accumulator registers per store");
        [[maybe_unused]] const v4f v = {acc_read<I>(), acc_read<I + 1>(), acc_read<I + 2>(), acc_read<I + 3>()};
        MM_DEVICE_ONLY(asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p + (I / 4) * NT * 4), "v"(v) : "memory");)
        AccLoop<I + 4, N>::store(p);
    }
};
template <int N>
struct AccLoop<N, N> {
    static __device__ __forceinline__ void zero() {}
    static __device__ __forceinline__ void round_bf16() {}
    static __device__ __forceinline__ void store(float *) {}
};

// ---------------------------------------------------------------------------------------------------------
// LDS-DMA of one slab, cut into pieces so that one piece can be issued between two MFMAs
// ---------------------------------------------------------------------------------------------------------
// The DMA instructions are issued from inline asm, NOT through the raw_buffer_load_lds builtin: hipcc (ROCm 7.2)
// orders every later ds_read behind a pending builtin LDS-DMA with an s_waitcnt vmcnt(0), which drains the whole
// prefetch queue once per K slab (measured: the loop then runs at DMA latency, ~47 % MFMA utilisation).  With asm
// the compiler does not see the LDS writes; ordering is ours: counted s_waitcnt vmcnt(N), then the workgroup
// barrier, then the reads (all asm statements carry a "memory" clobber).
// The descriptors (make_rsrc for the DMA; make_brsrc, compiler-visible, for the loads into registers of the 4-wave tiles,
// run_slabs_small), lds_address and the DMA instruction itself are mm::'s, mx_buffer_ops.h.  Here only the "no DMA" ablation:
__device__ __forceinline__ void dma16(const rsrc_t &rsrc, int voff, int soff, unsigned lds_addr) {
#if (MM_DBG & 2)
    MM_DEVICE_ONLY(asm volatile("" ::"v"(voff), "s"(rsrc), "s"(lds_addr), "s"(soff));)
#else
    mm::dma16(rsrc, voff, soff, lds_addr);
#endif
}
constexpr int OOB = 1 << 30;   // added to a lane's byte offset it puts the lane past any descriptor: the load returns zero (not for free)

// One operand of one segment: descriptor over the tile's rows (rows past the matrix edge read as zero and their
// outputs are masked) and the per-lane offset of DMA piece 0; piece `it` adds it * ROWS_PER_IT * rowbytes.
// The type depends on the LDS row pitch only; the element format enters through g128 (global bytes per row and 128 K: 64 fp4,
// 96 fp6, 128 fp8), a run-time member, so that the fp6 and fp8 activation segments (and the fp6 / fp8 weights of the
// matching-precision mode) share one type -- a segment can then request its SUCCESSOR's first slabs through a descriptor chosen
// at run time (run_slabs_big, "chaining").
template <int PITCH, int ROWS>
struct OperandDma {
    static constexpr int CPR = PITCH / 16;                 // 16-byte chunks per LDS row
    static constexpr int PIECES = ROWS * CPR / NT;         // DMA instructions per thread per slab
    static_assert(ROWS * CPR % NT == 0, "tile must be a whole number of wave instructions");
    static constexpr int ROWS_PER_IT = NT / CPR;
    rsrc_t rsrc;
    __amdgpu_buffer_rsrc_t brsrc;   // SMALL tiles only
    int voff0;
    int rowbytes;
    int g128;
    __device__ __forceinline__ void init(const uint8_t *base, int row0, int nrows, int nslab128, int g128_) {
        g128 = __builtin_amdgcn_readfirstlane(g128_);
        rowbytes = __builtin_amdgcn_readfirstlane(nslab128 * g128);
        int rows = nrows - row0;
        rows = rows > ROWS ? ROWS : rows;
        if constexpr (SMALL) brsrc = make_brsrc(base + (size_t)row0 * (unsigned)rowbytes, (unsigned)rows * (unsigned)rowbytes);
        if constexpr (!SMALL) rsrc = make_rsrc(base + (size_t)row0 * (unsigned)rowbytes, (unsigned)rows * (unsigned)rowbytes);
        const int tid = mm_tid() & (NT - 1);   // loader waves of the 4-wave tiles are threads NT .. 2 NT - 1
        const int row = tid / CPR;
        int c;
        if constexpr (CPR == 4) c = (tid & 3) ^ ((row >> 2) & 3);
        else c = (tid & 7) ^ ((row >> 1) & 7);
        // ROWS_PER_IT is a multiple of 32 for both pitches, so the swizzle term is the same for every piece
        if (g128 == 96) c = c >= 6 ? c - 6 : c;  // fp6 rows are 96 B: the pad chunks re-read valid bytes
        voff0 = row * rowbytes + c * 16;
    }
    // slab128 = index of the slab's first 128-deep K unit inside the segment
    template <int IT>
    __device__ __forceinline__ void piece(int slab128, const uint8_t *lds_tile, int wave) const {
#if (MM_DBG & 16384)
        // ablation: 128-byte rows fetched as HALF lines (an instruction covers 16 rows x 64 B instead of 8 rows x 128 B): the same
        // bytes and instruction count, twice the cache-line requests; results are garbage (the LDS image no longer matches)
        if constexpr (CPR == 8 && PIECES == 4) {
            const int tid = mm_tid() & (NT - 1);
            const int v = ((IT >> 1) * (NT / 4) + (tid >> 2)) * rowbytes + ((tid & 3) + 4 * (IT & 1)) * 16;
            dma16(rsrc, v, __builtin_amdgcn_readfirstlane(slab128 * g128),
                  __builtin_amdgcn_readfirstlane(lds_address(lds_tile) + (IT * NT + wave * 64) * 16));
            return;
        }
#endif
        dma16(rsrc, voff0 + IT * ROWS_PER_IT * rowbytes, __builtin_amdgcn_readfirstlane(slab128 * g128),
              __builtin_amdgcn_readfirstlane(lds_address(lds_tile) + (IT * NT + wave * 64) * 16));
    }
    // the same piece through registers: load<IT> now, store<IT> (same LDS bytes as the DMA would write) when it has arrived
    template <int IT>
    __device__ __forceinline__ v4i load(int slab128, int oob) const {
        return __builtin_amdgcn_raw_buffer_load_b128(brsrc, voff0 + IT * ROWS_PER_IT * rowbytes + oob,
                                                     __builtin_amdgcn_readfirstlane(slab128 * g128), 0);
    }
    template <int IT>
    __device__ __forceinline__ void store(const v4i &v, uint8_t *lds_tile) const {
        *reinterpret_cast<v4i *>(lds_tile + (IT * NT + (threadIdx.x & (NT - 1))) * 16) = v;
    }
};

// Scale-factor atoms of one operand (512 B = 128 rows x one 128-deep K unit; the reference layout, consumed as is).
// KD = 128: ONE instruction brings the atoms of the tile's two row tiles for the slab (lanes 0-31 / 32-63) -> LDS [rt][512].
// KD = 256: one instruction PER ROW TILE brings its two consecutive atoms (1 KiB contiguous in memory)    -> LDS [rt][ka][512].
template <int KD>
struct SfDma {
    rsrc_t rsrc;
    __amdgpu_buffer_rsrc_t brsrc;   // SMALL tiles only
    int voff[KD / 128];
    __device__ __forceinline__ void init(const uint8_t *sf, int row0, int row_tiles, int nslab128) {
        if constexpr (SMALL) brsrc = make_brsrc(sf, (unsigned)row_tiles * (unsigned)nslab128 * 512u);
        else rsrc = make_rsrc(sf, (unsigned)row_tiles * (unsigned)nslab128 * 512u);
        const int lane = mm_tid() & 63;
        if constexpr (KD == 128) {
            int rt = (row0 >> 7) + (lane >> 5);
            rt = rt < row_tiles ? rt : row_tiles - 1;
            voff[0] = rt * nslab128 * 512 + (lane & 31) * 16;
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                int rt = (row0 >> 7) + r;
                rt = rt < row_tiles ? rt : row_tiles - 1;
                voff[r] = rt * nslab128 * 512 + (lane >> 5) * 512 + (lane & 31) * 16;
            }
        }
    }
    // R: row tile of the piece (KD = 256 only)
    template <int R>
    __device__ __forceinline__ void issue(int slab128, const uint8_t *lds_sf) const {
        dma16(rsrc, voff[R], __builtin_amdgcn_readfirstlane(slab128 * 512),
              __builtin_amdgcn_readfirstlane(lds_address(lds_sf) + R * 1024));
    }
    template <int R>
    __device__ __forceinline__ v4i load(int slab128, int oob) const {
        return __builtin_amdgcn_raw_buffer_load_b128(brsrc, voff[R] + oob, __builtin_amdgcn_readfirstlane(slab128 * 512), 0);
    }
    template <int R>
    __device__ __forceinline__ void store(const v4i &v, uint8_t *lds_sf) const {
        *reinterpret_cast<v4i *>(lds_sf + R * 1024 + (threadIdx.x & 63) * 16) = v;
    }
};

// The 8-wave tiles: the scale pieces of a slab are issued by waves 0 .. 2 * KD / 128 - 1, ONE piece each (SlabDmaT::piece), so a wave
// needs one descriptor, one per-lane offset and one LDS offset, chosen once by its wave index -- not both operands' SfDma (two
// descriptors = 8 SGPRs, 2-4 offset VGPRs).  Round 6: the matching-precision 256-row kernel sat at 128 VGPRs + 1 spilled register whose
// reload inside the K loop carried an `s_waitcnt vmcnt(0)`, i.e. drained the DMA ring once per slab (VERDICT r5, weak #1).
//   KD = 128: wave 0 -> activations' atoms of both row tiles (lanes 0-31 / 32-63), wave 1 -> the weights'
//   KD = 256: waves 0 / 1 -> row tile 0 / 1 of the activations (two consecutive atoms each), waves 2 / 3 -> the weights'
template <int KD>
struct SfSel {
    rsrc_t rsrc;
    int voff;
    int lds_off;      // from the stage base
    __device__ __forceinline__ void init(const uint8_t *sfx, const uint8_t *sfw, int m0, int n0, int xrt, int wrt, int nslab128, int wave,
                                         int off_sfx, int off_sfw) {
        const bool is_w = KD == 128 ? (wave & 1) != 0 : (wave & 2) != 0;
        const uint8_t *sf = is_w ? sfw : sfx;
        const int row0 = is_w ? n0 : m0, row_tiles = is_w ? wrt : xrt;
        rsrc = make_rsrc(sf, (unsigned)row_tiles * (unsigned)nslab128 * 512u);
        const int lane = mm_tid() & 63;
        if constexpr (KD == 128) {
            int rt = (row0 >> 7) + (lane >> 5);
            rt = rt < row_tiles ? rt : row_tiles - 1;
            voff = rt * nslab128 * 512 + (lane & 31) * 16;
            lds_off = is_w ? off_sfw : off_sfx;
        } else {
            const int r = wave & 1;
            int rt = (row0 >> 7) + r;
            rt = rt < row_tiles ? rt : row_tiles - 1;
            voff = rt * nslab128 * 512 + (lane >> 5) * 512 + (lane & 31) * 16;
            lds_off = (is_w ? off_sfw : off_sfx) + r * 1024;
        }
    }
    __device__ __forceinline__ void issue(int slab128, const uint8_t *stage) const {
        dma16(rsrc, voff, __builtin_amdgcn_readfirstlane(slab128 * 512), __builtin_amdgcn_readfirstlane(lds_address(stage) + lds_off));
    }
};
struct SfNone {};

// Stage geometry of one segment kind
template <int XEL_, int WEL_, int KD_>
struct Geom {
    static constexpr int XEL = XEL_, WEL = WEL_, KD = KD_;
    static constexpr int KSTEPS = KD / 64;                       // 64-deep MFMA K steps per slab
    static constexpr int X_BYTES = BM * Op<XEL, KD>::PITCH, W_BYTES = BN * Op<WEL, KD>::PITCH;
    static constexpr int SF_EACH = (KD / 128) * 1024;            // two row tiles x KD/128 atoms per operand
    static constexpr int OFF_W = X_BYTES, OFF_SFX = OFF_W + W_BYTES, OFF_SFW = OFF_SFX + SF_EACH, STAGE = OFF_SFW + SF_EACH;
    // A slab is consumed in ~0.25-1 us but its DMA takes 1-3 us to land when any of its lines misses L2, so the DMA runs
    // NSTAGE - 1 slabs ahead of the MFMAs: three stages where they fit, two otherwise (the 256-deep fp4 x fp4 slabs of the
    // 256-row tile; fp8 weights).  The 128-row tiles (launches with too few tiles to fill the chip) would fit four to six
    // stages, and 256-deep fp6 / fp8 slabs too; both were measured on them (M = 128 .. 2048, Llama shapes) and changed nothing
    // beyond +-2 %: with two MFMAs per wave and K step those workgroups are bound by the LDS round trip of the next step's
    // fragments (~350 cycles per 64-deep step), not by DMA latency or per-slab overhead.  Reading the fragments a whole pair of
    // K steps ahead into a second register set (all ds_reads of a pair issued right after the barrier) was SLOWER by up to 25 %:
    // after a barrier all eight waves then read LDS at the same time and run MFMAs at the same time, instead of each wave
    // interleaving its reads with its MFMAs.  (A generic stage count also made the
    // matching-precision 256-row kernel, which sits at the 128-register limit of two waves per SIMD, spill 316 bytes per lane.)
    // Requesting the NEXT segment's first slab from a segment's last step (same ring: "chained"; other geometry: into a free
    // LDS range) was built twice and measured at +-1 % of the loop cycles: a boundary is the rounding, not the pipeline fill.
    // (The 4-wave tiles use exactly three stages as an exchange buffer between their loader and compute waves: run_slabs_small.
    // Up to eight DMA stages on them, with the 8-wave pipeline, did not change their 0.4 us per slab.)
    static constexpr int NSTAGE = LDS_BUDGET / STAGE >= MM_MAX_STAGES ? MM_MAX_STAGES : (LDS_BUDGET / STAGE >= 2 ? LDS_BUDGET / STAGE : 2);
    static_assert(2 * STAGE <= LDS_BUDGET, "two stages must fit");
    static constexpr int BYTES = NSTAGE * STAGE;
    static_assert(STAGE % 128 == 0 && OFF_W % 128 == 0, "operand tiles start at multiples of 128 bytes (FragOfsC)");
};

// The DMA side of one segment kind: both operands and their scale atoms.  Keyed by the LDS pitches and the slab depth (not by the
// element formats, see OperandDma), so the S and O segments share one type.
template <int XPITCH, int WPITCH, int KD_>
struct SlabDmaT {
    static constexpr int KD = KD_;
    static constexpr int OFF_W = BM * XPITCH, OFF_SFX = OFF_W + BN * WPITCH, OFF_SFW = OFF_SFX + (KD / 128) * 1024,
                         STAGE = OFF_SFW + (KD / 128) * 1024;
    OperandDma<XPITCH, BM> x;
    OperandDma<WPITCH, BN> w;
    std::conditional_t<SMALL, SfDma<KD>, SfNone> sfx, sfw;   // the loader / compute tiles: loads into registers (load / store below)
    std::conditional_t<SMALL, SfNone, SfSel<KD>> sf;          // the 8-wave tiles: this wave's one scale piece
    int wave;
    int first128;   // first 128-deep K unit of the segment this workgroup walks (0 unless split-K or the odd tail of the fp4 segment)
    static constexpr int XP = OperandDma<XPITCH, BM>::PIECES, WP = OperandDma<WPITCH, BN>::PIECES;
    static constexpr int NPIECES = XP + WP + 1;
    // segment Q of problem `a` for the tile at (m0, n0); gx128 / gw128 = global bytes per row and 128 K of the two operands
    __device__ __forceinline__ void init(const GemmArgs &a, int Q, int m0, int n0, int nslab128, int first, int wave_, int gx128, int gw128) {
        x.init(a.X[Q], m0, a.M, nslab128, gx128);
        w.init(a.W[Q], n0, a.N, nslab128, gw128);
        if constexpr (SMALL) {
            sfx.init(a.SFX[Q], m0, a.sfx_row_tiles, nslab128);
            sfw.init(a.SFW[Q], n0, a.sfw_row_tiles, nslab128);
        } else {
            sf.init(a.SFX[Q], a.SFW[Q], m0, n0, a.sfx_row_tiles, a.sfw_row_tiles, nslab128, wave_, OFF_SFX, OFF_SFW);
        }
        wave = wave_;
        first128 = first;
    }
    __device__ __forceinline__ int unit(int slab) const { return __builtin_amdgcn_readfirstlane(first128 + slab * (KD / 128)); }
    // The scale pieces of a slab (KD = 128: one for each operand, KD = 256: two) are issued by waves 0 .. SFW - 1 only: those waves
    // have NPIECES DMA instructions in flight per slab, the others NPIECES - 1 (run_slabs_big waits with the matching count).
    // Round 2 let EVERY wave issue one (the surplus waves repeated a piece) to keep one vmcnt immediate: 6 KB of 56 KB per slab of
    // the fp8 x fp4 segment were duplicates, and what a slab costs is the bytes the DMA moves (tools/gemm_clock.py ablations).
    static constexpr int SFW = 2 * (KD / 128);
    __device__ __forceinline__ bool sf_wave() const { return wave < SFW; }
    // piece P of slab `slab` (in KD units, relative to first128) into `stage`
    template <int P>
    __device__ __forceinline__ void piece(int slab, uint8_t *stage) const {
        const int u = unit(slab);
        if constexpr (P < XP) {
            x.template piece<P>(u, stage, wave);
        } else if constexpr (P < XP + WP) {
            w.template piece<P - XP>(u, stage + OFF_W, wave);
        } else if constexpr (SMALL) {
            // (the register path of the loader / compute tiles does not use this function)
        } else {
            if (wave < SFW) sf.issue(u, stage);
        }
    }
    template <int P = 0>
    __device__ __forceinline__ void all(int slab, uint8_t *stage) const {
        if constexpr (P < NPIECES) {
            piece<P>(slab, stage);
            all<P + 1>(slab, stage);
        }
    }
    // the register path of the 4-wave tiles: piece P of slab `slab` (zeros when the slab is past `count`; callers do not ask).
    // Every loader wave carries a scale piece (dealt by wave & 1 / wave & 3; with four loader waves the 128-deep geometry repeats each).
    template <int P>
    __device__ __forceinline__ v4i load(int slab, int count) const {
        const int u = unit(slab), oob = slab < count ? 0 : OOB;
        if constexpr (P < XP) {
            return x.template load<P>(u, oob);
        } else if constexpr (P < XP + WP) {
            return w.template load<P - XP>(u, oob);
        } else if constexpr (KD == 128) {
            return (wave & 1) ? sfw.template load<0>(u, oob) : sfx.template load<0>(u, oob);
        } else {
            const int k = wave & 3;
            return k == 0 ? sfx.template load<0>(u, oob) : k == 1 ? sfx.template load<1>(u, oob)
                 : k == 2 ? sfw.template load<0>(u, oob) : sfw.template load<1>(u, oob);
        }
    }
    template <int P>
    __device__ __forceinline__ void store(const v4i &v, uint8_t *stage) const {
        if constexpr (P < XP) {
            x.template store<P>(v, stage);
        } else if constexpr (P < XP + WP) {
            w.template store<P - XP>(v, stage + OFF_W);
        } else if constexpr (KD == 128) {
            if (wave & 1) sfw.template store<0>(v, stage + OFF_SFW);
            else sfx.template store<0>(v, stage + OFF_SFX);
        } else {
            const int k = wave & 3;
            if (k == 0) sfx.template store<0>(v, stage + OFF_SFX);
            else if (k == 1) sfx.template store<1>(v, stage + OFF_SFX);
            else if (k == 2) sfw.template store<0>(v, stage + OFF_SFW);
            else sfw.template store<1>(v, stage + OFF_SFW);
        }
    }
};
template <class G> using SlabDma = SlabDmaT<Op<G::XEL, G::KD>::PITCH, Op<G::WEL, G::KD>::PITCH, G::KD>;
template <class G>
__device__ __forceinline__ void init_slab_dma(SlabDma<G> &dma, const GemmArgs &a, int Q, int m0, int n0, int nslab128, int first, int wave) {
    static_assert(SlabDma<G>::STAGE == G::STAGE && SlabDma<G>::OFF_W == G::OFF_W && SlabDma<G>::OFF_SFW == G::OFF_SFW, "stage layout");
    dma.init(a, Q, m0, n0, nslab128, first, wave, Op<G::XEL, G::KD>::G128, Op<G::WEL, G::KD>::G128);
}

// scale dwords of the lane for one slab: [128-deep K unit of the slab][MFMA tile]
template <int KD>
struct Scales {
    int x[KD / 128][TM];
    int w[KD / 128][TN];
};

template <class G>
__device__ __forceinline__ void load_scales(Scales<G::KD> &sc, const uint8_t *stage, int gx, int gw, int li, int kb) {
    // SF atom = 128 rows: 16 bytes per (row & 31) = 4 row groups x 4 K blocks.  gx / gw = the 32-row group, counted from the
    // first row of the first atom the DMA brought (SfDma: the atom of row0 >> 7), at which the wave's TM*32 activation rows /
    // TN*32 weight rows start: group & 3 of atom group >> 2.
    constexpr int RT = G::KD == 128 ? 512 : 1024;    // LDS distance between the row tiles' atoms (see SfDma)
    const uint8_t *px = stage + G::OFF_SFX + (gx >> 2) * RT + li * 16 + (gx & 3) * 4;
    const uint8_t *pw = stage + G::OFF_SFW + (gw >> 2) * RT + li * 16 + (gw & 3) * 4;
    const int sh = 8 * kb;  // the lane's K block inside the 64-deep step; op_sel_hi then picks the step
#pragma unroll
    for (int ka = 0; ka < G::KD / 128; ++ka) {
        if constexpr (TM == 4) {
            const uint4 sx = *reinterpret_cast<const uint4 *>(px + ka * 512);
            sc.x[ka][0] = (int)(sx.x >> sh);
            sc.x[ka][1] = (int)(sx.y >> sh);
            sc.x[ka][2] = (int)(sx.z >> sh);
            sc.x[ka][3] = (int)(sx.w >> sh);
        } else if constexpr (TM == 2) {
            const uint2 sx = *reinterpret_cast<const uint2 *>(px + ka * 512);
            sc.x[ka][0] = (int)(sx.x >> sh);
            sc.x[ka][1] = (int)(sx.y >> sh);
        } else {
            sc.x[ka][0] = (int)(*reinterpret_cast<const uint32_t *>(px + ka * 512) >> sh);
        }
        if constexpr (TN == 4) {
            const uint4 sw = *reinterpret_cast<const uint4 *>(pw + ka * 512);
            sc.w[ka][0] = (int)(sw.x >> sh);
            sc.w[ka][1] = (int)(sw.y >> sh);
            sc.w[ka][2] = (int)(sw.z >> sh);
            sc.w[ka][3] = (int)(sw.w >> sh);
        } else if constexpr (TN == 2) {
            const uint2 sw = *reinterpret_cast<const uint2 *>(pw + ka * 512);
            sc.w[ka][0] = (int)(sw.x >> sh);
            sc.w[ka][1] = (int)(sw.y >> sh);
        } else {
            sc.w[ka][0] = (int)(*reinterpret_cast<const uint32_t *>(pw + ka * 512) >> sh);
        }
    }
}

// TM*TN MFMAs of one 64-deep K step on fragment set (xc, wc).  Interleaved with them, in this issue order:
//   the TM + TN fragment reads of the NEXT step (activations first, then weights), spread evenly over the MFMA slots;
//   from slot DMA_FIRST on, the DP::N DMA pieces of the policy object `dp`, spread evenly over the remaining slots.
// The MFMAs that are followed by reads are memory fences for the compiler, so the reads stay behind them.
template <int L, class LX, class LW>
__device__ __forceinline__ void issue_load(LX &load_x, LW &load_w) {
#if (MM_DBG & 512)
    return;  // ablation: no fragment reads in the loop (the MFMAs reuse the first fragments)
#endif
    if constexpr (L < TM) load_x(std::integral_constant<int, L>{});
    else load_w(std::integral_constant<int, L - TM>{});
}
template <int L, int LEND, class LX, class LW>
__device__ __forceinline__ void issue_loads(LX &load_x, LW &load_w) {
    if constexpr (L < LEND) {
        issue_load<L>(load_x, load_w);
        issue_loads<L + 1, LEND>(load_x, load_w);
    }
}
template <class DP, int D, int DEND>
__device__ __forceinline__ void issue_pieces(const DP &dp) {
    if constexpr (D < DEND) {
        dp.template piece<D>();
        issue_pieces<DP, D + 1, DEND>(dp);
    }
}
struct NoDma {
    static constexpr int N = 0;
    static constexpr bool FENCE = false;
    template <int P> __device__ __forceinline__ void piece() const {}
};
// HSEL: which half of the lane's scale dwords this step uses (see mfma_tile)
template <int XEL, int WEL, int HSEL, class DP, int P = 0, class LX, class LW>
__device__ __forceinline__ void mfma_step(const typename Frag<XEL>::type (&xc)[TM], const typename Frag<WEL>::type (&wc)[TN],
                                          const int (&sx)[TM], const int (&sw)[TN], const DP &dp, LX load_x, LW load_w) {
    constexpr int NM = TM * TN, NL = TM + TN, DMA_FIRST = NM > 1 ? 1 : 0, ND = NM - DMA_FIRST;
    if constexpr (P < NM) {
        constexpr int tn = P / TM, tm = P % TM;
        constexpr int l0 = P * NL / NM, l1 = (P + 1) * NL / NM;          // reads issued after this MFMA
        mfma_tile<tn * TM + tm, XEL, WEL, HSEL, (l1 > l0) || DP::FENCE>(xc[tm], wc[tn], sx[tm], sw[tn]);
        issue_loads<l0, l1>(load_x, load_w);
        if constexpr (DP::N > 0 && P >= DMA_FIRST) {
            constexpr int d0 = (P - DMA_FIRST) * DP::N / ND, d1 = (P - DMA_FIRST + 1) * DP::N / ND;
            issue_pieces<DP, d0, d1>(dp);
        }
        mfma_step<XEL, WEL, HSEL, DP, P + 1>(xc, wc, sx, sw, dp, load_x, load_w);
    }
}

// ---------------------------------------------------------------------------------------------------------
// The slab pipeline: both operands move in slabs of the same depth KD through NSTAGE stages
// (fp4 x fp4 segment: KD = 256, two stages; the other segments: KD = 128, three stages with fp4 weights, two otherwise)
// ---------------------------------------------------------------------------------------------------------
// K steps 0 .. KSTEPS-2 of a slab: they alternate between the two fragment sets, each loading the next step's fragments from
// the SAME stage in the shadow of its first MFMAs.
template <class G, int H, class XA, class WA, class FX, class FW>
__device__ __forceinline__ void inner_steps(XA &xa, XA &xb, WA &wa, WA &wb, const Scales<G::KD> &sc,
                                            const FX &fx, const FW &fw, const uint8_t *st) {
    if constexpr (H < G::KSTEPS - 1) {
        mfma_step<G::XEL, G::WEL, (H & 1), NoDma>(
            xa, wa, sc.x[H >> 1], sc.w[H >> 1], NoDma{},
            [&](auto t) { xb[decltype(t)::value] = load_frag<G::XEL, G::KD, H + 1>(st, fx, decltype(t)::value); },
            [&](auto t) { wb[decltype(t)::value] = load_frag<G::WEL, G::KD, H + 1>(st + G::OFF_W, fw, decltype(t)::value); });
        inner_steps<G, H + 1>(xb, xa, wb, wa, sc, fx, fw, st);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Slab pipeline of the 4-wave tiles (WM == 2): 64-row tiles for launches of a few dozen to a few hundred workgroups.
// Such a launch has one workgroup per CU and little MFMA work per slab, so nothing hides the latencies of a wave that does
// everything in order: with the 8-wave pipeline below (or any variant of it: deeper DMA rings, whole-slab read-ahead, operands
// staged through registers by the same waves) a workgroup walked a 128-deep slab in 0.3-0.5 us whatever the tile size
// (tools/mid_m_sweep.py, tools/mid_ksweep.py: 13-17 us for K = 4096 from M = 65 to M = 768; ablations: global loads, LDS
// writes, fragment reads and the barrier each added ~0.1 us, i.e. they did not overlap).  So the waves SPECIALISE:
//   waves 0-3 (compute): read the fragments and scales of slab s+1 from LDS into a second register set, run the MFMAs of
//                        slab s, barrier;
//   waves 4-7 (loaders): hold three slabs in flight in registers (plain buffer loads: LDS-DMA moves ~50 GB/s per CU however many
//                        waves issue it, register loads 83-124 GB/s, tools/l2_bw.py); per slab they write the slot of slab s+2
//                        to its LDS stage (ds_write_b128: the bytes the DMA would have written, same swizzle), refill the slot
//                        with slab s+2+R, barrier.
// One barrier per slab, shared by both roles: barrier s publishes slab s+2 and certifies that the compute waves hold slab s+1
// in registers.  Three stages (slab j in stage j % 3), R = 3 slots (slab j in slot j % 3).  Nothing is conditional in the
// loaders beyond one wave-uniform test per slab: slabs past the end are not requested and never computed on.
// Measured (M = 128, N = K = 4096, fp8 x fp4, 64 x 64 tiles, loop cycles per slab, tools/gemm_clock.py M=128): 628 = 128 (empty
// loop with its barrier) + 200 (fragment reads: 24 KB per slab) + 217 (ds_write of the 12 KB slab) + 80 (global loads); without
// MFMAs the same.  The LDS pipe is the bound -- reads and writes of different waves add up -- and a barrier per TWO slabs
// (four stages) changed nothing.  Still 11 us against 17 us for the 8-wave 128 x 128 tiles at M <= 256.
// ---------------------------------------------------------------------------------------------------------
template <class G>
struct SlabRegs {
    typename Frag<G::XEL>::type x[G::KSTEPS][TM];
    typename Frag<G::WEL>::type w[G::KSTEPS][TN];
    Scales<G::KD> sc;
};
template <class G, int H = 0>
__device__ __forceinline__ void read_slab(SlabRegs<G> &r, const uint8_t *st, const FragOfs<G::XEL, G::KD> &fx,
                                          const FragOfs<G::WEL, G::KD> &fw) {
    if constexpr (H < G::KSTEPS) {
#pragma unroll
        for (int t = 0; t < TM; ++t) r.x[H][t] = load_frag<G::XEL, G::KD, H>(st, fx, t);
#pragma unroll
        for (int t = 0; t < TN; ++t) r.w[H][t] = load_frag<G::WEL, G::KD, H>(st + G::OFF_W, fw, t);
        read_slab<G, H + 1>(r, st, fx, fw);
    }
}
template <int EL>
__device__ __forceinline__ v8i widen_frag(const typename Frag<EL>::type &f) {
    if constexpr (EL == EL_FP8) return v8i{f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7]};
    else if constexpr (EL == EL_FP6) return v8i{f[0], f[1], f[2], f[3], f[4], f[5], 0, 0};
    else return v8i{f[0], f[1], f[2], f[3], 0, 0, 0, 0};
}
// the MFMAs of one slab on compiler-owned accumulators (4-wave tiles).  Scale bytes as in mfma_tile: the lane's scale dword is
// already shifted by 8 * kb, step H takes byte 2 * (H & 1) of the 128-deep unit H >> 1.
template <class G, int H = 0>
__device__ __forceinline__ void mfma_slab(Acc &acc, const SlabRegs<G> &r) {
#if MM_SMALL
    if constexpr (H < G::KSTEPS) {
#if !(MM_DBG & 1)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
                acc.t[tn * TM + tm] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                    widen_frag<G::XEL>(r.x[H][tm]), widen_frag<G::WEL>(r.w[H][tn]), acc.t[tn * TM + tm], ElemTraits<G::XEL>::HW,
                    ElemTraits<G::WEL>::HW, 2 * (H & 1), r.sc.x[H >> 1][tm], 2 * (H & 1), r.sc.w[H >> 1][tn]);
#endif
        mfma_slab<G, H + 1>(acc, r);
    }
#endif
}
template <class G>
struct SlabSlot {
    v4i q[SlabDma<G>::NPIECES];
    template <int P = 0>
    __device__ __forceinline__ void load(const SlabDma<G> &dma, int slab, int count) {
        if constexpr (P < SlabDma<G>::NPIECES) {
            q[P] = dma.template load<P>(slab, count);
            load<P + 1>(dma, slab, count);
        }
    }
    template <int P = 0>
    __device__ __forceinline__ void store(const SlabDma<G> &dma, uint8_t *stage) const {
        if constexpr (P < SlabDma<G>::NPIECES) {
            dma.template store<P>(q[P], stage);
            store<P + 1>(dma, stage);
        }
    }
};

template <class G, class PRE>
__device__ __forceinline__ void run_slabs_small(Acc &acc, const GemmArgs &a, int Q, int nslab128, int first128, int count, int m0, int n0,
                                                uint8_t *smem, PRE pre) {
    constexpr int XEL = G::XEL, WEL = G::WEL, KD = G::KD;
    static_assert(G::NSTAGE >= 3, "the 4-wave pipeline uses three LDS stages");
    const int lane = mm_tid() & 63, wave = __builtin_amdgcn_readfirstlane(mm_tid() >> 6);
    uint8_t *const st0 = smem, *const st1 = smem + G::STAGE, *const st2 = smem + 2 * G::STAGE;
    // 6 slabs per round in both roles: the stage pattern (period 3), the slots (period 3) and the register sets (period 2)
    // all line up, and both roles pass exactly one barrier per slab.  F(J, stage of slab s+1, stage of slab s+2, s), J = s % 6.
#define MM_ROUND6(F)                                   \
    for (int s = 0; s < count; s += 6) {               \
        F(0, st1, st2, s);                             \
        if (s + 1 < count) F(1, st2, st0, s + 1);      \
        if (s + 2 < count) F(2, st0, st1, s + 2);      \
        if (s + 3 < count) F(3, st1, st2, s + 3);      \
        if (s + 4 < count) F(4, st2, st0, s + 4);      \
        if (s + 5 < count) F(5, st0, st1, s + 5);      \
    }
    if (wave >= NT / 64) {
        // ---------------- loader waves ----------------
        SlabDma<G> dma;
        init_slab_dma<G>(dma, a, Q, m0, n0, nslab128, first128, wave - NT / 64);      // index among the loader waves
        constexpr int R = 3;   // slabs in flight in registers (four, with 12-slab rounds, measured: +3 % time on three-segment splits)
        SlabSlot<G> q[R];
        // slabs past the end are not requested (wave-uniform branch; their slots go to LDS as they are and are never computed on).
        // Requesting them out of range instead -- the load returns zeros -- kept the loop branch-free but cost 0.8 us per launch of
        // a three-segment split: out-of-range buffer loads are not free.
#define MM_QLOAD(Q, S) if ((S) < count) Q.load(dma, S, count)
        MM_QLOAD(q[0], 0);
        MM_QLOAD(q[1], 1);
        MM_QLOAD(q[2], 2);
        q[0].store(dma, st0);
        MM_QLOAD(q[0], R);
        q[1].store(dma, st1);
        MM_QLOAD(q[1], R + 1);
        barrier_lds_only();   // slabs 0 and 1 are published
        // slab s: the slot of slab s+2 goes to its stage (the one slab s-1 has left) and is refilled with slab s+2+R
#define MM_LOADER(J, S_NEXT, S_AFTER, S)                                             \
    {                                                                                \
        if constexpr (!(MM_DBG & 8)) q[((J) + 2) % R].store(dma, S_AFTER);           \
        if constexpr (!(MM_DBG & 4)) { MM_QLOAD(q[((J) + 2) % R], (S) + 2 + R); }            \
        barrier_lds_only();                                                          \
    }
        MM_ROUND6(MM_LOADER)
#undef MM_LOADER
#undef MM_QLOAD
        return;
    }
    // ---------------- compute waves ----------------
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, kb = lane >> 5;
    pre();
    FragOfs<XEL, KD> fx;
    FragOfs<WEL, KD> fw;
    fx.init(wm * (TM * 32) + li, kb);
    fw.init(wn * (TN * 32) + li, kb);
    const int gx = ((m0 & 127) >> 5) + wm * TM, gw = ((n0 & 127) >> 5) + wn * TN;
    barrier_lds_only();
    SlabRegs<G> r[2];
    read_slab<G>(r[0], st0, fx, fw);
    load_scales<G>(r[0].sc, st0, gx, gw, li, kb);
    // slab s: computes on one register set while the other receives slab s+1
#define MM_COMPUTE(J, S_NEXT, S_AFTER, S)                                \
    {                                                                    \
        if constexpr (!(MM_DBG & 32)) {                                  \
            read_slab<G>(r[((J) + 1) & 1], S_NEXT, fx, fw);              \
            load_scales<G>(r[((J) + 1) & 1].sc, S_NEXT, gx, gw, li, kb); \
        }                                                                \
        mfma_slab<G>(acc, r[(J) & 1]);                                   \
        MM_DEVICE_ONLY(__builtin_amdgcn_sched_barrier(0);)   /* the MFMAs are issued before the wave waits at the barrier */ \
        barrier_lds_only();                                              \
    }
    MM_ROUND6(MM_COMPUTE)
#undef MM_COMPUTE
#undef MM_ROUND6
}

// DMA policies of the last K step of a slab (mfma_step issues DP::N pieces between its MFMAs)
template <class D>
struct SlabPiecesT {      // all pieces of slab `slab` of `dma` into `stage`
    static constexpr int N = D::NPIECES;
    static constexpr bool FENCE = false;
    const D &dma;
    int slab;
    uint8_t *stage;
    template <int P> __device__ __forceinline__ void piece() const { dma.template piece<P>(slab, stage); }
};
template <class D>
struct TwoSlabPieces {    // slabs 1 and 2 (those below `pref`) of a successor segment into its stages 1 and 2
    static constexpr int N = 2 * D::NPIECES;
    static constexpr bool FENCE = false;
    const D &dma;
    int pref;
    uint8_t *smem;
    template <int P> __device__ __forceinline__ void piece() const {
        constexpr int j = 1 + P / D::NPIECES;
        if (j < pref) dma.template piece<P % D::NPIECES>(j, smem + j * D::STAGE);
    }
};
// at most K slabs' worth of this wave's DMA instructions may stay in flight (waves that issue a scale piece have one more per slab)
template <int K, class D>
__device__ __forceinline__ void wait_slabs(const D &dma) {
    if constexpr (K == 0) {
        wait_vmcnt<0>();
    } else {
        static_assert(K * D::NPIECES < 64, "vmcnt is a 6-bit counter");
        if (dma.sf_wave()) wait_vmcnt<K * D::NPIECES>();
        else wait_vmcnt<K * (D::NPIECES - 1)>();
    }
}

// ---------------------------------------------------------------------------------------------------------
// Tile-major tail (the TAIL kernels: 256 x 256 tile, fp4 weights, bf16 output, no split-K, no fused activation; the last segment).
// Before: every CU ran its K loop to the end and then stored its 128 KiB at once; that write-out (~5 us at 4096^3, the HBM write
// rate with every CU storing, matrix pipe idle) was ~10 % of the launch.  Here the last TWO slabs of the launch, both resident in
// LDS once the last DMA has landed, are computed tile by tile so that finished output tiles leave while the MFMAs of the others
// still run.  The wave's 2 x 4 accumulator tiles go in four groups (tm, tn pair): per group eight MFMAs -- the four K steps of the
// two slabs on both tiles, alternating between the tiles so that no MFMA waits for the one before it; every accumulator receives
// its K steps in the order the slab-major loop gives them, so the sums are bit for bit the same.  Between those eight MFMAs runs
// the PREVIOUS group's epilogue: the rounding of write_tile (bf16, + bias, bf16) into a wave-private [32 rows][64 features] image,
// then 16-byte row-contiguous write-through stores of whole 128-byte lines.  The images live in the third stage of the ring,
// which held slab count - 3 and is free from the barrier of that slab on.  The fragments of a group are read from LDS when the
// group starts (the loop's two full fragment sets would not fit next to a second set for the next group).
// ---------------------------------------------------------------------------------------------------------
constexpr int TAIL_EP = 192;   // row pitch of a tail image: 48 dwords = 16 mod 32 banks, so the two rows a 32-lane half writes per
                               // ds_write_b32 fall on disjoint banks, and rows two apart start 32 banks apart (the row reads)
// Z0: the tail is the tile's whole K loop (the ping-pong kernel at count = 2, which never zeroes its accumulators): the first K step of
// every accumulator takes the constant 0 as srcC (mfma_tile's ZC).
template <class G, class FX, class FW, bool Z0 = false>
struct TailTM {
    using XF = typename Frag<G::XEL>::type;
    using WF = typename Frag<G::WEL>::type;
    static_assert(TM == 2 && TN == 4 && G::KSTEPS == 2 && G::NSTAGE == 3, "the tail is written out for the 256 x 256 tile on a three-stage 128-deep ring");
    // byte arithmetic: 8 waves x 32 rows x 192 B = 48 KiB of images in one 50 KiB stage (fp8 x fp4: 32 + 16 + 2 KiB)
    static_assert((NT / 64) * 32 * TAIL_EP <= G::STAGE, "the tail images fit in the stage the tail frees");
    const GemmArgs &a;
    const uint8_t *sa, *sb;      // stages of slab count - 2 and count - 1
    uint8_t *img;                // this wave's image
    const FX &fx;
    const FW &fw;
    Scales<G::KD> sca, scb;
    float bias[TN];
    int m0w, n0w;                // first token / feature of the wave's block
    int lane, li, hi;
    unsigned sel;
    XF xs[4];                    // the four K steps of the group's activation fragment (tm)
    WF ws[2][4];                 // ... and of its two weight fragments

    template <int TM_>
    __device__ __forceinline__ void load_x() {
        xs[0] = load_frag<G::XEL, G::KD, 0>(sa, fx, TM_);
        xs[1] = load_frag<G::XEL, G::KD, 1>(sa, fx, TM_);
        xs[2] = load_frag<G::XEL, G::KD, 0>(sb, fx, TM_);
        xs[3] = load_frag<G::XEL, G::KD, 1>(sb, fx, TM_);
    }
    template <int TN_>
    __device__ __forceinline__ void load_w(WF (&w)[4]) {
        w[0] = load_frag<G::WEL, G::KD, 0>(sa + G::OFF_W, fw, TN_);
        w[1] = load_frag<G::WEL, G::KD, 1>(sa + G::OFF_W, fw, TN_);
        w[2] = load_frag<G::WEL, G::KD, 0>(sb + G::OFF_W, fw, TN_);
        w[3] = load_frag<G::WEL, G::KD, 1>(sb + G::OFF_W, fw, TN_);
    }
    // MFMA I of group (TM_, P): K step I >> 1 on tile J = I & 1 of the pair
    template <int TM_, int P, int I>
    __device__ __forceinline__ void mfma() {
        constexpr int J = I & 1, H = I >> 1, TN_ = 2 * P + J;
        const Scales<G::KD> &sc = H < 2 ? sca : scb;
        mfma_tile<TN_ * TM + TM_, G::XEL, G::WEL, (H & 1), true, Z0 && H == 0>(xs[H], ws[J][H], sc.x[0][TM_], sc.w[0][TN_]);
    }
    // (v0, v1) = this lane's feature at tokens t, t + 1 -> features (li & ~1, li | 1) at token t + (lane & 1): write_tile's pair_to_token
    __device__ __forceinline__ unsigned pair_to_token(float v0, float v1, float b) const {
        unsigned out = 0;
        MM_DEVICE_ONLY(
            unsigned p;
            asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(p) : "v"(v0), "v"(v1));
            if (a.bias != nullptr) {
                const float r0 = __uint_as_float(p << 16) + b, r1 = __uint_as_float(p & 0xFFFF0000u) + b;
                asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(p) : "v"(r0), "v"(r1));
            }
            const unsigned other = (unsigned)__builtin_amdgcn_mov_dpp((int)p, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
            out = __builtin_amdgcn_perm(other, p, sel);)
        return out;
    }
    // chunk C of group (TM_, P)'s rounding: registers 4q .. 4q + 3 (tokens 8q + 4hi + 0..3) of tile J = C >> 2, q = C & 3
    template <int TM_, int P, int C>
    __device__ __forceinline__ void round_chunk() {
        constexpr int J = C >> 2, Q = C & 3, T = (2 * P + J) * TM + TM_;
        if constexpr (C == 0) acc_settle();   // the group's last MFMA issued one MFMA ago at least; 18 wait states before a VALU read
        const float v0 = acc_read<16 * T + 4 * Q>(), v1 = acc_read<16 * T + 4 * Q + 1>();
        const float v2 = acc_read<16 * T + 4 * Q + 2>(), v3 = acc_read<16 * T + 4 * Q + 3>();
        uint8_t *wr = img + (4 * hi + (lane & 1)) * TAIL_EP + (li & ~1) * 2 + J * 64;
        *reinterpret_cast<unsigned *>(wr + (8 * Q) * TAIL_EP) = pair_to_token(v0, v1, bias[2 * P + J]);
        *reinterpret_cast<unsigned *>(wr + (8 * Q + 2) * TAIL_EP) = pair_to_token(v2, v3, bias[2 * P + J]);
    }
    // the image of group (TM_, P) to D: four wave instructions of eight 128-byte rows (write_tile's TN = 2 row mapping)
    template <int TM_, int P>
    __device__ __forceinline__ void store_group() {
        const int rgrp = ((0x96 >> ((lane >> 2) & 7)) & 1) + 2 * hi, ridx = ((lane >> 3) & 3) * 4 + (lane & 3);
        const bool vec_ok = (a.N & 7) == 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int rowl = 8 * j + (rgrp & 1) + 4 * (rgrp >> 1) + 2 * (ridx >> 3), ch = ridx & 7;
            const uint4 v = *reinterpret_cast<const uint4 *>(img + rowl * TAIL_EP + ch * 16);
            const int m = m0w + TM_ * 32 + rowl, n = n0w + P * 64 + ch * 8;
            if (m < a.M) {
                uint16_t *dst = a.D + (size_t)m * a.N + n;
                if (vec_ok && n + 7 < a.N) {
                    typedef unsigned v4u __attribute__((ext_vector_type(4)));
                    [[maybe_unused]] const v4u vv = {v.x, v.y, v.z, v.w};
                    MM_DEVICE_ONLY(asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(dst), "v"(vv) : "memory");)
                } else {
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (n + e < a.N) dst[e] = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
                }
            }
        }
    }
    // group GI = (tm, tn pair) = (GI >> 1, GI & 1): its fragments, its eight MFMAs with group GI - 1's rounding between them, then
    // group GI - 1's stores.  GI = 4: the last group's rounding and stores, nothing left to hide them behind.
    template <int GI, int I = 0>
    __device__ __forceinline__ void mfmas_with_rounding() {
        if constexpr (I < 8) {
            mfma<(GI >> 1), (GI & 1), I>();
            if constexpr (GI > 0) round_chunk<((GI - 1) >> 1), ((GI - 1) & 1), I>();
            mfmas_with_rounding<GI, I + 1>();
        }
    }
    template <int GI>
    __device__ __forceinline__ void group() {
        if constexpr (GI < 4) {
            constexpr int TM_ = GI >> 1, P = GI & 1;
            if constexpr (P == 0) load_x<TM_>();
            load_w<2 * P>(ws[0]);
            load_w<2 * P + 1>(ws[1]);
            mfmas_with_rounding<GI>();
        } else {
#if MM_CLOCKS
            // loop end of the TAIL kernels: the last MFMA is issued (raw stamps; tile_body makes them relative to its start)
            if (a.clock_out != nullptr && mm_tid() == 0) {
                a.clock_out[4 * blockIdx.x] = __builtin_amdgcn_s_memtime();
                a.clock_out[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
            }
#endif
            round_chunk<1, 1, 0>(); round_chunk<1, 1, 1>(); round_chunk<1, 1, 2>(); round_chunk<1, 1, 3>();
            round_chunk<1, 1, 4>(); round_chunk<1, 1, 5>(); round_chunk<1, 1, 6>(); round_chunk<1, 1, 7>();
        }
        if constexpr (GI > 0) store_group<((GI - 1) >> 1), ((GI - 1) & 1)>();
        if constexpr (GI < 4) group<GI + 1>();
    }
};

// The tail itself: called in place of the loop's last two iterations.  On entry stage c2 holds slab count - 2 (complete), stage c1
// slab count - 1 (in flight), stage cf nothing that any wave still reads.  Z0: the accumulators are unwritten on entry (TailTM).
template <class G, bool Z0 = false, class FX, class FW>
__device__ __forceinline__ void run_tail(const GemmArgs &a, int m0, int n0, uint8_t *smem, int c2, int c1, int cf, const Scales<G::KD> &sca,
                                         const FX &fx, const FW &fw, int gx, int gw) {
    const int lane = mm_tid() & 63, wave = __builtin_amdgcn_readfirstlane(mm_tid() >> 6);
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, kb = lane >> 5;
    wait_vmcnt<0>();       // this thread's share of slab count - 1 has landed ...
    barrier_lds_only();    // ... and every thread's
    TailTM<G, FX, FW, Z0> t{a, smem + c2 * G::STAGE, smem + c1 * G::STAGE, smem + cf * G::STAGE + wave * (32 * TAIL_EP), fx, fw};
    t.sca = sca;
    load_scales<G>(t.scb, t.sb, gx, gw, li, kb);
    t.m0w = m0 + wm * (TM * 32);
    t.n0w = n0 + wn * (TN * 32);
    t.lane = lane;
    t.li = li;
    t.hi = lane >> 5;
    t.sel = (lane & 1) ? 0x03020706u : 0x05040100u;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int n = t.n0w + tn * 32 + li;
        t.bias[tn] = (a.bias != nullptr && n < a.N) ? bf16_bits_to_f32(a.bias[n]) : 0.0f;
    }
    t.template group<0>();
}

// Chaining.  A segment's successor: while segment A walks its last slabs it requests the first `pref` slabs of segment B
// (pref = min(B's stages, B's slabs); 0 = no chaining), so that B starts with slab 0 in LDS, certified by A's last barrier, and
// slabs 1 .. pref-1 in flight -- exactly the state B's own prologue would have produced, minus the prologue.  Without it a segment
// boundary costs the issue of up to three slabs of DMA (the issue itself blocks: the memory pipeline takes a 1 KB DMA instruction
// every ~40 cycles), their landing, a barrier and the accumulator rounding in a row: ~3.3 k cycles + ~2.2 k of rounding per
// boundary at 4096^3 (tools/gemm_clock.py, fused vs reference rounding).  With it: ~1.5 k cycles fused, ~2.9 k with the reference
// rounding (the rounding now sits exposed, after B's first fragment reads are issued; it used to overlap the landing of the
// first slab, which is why round 2 measured chaining alone at +-1 %).
//   SAME geometry (S -> O: equal stage size, stage count and piece counts): B's slabs continue A's ring.
//   DIFFERENT geometry (the 256-deep fp4 segment, two 68 KB stages -> a 128-deep segment, stages of 50 / 66 KB at 0, STAGE, ...):
//     A starts its ring so that its LAST slab sits in its stage 1; then B's stage 0 lies inside A's stage 0, which is free from the
//     barrier of A's second-to-last slab on (B's slab 0 is requested there), and B's stages 1 and 2 become free at the barrier of
//     A's last slab (B's slabs 1 and 2 are requested there).
// (the successor's descriptor travels as a reference parameter `nxd` next to `pref`: everything stays in SGPRs after inlining)

// One run of `count` slabs (KD deep) of segment Q, starting at its 128-deep K unit `first128`, through a DMA pipeline of
// G::NSTAGE stages.  pref_in = 0: no DMA is in flight on entry and every wave is past its last LDS read; the first slabs are
// requested here.  pref_in > 0 (chained in): the predecessor requested slabs 0 .. pref_in-1, slab 0 (in stage cur0) is complete.
// `pre` runs once before the first MFMA: the place for work that needs no LDS and no matrix pipe (the bf16 rounding of the
// accumulators between two segments); unchained it sits between the issue of the first DMAs and the wait for them.
// Returns the ring position after the last slab (where a same-geometry successor's slab 0 lies).
// CH = false: no successor (nx is ignored) and never chained in.
// TAIL: the last segment of a TAIL kernel (count >= 2, no successor): the last two slabs run tile-major and write the output (run_tail).
template <class G, bool CH, class NX, class PRE, bool TAIL = false>
__device__ __forceinline__ int run_slabs_big(const GemmArgs &a, int Q, int nslab128, int first128, int count, int m0, int n0,
                                             uint8_t *smem, PRE pre, int pref_in, int cur0, const NX &nxd, int nx_pref) {
    constexpr int XEL = G::XEL, WEL = G::WEL, KD = G::KD;
    constexpr bool SAME = CH && (KD == NX::KD), DIFF = CH && (KD != NX::KD);
    static_assert(!TAIL || G::NSTAGE == 3, "the tail runs on a three-stage ring");
    static_assert(!SAME || (NX::STAGE == G::STAGE && NX::NPIECES == SlabDma<G>::NPIECES), "a same-geometry successor continues the ring");
    const int lane = mm_tid() & 63, wave = __builtin_amdgcn_readfirstlane(mm_tid() >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, kb = lane >> 5;

    SlabDma<G> dma;
    init_slab_dma<G>(dma, a, Q, m0, n0, nslab128, first128, wave);

    constexpr int NS = G::NSTAGE;
    static_assert(NS == 2 || NS == 3, "this pipeline is written out for two or three stages");
    static_assert(!DIFF || NS == 2, "a successor of another geometry needs the two-stage ring (see Chaining above run_slabs_big)");
    auto stage_at = [&](int i) { return smem + i * G::STAGE; };
    auto next_of = [&](int i) { return (i + 1 == NS) ? 0 : i + 1; };
    int cur = cur0;
    // The ring's stream: this segment's slabs, then (SAME) the successor's first nx_pref.  On entry its first pref_in slabs have
    // been requested by the predecessor; request the rest of the first NS here (a chained-in segment shorter than the ring still
    // owes its successor's first slabs), then -- unless chained in -- wait for slab 0 only.
    const int vcount = count + (SAME ? nx_pref : 0);
    {
        int st = cur;
#pragma unroll
        for (int v = 0; v < NS; ++v) {
            if (v >= pref_in) {
                if (v < count) dma.all(v, stage_at(st));
                else if (SAME && v < vcount) nxd.all(v - count, stage_at(st));
            }
            st = next_of(st);
        }
    }
    if (pref_in == 0) {
        pre();
        if (NS == 3 && vcount > 2) wait_slabs<2>(dma);
        else if (vcount > 1) wait_slabs<1>(dma);
        else wait_slabs<0>(dma);
        barrier_lds_only();
    }

    FragOfsOf<G, XEL> fx;
    FragOfsOf<G, WEL> fw;
    fx.init(wm * (TM * 32) + li, kb);
    fw.init(wn * (TN * 32) + li, kb);
    // two fragment sets; K step h of a slab computes on set h & 1 (the number of K steps per slab is even)
    typename Frag<XEL>::type x0[TM], x1[TM];
    typename Frag<WEL>::type w0[TN], w1[TN];
    Scales<KD> sc;
#pragma unroll
    for (int t = 0; t < TM; ++t) x0[t] = load_frag<XEL, KD, 0>(stage_at(cur), fx, t);
#pragma unroll
    for (int t = 0; t < TN; ++t) w0[t] = load_frag<WEL, KD, 0>(stage_at(cur) + G::OFF_W, fw, t);
    // 32-row groups of the wave's rows inside the scale atoms in LDS (tiles narrower than an atom start at m0 & 127 / n0 & 127)
    const int gx = ((m0 & 127) >> 5) + wm * TM, gw = ((n0 & 127) >> 5) + wn * TN;
    load_scales<G>(sc, stage_at(cur), gx, gw, li, kb);
    // Chained in: the rounding runs while the first fragments travel from LDS.  (Rounding tile by tile in front of each tile's
    // first MFMA of the new segment instead, so that the matrix pipe starts on the tiles that are done, was measured at 76.9 k
    // against 75.1 k loop cycles for (2048,128,1920) at 4096^3: the rounding is VALU-bound -- ~3.5 instructions per value on
    // accumulators that live in AGPRs -- and the eight MFMAs it could hide are a fraction of it; not kept.)
    if (pref_in != 0) pre();

#ifdef MM_PRESSURE
    int keep_[MM_PRESSURE];
#pragma unroll
    for (int i = 0; i < MM_PRESSURE; ++i) { keep_[i] = lane * (i + 3); MM_DEVICE_ONLY(asm volatile("" : "+v"(keep_[i]));) }
#endif
    for (int s = 0; s < (TAIL ? count - 2 : count); ++s) {
        const int nxt = next_of(cur);
        uint8_t *st_cur = stage_at(cur);
        uint8_t *st_nxt = stage_at(nxt);
        // K steps 0 .. KSTEPS-2 on the current stage
        inner_steps<G, 0>(x0, x1, w0, w1, sc, fx, fw, st_cur);
        // Wait for this thread's share of slab s+1 and nothing younger: of the slabs requested so far (up to s+NS-1) the ones
        // after s+1 may stay in flight.  (With a successor of another geometry the ring has two stages: everything is waited for.)
        if (NS == 3 && s + 2 < vcount) wait_slabs<1>(dma);
        else wait_slabs<0>(dma);
        // then the barrier: every wave has its last-step fragments in registers, so stage[cur] is free, and slab s+1 is
        // complete in LDS
        barrier_lds_only();
        // last K step on (x1, w1); meanwhile step 0 of the next slab is read from the next stage and the DMA of slab s+NS
        // refills stage[cur] (one DMA instruction per MFMA).  Past the segment's end the successor's first slabs are requested
        // instead (see "Chaining" above run_slabs_big); without one there is nothing left to request (and in the very last iteration the fragments
        // read ahead are never used).
        Scales<KD> scn;
        load_scales<G>(scn, st_nxt, gx, gw, li, kb);
        auto lx = [&](auto t) { x0[decltype(t)::value] = load_frag<XEL, KD, 0>(st_nxt, fx, decltype(t)::value); };
        auto lw = [&](auto t) { w0[decltype(t)::value] = load_frag<WEL, KD, 0>(st_nxt + G::OFF_W, fw, decltype(t)::value); };
        constexpr int HL = G::KSTEPS - 1;
        const int v = s + NS;
        if (v < count) {
            mfma_step<XEL, WEL, (HL & 1), SlabPiecesT<SlabDma<G>>>(x1, w1, sc.x[HL >> 1], sc.w[HL >> 1], SlabPiecesT<SlabDma<G>>{dma, v, st_cur}, lx, lw);
        } else if (SAME && v - count < nx_pref) {
            mfma_step<XEL, WEL, (HL & 1), SlabPiecesT<NX>>(x1, w1, sc.x[HL >> 1], sc.w[HL >> 1], SlabPiecesT<NX>{nxd, v - count, st_cur}, lx, lw);
        } else if (DIFF && nx_pref > 0 && v == count) {           // second-to-last slab: the successor's stage 0 is free
            mfma_step<XEL, WEL, (HL & 1), SlabPiecesT<NX>>(x1, w1, sc.x[HL >> 1], sc.w[HL >> 1], SlabPiecesT<NX>{nxd, 0, smem}, lx, lw);
        } else if (DIFF && nx_pref > 1 && v == count + 1) {       // last slab: its stages 1 and 2 are
            mfma_step<XEL, WEL, (HL & 1), TwoSlabPieces<NX>>(x1, w1, sc.x[HL >> 1], sc.w[HL >> 1], TwoSlabPieces<NX>{nxd, nx_pref, smem}, lx, lw);
        } else {
            mfma_step<XEL, WEL, (HL & 1), NoDma>(x1, w1, sc.x[HL >> 1], sc.w[HL >> 1], NoDma{}, lx, lw);
        }
        sc = scn;
        cur = nxt;
    }
#ifdef MM_PRESSURE
#pragma unroll
    for (int i = 0; i < MM_PRESSURE; ++i) { MM_DEVICE_ONLY(asm volatile("" ::"v"(keep_[i]));) }
#endif
    if constexpr (TAIL) {
        // slab count - 2 is in stage cur, count - 1 in the next; the third held count - 3 (or nothing when count = 2)
        run_tail<G>(a, m0, n0, smem, cur, next_of(cur), next_of(next_of(cur)), sc, fx, fw, gx, gw);
    }
    return cur;
}

template <class G, bool CH, class NX, class PRE, bool TAIL = false>
__device__ __forceinline__ int run_slabs(Acc &acc, const GemmArgs &a, int Q, int nslab128, int first128, int count, int m0, int n0,
                                         uint8_t *smem, PRE pre, int pref_in, int cur0, const NX &nxd, int nx_pref) {
    if constexpr (SMALL) {
        static_assert(!TAIL, "the tail belongs to the 8-wave pipeline");
        run_slabs_small<G>(acc, a, Q, nslab128, first128, count, m0, n0, smem, pre);
        return 0;
    } else {
        return run_slabs_big<G, CH, NX, PRE, TAIL>(a, Q, nslab128, first128, count, m0, n0, smem, pre, pref_in, cur0, nxd, nx_pref);
    }
}

// The geometries of the three segments.  The fp4 x fp4 segment runs 256-deep slabs (see Op) and, when its width is an odd
// multiple of 128, one last 128-deep slab on the 128-deep geometry.
// Tried for the fp6 / fp8 activation segments against fp4 weights and NOT kept (git history: "dual-ring pipeline"): activation
// slabs 128 deep and the fp4 weight rows 256 deep (whole cache lines for the weights too) through two rings of two slots each.
// 25 % fewer line requests, results identical, but 82.5 k loop cycles against 78.5 k and 41.4 against 39.3 us at 4096^3 on the
// same device: the super-slab of four steps with two unequal barriers loses more than the lines save.  Likewise two stages
// instead of three (MM_FORCE_NS2 experiment): fewer cycles (76.5 k), but 0 ... +5 % time depending on the device.
template <bool W4> struct Segs {
    using N256 = Geom<EL_FP4, EL_FP4, 256>;
    using N128 = Geom<EL_FP4, EL_FP4, 128>;
    using S = Geom<EL_FP6, (W4 ? EL_FP4 : EL_FP6), 128>;
    using O = Geom<EL_FP8, (W4 ? EL_FP4 : EL_FP8), 128>;
    using DmaSO = SlabDma<S>;                                  // the S and O segments share their DMA type (OperandDma)
    static_assert(std::is_same<SlabDma<S>, SlabDma<O>>::value && S::NSTAGE == O::NSTAGE, "S and O chain through one ring");
    // Chaining (see "Chaining" above run_slabs_big) on the 256-row tile only: there the fp4 x fp4 ring has two stages, as the hand-over needs; the
    // 128-row tiles (launches that cannot fill the chip) keep every segment's own prologue.
    // And with fp4 weights only (the production mode): the matching-precision 256-row kernel sits at its 128-VGPR limit and
    // spills with the second set of descriptors.
    static constexpr bool CHAIN = (MM_CHAIN && W4 && BM == 256 && !SMALL && MM_FP4_KD256 && N256::NSTAGE == 2 && S::STAGE <= N256::STAGE &&
                                   S::NSTAGE * S::STAGE <= LDS_BUDGET);
    // per-wave transpose regions of the epilogue (reuse the stages); the fused gate / up epilogue adds its scale atoms and code images
    static constexpr int EPILOGUE = (NT / 64) * 32 * 320 + ((WM == 4 && TN == 4) ? 1024 + (NT / 64) * 2048 : 0);
    static constexpr int cmax(int x, int y) { return x > y ? x : y; }
    static constexpr int TOTAL = cmax(cmax(cmax(N256::BYTES, N128::BYTES), cmax(S::BYTES, O::BYTES)), EPILOGUE);
    static_assert(TOTAL <= LDS_BUDGET, "LDS budget");
};
template <bool W4> struct Lds { static constexpr int TOTAL = Segs<W4>::TOTAL; };

// segment Q over its 128-deep K units [first, first + count) WITHOUT chaining (split-K ranges, the 128-row and 64-row tiles):
// `pre` runs once, before the first wait (see run_slabs)
template <bool W4, int Q, class PRE>
__device__ __forceinline__ void run_segment(Acc &acc, const GemmArgs &a, int nslab128, int first, int count, int m0, int n0, uint8_t *smem,
                                            PRE pre) {
    using SG = Segs<W4>;
    const typename SG::DmaSO none{};   // never read: CH = false
    if constexpr (Q == 0) {
#if MM_FP4_KD256 && MM_WM >= 2     // (the 32-row tiles' two loader waves cannot carry the four scale pieces of a 256-deep slab)
        const int n2 = count >> 1;
        if (n2) run_slabs<typename SG::N256, false>(acc, a, 0, nslab128, first, n2, m0, n0, smem, pre, 0, 0, none, 0);
        if (count & 1) {
            if (n2) {
                barrier_lds_only();   // every wave is past its last read of the 256-deep stages before they are refilled
                run_slabs<typename SG::N128, false>(acc, a, 0, nslab128, first + 2 * n2, 1, m0, n0, smem, [] {}, 0, 0, none, 0);
            } else {
                run_slabs<typename SG::N128, false>(acc, a, 0, nslab128, first, 1, m0, n0, smem, pre, 0, 0, none, 0);
            }
        }
#else
        run_slabs<typename SG::N128, false>(acc, a, 0, nslab128, first, count, m0, n0, smem, pre, 0, 0, none, 0);
#endif
    } else if constexpr (Q == 1) {
        run_slabs<typename SG::S, false>(acc, a, 1, nslab128, first, count, m0, n0, smem, pre, 0, 0, none, 0);
    } else {
        run_slabs<typename SG::O, false>(acc, a, 2, nslab128, first, count, m0, n0, smem, pre, 0, 0, none, 0);
    }
}

// The three segments of one tile in a row, chained where the geometry allows (Segs::CHAIN, see "Chaining" above run_slabs_big): the fp4 segment hands
// over to the first 128-deep segment that exists, S hands over to O.  `round_acc` = the rounding between two segments.
// TAIL: the O segment (n2s >= 2, the launcher's rule) ends with the tile-major tail, which writes the output (run_tail).
template <bool W4, bool TAIL, class RND>
__device__ __forceinline__ void run_all_segments(Acc &acc, const GemmArgs &a, int n0s, int n1s, int n2s, int m0, int n0, uint8_t *smem,
                                                 RND round_acc) {
    using SG = Segs<W4>;
    using DmaSO = typename SG::DmaSO;
    static_assert(!TAIL || SG::CHAIN, "the tail is built into the chained segment sequence of the 256-row tile");
    auto nothing = [] {};
    if constexpr (!SG::CHAIN) {
        if (n0s) run_segment<W4, 0>(acc, a, n0s, 0, n0s, m0, n0, smem, nothing);
        if (n1s) {
            if (n0s) {
                barrier_lds_only();  // the previous segment's last LDS reads are done before the stages are refilled
                run_segment<W4, 1>(acc, a, n1s, 0, n1s, m0, n0, smem, round_acc);
            } else {
                run_segment<W4, 1>(acc, a, n1s, 0, n1s, m0, n0, smem, nothing);
            }
        }
        if (n2s) {
            if (n0s | n1s) {
                barrier_lds_only();
                run_segment<W4, 2>(acc, a, n2s, 0, n2s, m0, n0, smem, round_acc);
            } else {
                run_segment<W4, 2>(acc, a, n2s, 0, n2s, m0, n0, smem, nothing);
            }
        }
    } else {
        const int wave = __builtin_amdgcn_readfirstlane(mm_tid() >> 6);
        constexpr int NSO = SG::S::NSTAGE;
        // the successor of the fp4 segment: S if it exists, else O; the fp4 segment hands over only when it is a whole number
        // of 256-deep slabs, at least two
        const int qn = n1s ? 1 : 2, cn = n1s ? n1s : n2s;
        const bool chain_n = n0s >= 4 && !(n0s & 1) && cn > 0;
        DmaSO dn, d2;   // descriptors of the fp4 segment's successor and of the O segment (harmless when those do not exist)
        dn.init(a, qn, m0, n0, cn, 0, wave, n1s ? Op<SG::S::XEL, 128>::G128 : Op<SG::O::XEL, 128>::G128,
                n1s ? Op<SG::S::WEL, 128>::G128 : Op<SG::O::WEL, 128>::G128);
        const bool chain_s = n1s > 0 && n2s > 0;
        d2.init(a, 2, m0, n0, n2s, 0, wave, Op<SG::O::XEL, 128>::G128, Op<SG::O::WEL, 128>::G128);
        int pref = 0, cur = 0;      // state handed from a segment to its successor
        bool any = false;           // a segment has run: the next one rounds the accumulators first
        auto pre = [&] {
            if (any) round_acc();
        };
        if (n0s) {
            if (chain_n) {
                const int n2 = n0s >> 1;
                pref = cn < NSO ? cn : NSO;
                run_slabs<typename SG::N256, true>(acc, a, 0, n0s, 0, n2, m0, n0, smem, nothing, 0, n2 & 1, dn, pref);
            } else {
                run_segment<W4, 0>(acc, a, n0s, 0, n0s, m0, n0, smem, nothing);
            }
            any = true;
        }
        if (n1s) {
            if (any && pref == 0) barrier_lds_only();  // unchained: the previous segment's last LDS reads are done before the refill
            const int pout = chain_s ? (n2s < NSO ? n2s : NSO) : 0;
            cur = run_slabs<typename SG::S, true>(acc, a, 1, n1s, 0, n1s, m0, n0, smem, pre, pref, 0, d2, pout);
            pref = pout;
            any = true;
        }
        if (n2s) {
            if (any && pref == 0) barrier_lds_only();
            run_slabs<typename SG::O, true, DmaSO, decltype(pre), TAIL>(acc, a, 2, n2s, 0, n2s, m0, n0, smem, pre, pref, pref ? cur : 0, d2, 0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Ping-pong K loop (the PP kernel: 256 x 256 tile, fp4 weights, bf16 output, a launch that is ONE fp8 x fp4 segment of >= 2 slabs,
// nothing chained in; the launcher's rule, g256_pingpong).  In run_slabs_big all eight waves run their MFMAs, reach the barrier and
// wait for their post-barrier fragment reads at the same time, so every SIMD's matrix pipe runs dry around each rendezvous (19 % of
// the loop with no DMA at all, profiles/r06_delivery.txt).  Here the two waves of a SIMD (w and w + 4) take turns:
//   G0 = waves 0-3, G1 = waves 4-7.  The loop is a chain of PERIODS, each ending in one workgroup barrier; in every period one
//   group is in its COMPUTE phase (the 16 MFMAs of one slab, both K steps, back to back from a fragment set already in registers)
//   and the other in its MEMORY phase (the ds_reads of its next slab's fragments and scales into that same set, and its own DMA
//   pieces of the slab two ahead).  G1 runs exactly one period behind G0.  Slab s lives in stage s % 3:
//     period 2s:     G0 memory(s)   G1 compute(s - 1)      G0 requests its pieces of slab s + 2 into stage (s + 2) % 3
//     period 2s + 1: G0 compute(s)  G1 memory(s)           G1 requests its pieces of slab s + 2
//   Stage (s + 2) % 3 held slab s - 1, last read by G1 in period 2s - 1 (lgkmcnt(0) in front of that barrier).  Slab s + 1 must be
//   complete before G0 reads it in period 2s + 2: both groups certify it with a counted vmcnt in front of the barrier that ends
//   period 2s + 1 -- G0 at the end of compute(s) (its pieces of s + 1 went out in period 2s - 2), G1 at the end of memory(s), right
//   after issuing its pieces of s + 2 (its pieces of s + 1 went out in period 2s - 1).  The scale pieces are issued by waves 0 and 1,
//   both in G0, so G1's count has no scale piece in it.  Never vmcnt(0) inside the loop.
// Every accumulator still receives its K steps slab by slab, step 0 before step 1: the sums are bit for bit those of run_slabs_big.
// The head (round 18, profiles/r18_head.txt).  One tile per CU and one round of tiles per launch: nothing overlaps what a workgroup does
// before its first MFMA, so that is kept to the requests and their latency.
//   - The accumulators are never zeroed (128 v_accvgpr_write per wave, two waves per SIMD, used to stand in front of the first request).
//     The first K step of every accumulator -- slab 0, step 0: the first eight MFMAs of each group's first compute phase, peeled out of
//     the loop (compute<Z0>), or of the tail when count = 2 (run_tail<Z0>) -- takes the inline constant 0 as srcC and only writes the
//     accumulator.  0 + x in the matrix pipe is what accumulating onto a zeroed register gives: the outputs keep their bits.
//   - After the tile mapping a wave builds its DMA descriptors and issues its slab-0 pieces; the fragment offsets, gx / gw and the
//     PingPong object follow behind that issue.  (The tail's bias loads stay in run_tail: they are vector-memory loads and would enter
//     the vmcnt accounting of the loop.)
//   - Slab 1 is requested behind the HEAD BARRIER, which every wave reaches when the memory pipe has taken its slab-0 pieces.  The pipe
//     serves in issue order across waves (one 1 KiB piece per ~31 cycles), so without that barrier a wave that is ahead puts its slab-1
//     pieces in front of the other waves' slab-0 pieces and the slab-0 certificate waits for up to 100 pieces instead of about 50.
//     vmcnt accounting of the prologue: slab 0 (NPIECES or NPIECES - 1 per wave), head barrier, slab 1 (the same count), then
//     wait_slabs<1> = at most one slab's worth outstanding = this wave's slab-0 pieces have landed, then the certificate barrier.
// Barriers (P = count - 2 ping-pong slabs): the prologue's two (head barrier, slab-0 certificate), then per group P memory + P compute
// phases and ONE extra period -- G1's first (period 0, it has no compute(-1)), G0's last (period 2P, G1 computes slab count - 3 while
// G0 only waits) -- both only when P > 0: 2 + 2P + (P > 0) barriers per wave in each group, then run_tail's own.  count = 2: no
// ping-pong period; count = 3: one slab, periods 0-2.  After the last one the state is exactly what run_tail documents: slab count - 2
// complete in its stage (certified at the end of period 2P - 1, or by the prologue when P = 0), slab count - 1 requested, the stage of
// slab count - 3 free.  -DMM_PP_HEAD_BARRIER=0 (A/B builds): slab 1 right behind the moved set-up, no head barrier.
// MM_PP_CPIECES = c (0-2): the first c DMA pieces of a wave's share of a slab go out in its compute phase, one after every second
// MFMA, instead of in its memory phase.  MM_PP_FLIP = 1: the computing wave of a SIMD at priority 1 (set and reset at the compute
// phase's edges) instead of the static priority 1 of waves 4-7 (tile_body).
// Register hazard: a memory phase overwrites the srcA / srcB fragment registers that the same wave's MFMAs read in the previous
// period.  The gfx950 hazard table has a write-after-read entry for an MFMA's srcC only (the accumulators: AGPRs that no ds_read
// writes), none for srcA / srcB, which the MFMA reads at issue; and a barrier lies between the last MFMA and the first such read,
// which goes to step 0's fragments, read by MFMAs eight MFMAs earlier still.  (run_slabs_big overwrites set 0 after a barrier in the
// same way.)
// ---------------------------------------------------------------------------------------------------------
#ifndef MM_PP_CPIECES
#define MM_PP_CPIECES 0
#endif
#ifndef MM_PP_FLIP
#define MM_PP_FLIP 0
#endif
#ifndef MM_PP_HEAD_BARRIER
#define MM_PP_HEAD_BARRIER 1
#endif
template <class G>
struct PingPong {
    using D = SlabDma<G>;
    static constexpr int XEL = G::XEL, WEL = G::WEL, KD = G::KD, CP = MM_PP_CPIECES;
    static_assert(G::KSTEPS == 2 && G::NSTAGE == 3 && TM == 2 && TN == 4, "the ping-pong loop is written for the 256 x 256 tile on a three-stage 128-deep ring");
    static_assert(D::SFW <= 4, "the scale pieces are issued by waves of G0 only (G1's vmcnt counts none)");
    static_assert(CP >= 0 && CP <= 2 && CP < D::XP, "compute-phase pieces are activation pieces");
    using XF = typename Frag<XEL>::type;
    using WF = typename Frag<WEL>::type;
    const D &dma;
    const FragOfsOf<G, XEL> &fx;
    const FragOfsOf<G, WEL> &fw;
    int gx, gw, li, kb;
    XF x[2][TM];        // one slab's fragments, both K steps: 32 + 32 VGPRs (run_slabs_big's x0 / x1 / w0 / w1)
    WF w[2][TN];
    Scales<KD> sc;

    template <int H>
    __device__ __forceinline__ void read_step(const uint8_t *st) {
#pragma unroll
        for (int t = 0; t < TM; ++t) x[H][t] = load_frag<XEL, KD, H>(st, fx, t);
#pragma unroll
        for (int t = 0; t < TN; ++t) w[H][t] = load_frag<WEL, KD, H>(st + G::OFF_W, fw, t);
    }
    template <int P = CP>
    __device__ __forceinline__ void mem_pieces(int slab, uint8_t *stage) const {
        if constexpr (P < D::NPIECES) {
            dma.template piece<P>(slab, stage);
            mem_pieces<P + 1>(slab, stage);
        }
    }
    // memory phase: slab `st`'s fragments and scales (step 0 first), then this wave's memory-phase pieces of slab `ahead`
    __device__ __forceinline__ void memory(const uint8_t *st, int ahead, uint8_t *st_ahead) {
        read_step<0>(st);
        read_step<1>(st);
        load_scales<G>(sc, st, gx, gw, li, kb);
        mem_pieces(ahead, st_ahead);
        // the scale shifts stay in this phase, behind the DMA issue (hipcc would sink them behind the barrier, to the head of the
        // compute phase)
        MM_DEVICE_ONLY(asm volatile("" : "+v"(sc.x[0][0]), "+v"(sc.x[0][1]), "+v"(sc.w[0][0]), "+v"(sc.w[0][1]), "+v"(sc.w[0][2]),
                                    "+v"(sc.w[0][3]));)
    }
    // compute phase: MFMA I = K step I >> 3 on tile I & 7 (run_slabs_big's order), compute-phase piece J after MFMA 2J + 1
    // Z0: the group's first compute phase (slab 0).  Nothing has written the accumulators: the eight MFMAs of K step 0 take the
    // constant 0 as srcC (mfma_tile's ZC).
    template <bool Z0 = false, int I = 0>
    __device__ __forceinline__ void compute(int ahead, uint8_t *st_ahead) const {
        if constexpr (I < 16) {
            constexpr int H = I >> 3, P = I & 7, tn = P / TM, tm = P % TM;
            mfma_tile<tn * TM + tm, XEL, WEL, H, false, Z0 && H == 0>(x[H][tm], w[H][tn], sc.x[0][tm], sc.w[0][tn]);
            if constexpr ((I & 1) && (I >> 1) < CP) dma.template piece<(I >> 1)>(ahead, st_ahead);
            compute<Z0, I + 1>(ahead, st_ahead);
        }
    }
};

// head stamps of the instrumented build (s_memtime, raw): this wave's first DMA request and its first MFMA; tile_body stores them
struct HeadStamps {
    unsigned long long dma = 0, mfma = 0;
};
template <class G>
__device__ __forceinline__ void run_pingpong(const GemmArgs &a, int count, int m0, int n0, uint8_t *smem, [[maybe_unused]] HeadStamps &hs) {
    using D = SlabDma<G>;
    const int lane = mm_tid() & 63, wave = __builtin_amdgcn_readfirstlane(mm_tid() >> 6);
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, kb = lane >> 5;
    const bool g1 = wave >= NT / 128;     // wave-uniform: waves 4-7
    D dma;
    init_slab_dma<G>(dma, a, 2, m0, n0, count, 0, wave);
    auto stage_at = [&](int i) { return smem + i * G::STAGE; };
    // Head (round 18): the requests for slab 0 are the first thing a wave does -- the accumulators are never zeroed (compute<Z0>,
    // run_tail<Z0>), and everything that does not go into a DMA instruction is worked out behind their issue, under their latency.
#if MM_CLOCKS
    hs.dma = __builtin_amdgcn_s_memtime();
#endif
    dma.all(0, stage_at(0));
    // (the asm keeps hipcc from hoisting the set-up below, which hangs on li_, above the DMA issue)
    int li_ = li;
    MM_DEVICE_ONLY(asm volatile("" : "+v"(li_));)
    FragOfsOf<G, G::XEL> fx;
    FragOfsOf<G, G::WEL> fw;
    fx.init(wm * (TM * 32) + li_, kb);
    fw.init(wn * (TN * 32) + li_, kb);
    const int gx = ((m0 & 127) >> 5) + wm * TM, gw = ((n0 & 127) >> 5) + wn * TN;
    PingPong<G> pp{dma, fx, fw, gx, gw, li, kb};
#if MM_PP_FLIP && MM_PRIO
    MM_DEVICE_ONLY(asm volatile("s_setprio 0");)   // (tile_body gave waves 4-7 the static priority)
#endif
    // Slab 1 goes out only when EVERY wave has handed its slab-0 pieces to the memory pipe, which serves them in issue order: the
    // head barrier.  Without it a wave that is ahead (waves 4-7 win every issue arbitration) queues its slab-1 pieces in front of the
    // other waves' slab-0 pieces, and the slab-0 certificate below waits for up to 100 pieces instead of about 50.
#if MM_PP_HEAD_BARRIER
    barrier_lds_only();
#endif
    dma.all(1, stage_at(1));
    wait_slabs<1>(dma);                             // this wave's slab-0 pieces have landed; its slab-1 pieces may stay in flight
    barrier_lds_only();
    const int P = count - 2;
    // one ping-pong slab of a group: memory(s), barrier, compute(s), barrier.  Z0: the group's first (s = 0), peeled out of the loop
    // so that the loop's MFMAs all accumulate
    auto slab = [&](auto z0, int s, int st) {
        const int sa = st == 0 ? 2 : st - 1;        // stage of slab s + 2 (= that of slab s - 1)
        pp.memory(stage_at(st), s + 2, stage_at(sa));
        // G1: its pieces of slab s + 1 have landed; those of s + 2 (memory phase, issued just now) may stay in flight
        if (g1) wait_vmcnt<D::NPIECES - 1 - PingPong<G>::CP>();
        barrier_lds_only();
#if MM_PP_FLIP
        MM_DEVICE_ONLY(asm volatile("s_setprio 1");)
#endif
#if MM_CLOCKS
        if constexpr (decltype(z0)::value) hs.mfma = __builtin_amdgcn_s_memtime();
#endif
        pp.template compute<decltype(z0)::value>(s + 2, stage_at(sa));
#if MM_PP_FLIP
        MM_DEVICE_ONLY(asm volatile("s_setprio 0");)
#endif
        // G0: its pieces of slab s + 1 have landed; all of s + 2 may stay in flight
        if (!g1) wait_slabs<1>(dma);
        MM_DEVICE_ONLY(__builtin_amdgcn_sched_barrier(0);)   // the MFMAs are issued before the wave waits at the barrier
        barrier_lds_only();
    };
    if (P == 0) {
        // stage 0 holds slab 0 (complete), stage 1 slab 1 (requested), stage 2 nothing; the tail writes the accumulators first
        Scales<G::KD> sca;
        load_scales<G>(sca, stage_at(0), gx, gw, li, kb);
        run_tail<G, true>(a, m0, n0, smem, 0, 1, 2, sca, fx, fw, gx, gw);
        return;
    }
    if (g1) barrier_lds_only();                    // period 0: G1 has no compute(-1)
    slab(std::true_type{}, 0, 0);
    int st = 1;                                     // stage of slab s
    for (int s = 1; s < P; ++s) {
        slab(std::false_type{}, s, st);
        st = st == 2 ? 0 : st + 1;
    }
    if (!g1) barrier_lds_only();                   // period 2P: G1 computes slab count - 3, G0 waits
    // stage st holds slab count - 2 (complete), the next one count - 1 (requested), the third count - 3 (free)
    const int c1 = st == 2 ? 0 : st + 1, cf = c1 == 2 ? 0 : c1 + 1;
    Scales<G::KD> sca;
    load_scales<G>(sca, stage_at(st), gx, gw, li, kb);
    run_tail<G>(a, m0, n0, smem, st, c1, cf, sca, fx, fw, gx, gw);
}

// ---------------------------------------------------------------------------------------------------------
// Epilogue of one tile: the accumulators (AGPRs a[0 : NACC-1] of the 8-wave tiles, `acc` of the 4-wave tiles) as bf16 (+ bias)
// to D.  Every wave of the caller is past its last read of the operand stages (LDS is reused for the transposes).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void write_tile(const GemmArgs &a, Acc &acc, const int m0, const int n0, uint8_t *smem) {
    // ---- epilogue: bf16 (+bias) -> LDS [32 tokens][TN*32 features] per wave -> 16-byte row-contiguous stores ----
    // The accumulator has the feature on the lane and four consecutive tokens in registers 4g..4g+3.  Per register pair:
    // v_cvt_pk_bf16_f32 packs the two TOKENS of this lane's feature, one quad-permute DPP fetches the neighbour lane's pair
    // and one v_perm_b32 (selector by lane parity) turns the 2 x 2 block into the two FEATURES (li & ~1, +1) of ONE token:
    // 4 instructions per two values, then one 4-byte LDS write.  (The first version transposed 4 x 4 blocks with two DPP rounds
    // and eleven selects per four values; the epilogue was VALU-bound at ~3.3 us.)
    // LDS image: row pitch 320 B = 80 dwords = 16 mod 32 banks, so the two rows (lane parity) that a 32-lane half writes per
    // ds_write_b32 fall on disjoint banks; the row reads below give every 16-lane service group of ds_read_b128 one whole
    // 256-byte row (all 64 banks once).  Both were 2-way conflicted before (the 528 k SQ_LDS_BANK_CONFLICT cycles of the round-1
    // profile = 2 k cycles per CU, all of them in this epilogue; the main loop's fragment reads are conflict-free).
    const int lane = mm_tid() & 63, wave = mm_tid() >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, hi = lane >> 5;
#if MM_SMALL
#define MM_ACC_GET(T_, I_) acc.t[T_][I_]
#else
#define MM_ACC_GET(T_, I_) acc_read<16 * (T_) + (I_)>()
#endif
    if (a.out_f32) {
        // MM_OUT_F32 (tensor-parallel partial sums): the fp32 accumulators as they are.  The lane holds feature li of tokens
        // 8g + 4hi + i: a wave instruction writes two rows of 32 consecutive floats (128-byte segments), no transpose needed.
        float *D32 = reinterpret_cast<float *>(a.D);
#define MM_F32_TILE(TM_, TN_)                                                                              \
        {                                                                                                  \
            float v[16];                                                                                   \
            v[0] = MM_ACC_GET(TN_ * TM + TM_, 0);   v[1] = MM_ACC_GET(TN_ * TM + TM_, 1);                  \
            v[2] = MM_ACC_GET(TN_ * TM + TM_, 2);   v[3] = MM_ACC_GET(TN_ * TM + TM_, 3);                  \
            v[4] = MM_ACC_GET(TN_ * TM + TM_, 4);   v[5] = MM_ACC_GET(TN_ * TM + TM_, 5);                  \
            v[6] = MM_ACC_GET(TN_ * TM + TM_, 6);   v[7] = MM_ACC_GET(TN_ * TM + TM_, 7);                  \
            v[8] = MM_ACC_GET(TN_ * TM + TM_, 8);   v[9] = MM_ACC_GET(TN_ * TM + TM_, 9);                  \
            v[10] = MM_ACC_GET(TN_ * TM + TM_, 10); v[11] = MM_ACC_GET(TN_ * TM + TM_, 11);                \
            v[12] = MM_ACC_GET(TN_ * TM + TM_, 12); v[13] = MM_ACC_GET(TN_ * TM + TM_, 13);                \
            v[14] = MM_ACC_GET(TN_ * TM + TM_, 14); v[15] = MM_ACC_GET(TN_ * TM + TM_, 15);                \
            const int n = n0 + wn * (TN * 32) + TN_ * 32 + li;                                             \
            _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                               \
                /* register r = token 8 * (r / 4) + 4 * hi + r % 4 of the wave's 32-row block */           \
                const int m = m0 + wm * (TM * 32) + TM_ * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);            \
                if (n < a.N && m < a.M) D32[(size_t)m * a.N + n] = v[r];                                   \
            }                                                                                              \
        }
#if MM_TN == 4
#define MM_F32_ROW(TM_) MM_F32_TILE(TM_, 0) MM_F32_TILE(TM_, 1) MM_F32_TILE(TM_, 2) MM_F32_TILE(TM_, 3)
#elif MM_TN == 2
#define MM_F32_ROW(TM_) MM_F32_TILE(TM_, 0) MM_F32_TILE(TM_, 1)
#else
#define MM_F32_ROW(TM_) MM_F32_TILE(TM_, 0)
#endif
        MM_F32_ROW(0)
#if MM_TM >= 2
        MM_F32_ROW(1)
#endif
#if MM_TM == 4
        MM_F32_ROW(2)
        MM_F32_ROW(3)
#endif
#undef MM_F32_ROW
#undef MM_F32_TILE
        return;
    }
    constexpr int EP = 320;
    uint8_t *reg = smem + wave * (32 * EP);
    float bias[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int n = n0 + wn * (TN * 32) + tn * 32 + li;
        bias[tn] = (a.bias != nullptr && n < a.N) ? bf16_bits_to_f32(a.bias[n]) : 0.0f;
    }
    const bool vec_ok = (a.N & 7) == 0;
    [[maybe_unused]] const unsigned sel = (lane & 1) ? 0x03020706u : 0x05040100u;   // v_perm_b32 selector, see pair_to_token
    uint8_t *wr = reg + (4 * hi + (lane & 1)) * EP + (li & ~1) * 2;
    // service groups of ds_read_b128 (MI355X_MICROARCH.md, LDS): lanes {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same
    // + 32: group = bit (lane >> 2) of 0b10010110 (+ 2 for the upper half), position inside the group = 4 * (lane >> 3 & 3) + lane & 3
    const int rgrp = ((0x96 >> ((lane >> 2) & 7)) & 1) + 2 * hi, ridx = ((lane >> 3) & 3) * 4 + (lane & 3);
    auto store_rows = [&](int tm) {
        // wave-local hand-over: the same wave reads back what it wrote (LDS is in order per wave, no barrier needed)
        constexpr int RPI = 16 / TN;   // rows per wave instruction (256-, 128- or 64-byte rows)
#pragma unroll
        for (int j = 0; j < 32 / RPI; ++j) {
            // TN = 4: group g reads row 4j + g whole; TN = 2: group g reads rows 8j + (g & 1) + 4 (g >> 1) and that + 2
            // (two 128-byte rows whose first banks are 32 apart at this pitch); TN = 1: lane -> row 16j + lane / 4, plain
            const int rowl = TN == 4 ? 4 * j + rgrp : TN == 2 ? 8 * j + (rgrp & 1) + 4 * (rgrp >> 1) + 2 * (ridx >> 3) : 16 * j + (lane >> 2);
            const int ch = TN == 4 ? ridx : TN == 2 ? (ridx & 7) : (lane & 3);
            const uint4 v = *reinterpret_cast<const uint4 *>(reg + rowl * EP + ch * 16);
            const int m = m0 + wm * (TM * 32) + tm * 32 + rowl;
            const int n = n0 + wn * (TN * 32) + ch * 8;
            if (m < a.M) {
                uint16_t *dst = a.D + (size_t)m * a.N + n;
                if (vec_ok && n + 7 < a.N) {
                    // write-through store (sc0 sc1): the 32 MiB of D leave the XCD's L2 as they are written instead of staying
                    // dirty until the end of the kernel.  Nothing re-reads D through this L2 (the consumer is another kernel, on
                    // any XCD), and the flush of the dirty lines sat on the kernel boundary: kernel 50.7 -> 48.9 us, back-to-back
                    // step 51.7 -> 49.7 us at 4096^3 (plain / nt / sc1 / sc0 sc1 measured on one device: 50.6 / 49.9 / 49.2 / 49.0).
                    typedef unsigned v4u __attribute__((ext_vector_type(4)));
                    [[maybe_unused]] const v4u vv = {v.x, v.y, v.z, v.w};
                    MM_DEVICE_ONLY(asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(dst), "v"(vv) : "memory");)
                } else {
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (n + e < a.N) dst[e] = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
                }
            }
        }
    };
    // (v0, v1) = this lane's feature at tokens t, t + 1  ->  features (li & ~1, li | 1) at token t + (lane & 1), packed bf16.
    // With a bias: D = bf16(bf16(acc) + bias) as the reference's separate `y + bias` (qLinearLayer.py:70-71).
    auto pair_to_token = [&](float v0, float v1, float b) -> unsigned {
        unsigned out = 0;
        MM_DEVICE_ONLY(
            unsigned p;
            asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(p) : "v"(v0), "v"(v1));
            if (a.bias != nullptr) {
                const float r0 = __uint_as_float(p << 16) + b, r1 = __uint_as_float(p & 0xFFFF0000u) + b;
                asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(p) : "v"(r0), "v"(r1));
            }
            const unsigned other = (unsigned)__builtin_amdgcn_mov_dpp((int)p, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
            // even lane: (own.lo, other.lo) = features (f, f+1) at token t; odd lane: (other.hi, own.hi) = the same features at t + 1
            out = __builtin_amdgcn_perm(other, p, sel);)
        return out;
    };
#define MM_EPI_TILE(TM_, TN_)                                                                                      \
    {                                                                                                              \
        float v[16];                                                                                               \
        v[0] = MM_ACC_GET(TN_ * TM + TM_, 0);   v[1] = MM_ACC_GET(TN_ * TM + TM_, 1);              \
        v[2] = MM_ACC_GET(TN_ * TM + TM_, 2);   v[3] = MM_ACC_GET(TN_ * TM + TM_, 3);              \
        v[4] = MM_ACC_GET(TN_ * TM + TM_, 4);   v[5] = MM_ACC_GET(TN_ * TM + TM_, 5);              \
        v[6] = MM_ACC_GET(TN_ * TM + TM_, 6);   v[7] = MM_ACC_GET(TN_ * TM + TM_, 7);              \
        v[8] = MM_ACC_GET(TN_ * TM + TM_, 8);   v[9] = MM_ACC_GET(TN_ * TM + TM_, 9);              \
        v[10] = MM_ACC_GET(TN_ * TM + TM_, 10); v[11] = MM_ACC_GET(TN_ * TM + TM_, 11);            \
        v[12] = MM_ACC_GET(TN_ * TM + TM_, 12); v[13] = MM_ACC_GET(TN_ * TM + TM_, 13);            \
        v[14] = MM_ACC_GET(TN_ * TM + TM_, 14); v[15] = MM_ACC_GET(TN_ * TM + TM_, 15);            \
        _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                            \
            /* registers 4g..4g+3 = tokens 8g + 4hi + 0..3 of the wave's 32-row block */                           \
            *reinterpret_cast<unsigned *>(wr + (8 * g) * EP + TN_ * 64) = pair_to_token(v[4 * g], v[4 * g + 1], bias[TN_]);         \
            *reinterpret_cast<unsigned *>(wr + (8 * g + 2) * EP + TN_ * 64) = pair_to_token(v[4 * g + 2], v[4 * g + 3], bias[TN_]); \
        }                                                                                                          \
    }
#if MM_TN == 4
#define MM_EPI_ROW(TM_)                                                                                            \
    MM_EPI_TILE(TM_, 0) MM_EPI_TILE(TM_, 1) MM_EPI_TILE(TM_, 2) MM_EPI_TILE(TM_, 3)                                \
    store_rows(TM_);
#elif MM_TN == 2
#define MM_EPI_ROW(TM_)                                                                                            \
    MM_EPI_TILE(TM_, 0) MM_EPI_TILE(TM_, 1)                                                                        \
    store_rows(TM_);
#else
#define MM_EPI_ROW(TM_)                                                                                            \
    MM_EPI_TILE(TM_, 0)                                                                                            \
    store_rows(TM_);
#endif
    MM_EPI_ROW(0)
#if MM_TM >= 2
    MM_EPI_ROW(1)
#endif
#if MM_TM == 4
    MM_EPI_ROW(2)
    MM_EPI_ROW(3)
#endif
#undef MM_EPI_ROW
#undef MM_EPI_TILE
#undef MM_ACC_GET
}

// ---------------------------------------------------------------------------------------------------------
// Fused gate / up epilogue (256-feature tiles of the 8-wave kernels; GemmArgs::act, mm_gate_up_activate).
// The reference computes h = act_fn(gate_proj(x)) * up_proj(x) through HBM and quantizes h for down_proj (model/qLlamaLayer.py:377-387;
// its fused activate_quantize_x, mgemm/src/activate.cu:44-202, bindings.cpp:307-334, reads gate and up back from HBM).  Here the
// weight rows of gate_proj and up_proj are interleaved per 128 features when they are packed, so the tile at n0 holds gate features
// [f0, f0 + 128) in its waves wn = 0 and the up features of the same indices in its waves wn = 1, f0 = n0 / 2: the tile has
// everything that 128 columns of h need.  Per 32-row slice of every wave row:
//   A. every wave rounds its accumulators to bf16 exactly as write_tile does (the bits mm_matmul would have written) and puts them
//      into its [32 rows][128 features] LDS image; 16-byte chunk c of a 64-byte group sits at c ^ (row & 3), see B;
//   B. after a barrier thread (wave w, lane l) takes row 16 w + l / 4 of the slice's 128 rows and 32-feature group l % 4: it reads
//      its 32 gate and 32 up values from the images of waves (w / 2, 0) and (w / 2, 1) -- conflict-free: a ds_read_b128 service
//      group holds four rows with four different row & 3 -- evaluates silu(gate) * up in fp32 and quantizes the group with the code
//      of activate_quantize_x (mx_direct_convert.h: same bytes).  fp4 codes (16 bytes per lane, a lane quad = 64 contiguous bytes
//      of a row) leave from the lanes; fp6 / fp8 codes go through a wave-private code image and leave 16 bytes per lane side by
//      side (whole 96- / 128-byte row pieces), write-through;
//   C. the four scale bytes of a lane quad are merged (DPP) and collected in LDS as the two complete 512-byte SF atoms of the
//      tile's rows for this 128-column slab of the consumer's K axis; one wave writes them out, 16 bytes per lane.
// The consumer's segments are multiples of 128 columns, so a tile's 128 features lie in ONE of them: format and destination are
// workgroup-uniform.  No bias (gate_proj / up_proj have none in the models of BASELINE.json).
// ---------------------------------------------------------------------------------------------------------
// BF16H (the MoE experts, mx_gemm256_moe_act_kernel): h is the bf16 value bf16(bf16(silu(gate)) * up) (silu_mul_bf16) and its groups are
// quantized by the reorder quantizer's arithmetic on bf16 pairs (finish_group, mx_group_convert.h) -- the bytes of
// mm_moe_activate_quantize, whose reorder index the packed weight's row order has taken in.
#if MM_WM == 4 && MM_TN == 4
template <bool BF16H = false>
__device__ __forceinline__ void write_tile_act(const GemmArgs &a, const int m0, const int n0, uint8_t *smem) {
    constexpr int EP = 320;
    constexpr int IMG = (NT / 64) * 32 * EP;            // the eight bf16 images
    constexpr int SFST = IMG;                           // [2 atoms][512] scale bytes; then the per-wave code images of 16 rows x 128 bytes
    constexpr int CODES_AT = IMG + 1024;
    static_assert(IMG + 1024 + (NT / 64) * 2048 <= LDS_BUDGET, "LDS of the fused gate / up epilogue");
    const int lane = mm_tid() & 63, wave = mm_tid() >> 6;
    const int li = lane & 31, hi = lane >> 5;
    uint8_t *reg = smem + wave * (32 * EP);
    // the tile's 128 intermediate features inside the consumer's K split
    const int f0 = (n0 >> 8) << 7;
    const int KN = a.act_K[0], KS = a.act_K[1];
    const int seg = __builtin_amdgcn_readfirstlane(f0 < KN ? 0 : (f0 < KN + KS ? 1 : 2));
    const int fo = f0 - (seg == 0 ? 0 : seg == 1 ? KN : KN + KS);        // first feature inside the segment: a multiple of 128
    // (BF16H: `a` is the expert's own copy of the argument block, in registers -- selects, since an index that is not a constant would
    // send the whole block to scratch.    // Every value goes through readfirstlane (they are uniform) before the select: a select between loads from the block would be
    // folded back into one load at a computed address.)
    int kseg;
    if constexpr (BF16H)
        kseg = seg == 0 ? __builtin_amdgcn_readfirstlane(KN) : (seg == 1 ? __builtin_amdgcn_readfirstlane(KS) : __builtin_amdgcn_readfirstlane(a.act_K[2]));
    else kseg = a.act_K[seg];
    [[maybe_unused]] const unsigned sel = (lane & 1) ? 0x03020706u : 0x05040100u;   // as write_tile
    // A: this lane writes rows 8 g + 4 hi + (lane & 1) and that + 2: row & 3 = (lane & 1) and (lane & 1) + 2
    const int col = (li & 6) << 1, ch = li >> 3;
    uint8_t *wr0 = reg + (4 * hi + (lane & 1)) * EP + ((ch ^ (lane & 1)) << 4) + col;
    uint8_t *wr2 = reg + (4 * hi + (lane & 1)) * EP + ((ch ^ (lane & 1) ^ 2) << 4) + col;
    auto pair_to_token = [&](float v0, float v1) -> unsigned {
        unsigned out = 0;
        MM_DEVICE_ONLY(
            unsigned p;
            asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(p) : "v"(v0), "v"(v1));
            const unsigned other = (unsigned)__builtin_amdgcn_mov_dpp((int)p, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
            out = __builtin_amdgcn_perm(other, p, sel);)
        return out;
    };
    // B: this thread's row of the slice and its group
    const int q = lane >> 2, g = lane & 3;
    const int rr = 16 * (wave & 1) + q;                                  // row inside the producing waves' 32-row images
    const uint8_t *gate = smem + (wave & ~1) * (32 * EP) + rr * EP + g * 64, *up = gate + 32 * EP;
    const int sw = rr & 3;
    uint8_t *codes = smem + CODES_AT + wave * 2048;
    uint8_t *sfst = smem + SFST;
    auto quantize_slice = [&](int tm) {
        const int row_t = (wave >> 1) * (TM * 32) + tm * 32 + rr;        // row inside the tile
        const int m = m0 + row_t;
        uint32_t byte;
        if constexpr (BF16H) {
            uint32_t hv[16], amax = 0;     // hv[i] = {element 2 i, element 2 i + 1} as bf16 bits; amax: the larger magnitude bits of either half
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float x[8], b[8];
                unpack8(*reinterpret_cast<const uint4 *>(gate + ((c ^ sw) << 4)), x);
                unpack8(*reinterpret_cast<const uint4 *>(up + ((c ^ sw) << 4)), b);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t lo16 = silu_mul_bf16(x[2 * k], b[2 * k]), hi16 = silu_mul_bf16(x[2 * k + 1], b[2 * k + 1]);
                    hv[4 * c + k] = lo16 | (hi16 << 16);
                    const uint32_t ml = lo16 & 0x7FFFu, mh = hi16 & 0x7FFFu;
                    amax = amax > ml ? amax : ml;
                    amax = amax > mh ? amax : mh;
                }
            }
            if (seg == 0) {
                uint8_t *dst = a.act_o[0] + (size_t)m * (size_t)(kseg >> 1) + (fo >> 1) + g * 16;
                if (m < a.M) byte = finish_group<EL_FP4, true>(hv, amax, dst);
                else byte = 127u;
            } else if (seg == 1) {
                byte = finish_group<EL_FP6>(hv, amax, codes + q * 96 + g * 24);
            } else {
                byte = finish_group<EL_FP8>(hv, amax, codes + q * 128 + g * 32);
            }
        } else {
        float v[32];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float x[8], b[8];
            unpack8(*reinterpret_cast<const uint4 *>(gate + ((c ^ sw) << 4)), x);
            unpack8(*reinterpret_cast<const uint4 *>(up + ((c ^ sw) << 4)), b);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[8 * c + e] = silu_mul(x[e], b[e]);
        }
        if (seg == 0) {
            // (rows past M: the store is skipped, the group is still quantized -- its scale byte goes into the atom's padding)
            uint8_t *dst = a.act_o[0] + (size_t)m * (size_t)(kseg >> 1) + (fo >> 1) + g * 16;
            if (m < a.M) byte = quantize32<EL_FP4>(v, dst);
            else byte = 127u;
        } else if (seg == 1) {
            byte = quantize32<EL_FP6>(v, codes + q * 96 + g * 24);
        } else {
            byte = quantize32<EL_FP8>(v, codes + q * 128 + g * 32);
        }
        }
        // C: the quad's four scale bytes -> one dword of the row's SF entry (layout: mx_common.h sf_offset)
        const uint32_t b1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0x55, 0xF, 0xF, false);
        const uint32_t b2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0xAA, 0xF, 0xF, false);
        const uint32_t b3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)byte, 0xFF, 0xF, 0xF, false);
        if (g == 0)
            *reinterpret_cast<uint32_t *>(sfst + (row_t >> 7) * 512 + (row_t & 31) * 16 + ((row_t >> 5) & 3) * 4) =
                byte | (b1 << 8) | (b2 << 16) | (b3 << 24);
        if (seg != 0) {
            __builtin_amdgcn_wave_barrier();   // one wave: its LDS instructions complete in order
            const int mw = m0 + (wave >> 1) * (TM * 32) + tm * 32 + 16 * (wave & 1);     // first row of this wave's 16
            if (seg == 2) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int t = lane + 64 * i, r = t >> 3, c = t & 7;
                    const uint4 cv = *reinterpret_cast<const uint4 *>(codes + r * 128 + c * 16);
                    if (mw + r < a.M) store16<true>(a.act_o[2] + (size_t)(mw + r) * (size_t)kseg + fo + c * 16, cv.x, cv.y, cv.z, cv.w);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int t = lane + 64 * i, r = t / 6, c = t - 6 * r;
                    if (t < 96) {
                        const uint4 cv = *reinterpret_cast<const uint4 *>(codes + r * 96 + c * 16);
                        if (mw + r < a.M)
                            store16<true>(a.act_o[1] + (size_t)(mw + r) * (size_t)(kseg / 4 * 3) + (fo / 4 * 3) + c * 16, cv.x, cv.y, cv.z, cv.w);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();   // the code image is read before the next slice overwrites it
        }
    };
#define MM_ACT_TILE(TM_, TN_)                                                                                       \
    {                                                                                                               \
        float v[16];                                                                                                \
        v[0] = acc_read<16 * (TN_ * TM + TM_) + 0>();   v[1] = acc_read<16 * (TN_ * TM + TM_) + 1>();               \
        v[2] = acc_read<16 * (TN_ * TM + TM_) + 2>();   v[3] = acc_read<16 * (TN_ * TM + TM_) + 3>();               \
        v[4] = acc_read<16 * (TN_ * TM + TM_) + 4>();   v[5] = acc_read<16 * (TN_ * TM + TM_) + 5>();               \
        v[6] = acc_read<16 * (TN_ * TM + TM_) + 6>();   v[7] = acc_read<16 * (TN_ * TM + TM_) + 7>();               \
        v[8] = acc_read<16 * (TN_ * TM + TM_) + 8>();   v[9] = acc_read<16 * (TN_ * TM + TM_) + 9>();               \
        v[10] = acc_read<16 * (TN_ * TM + TM_) + 10>(); v[11] = acc_read<16 * (TN_ * TM + TM_) + 11>();             \
        v[12] = acc_read<16 * (TN_ * TM + TM_) + 12>(); v[13] = acc_read<16 * (TN_ * TM + TM_) + 13>();             \
        v[14] = acc_read<16 * (TN_ * TM + TM_) + 14>(); v[15] = acc_read<16 * (TN_ * TM + TM_) + 15>();             \
        _Pragma("unroll") for (int gq = 0; gq < 4; ++gq) {                                                          \
            *reinterpret_cast<unsigned *>(wr0 + (8 * gq) * EP + TN_ * 64) = pair_to_token(v[4 * gq], v[4 * gq + 1]);            \
            *reinterpret_cast<unsigned *>(wr2 + (8 * gq + 2) * EP + TN_ * 64) = pair_to_token(v[4 * gq + 2], v[4 * gq + 3]);    \
        }                                                                                                           \
    }
#define MM_ACT_SLICE(TM_)                                                                                           \
    MM_ACT_TILE(TM_, 0) MM_ACT_TILE(TM_, 1) MM_ACT_TILE(TM_, 2) MM_ACT_TILE(TM_, 3)                                 \
    barrier_lds_only();                        /* the slice's eight images are complete */                          \
    quantize_slice(TM_);
    MM_ACT_SLICE(0)
#if MM_TM == 2
    barrier_lds_only();                        // every thread is past its reads of slice 0's images
    MM_ACT_SLICE(1)
#endif
#undef MM_ACT_SLICE
#undef MM_ACT_TILE
    barrier_lds_only();                        // the SF atoms are complete (LDS-only barriers: a persistent launch has the next tile's DMAs in flight here)
    if (wave == 0) {
        const int atom = lane >> 5;
        if (atom * 128 < BM && m0 + atom * 128 < a.M) {
            const uint4 sv = *reinterpret_cast<const uint4 *>(sfst + lane * 16);
            uint8_t *act_sf;
            if constexpr (BF16H) {
                auto uniform = [](uint8_t *p) {
                    const unsigned long long v = (unsigned long long)p;
                    const unsigned lo32 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi32 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
                    return (uint8_t *)(((unsigned long long)hi32 << 32) | lo32);
                };
                uint8_t *const sf0 = uniform(a.act_sf[0]), *const sf1 = uniform(a.act_sf[1]), *const sf2 = uniform(a.act_sf[2]);
                act_sf = seg == 0 ? sf0 : (seg == 1 ? sf1 : sf2);
            }
            else act_sf = a.act_sf[seg];
            uint8_t *dst = act_sf + ((size_t)((m0 >> 7) + atom) * (size_t)(kseg >> 7) + (size_t)(fo >> 7)) * 512u + (lane & 31) * 16;
            store16<true>(dst, sv.x, sv.y, sv.z, sv.w);
        }
    }
}
#endif

// ---------------------------------------------------------------------------------------------------------
// Split-K with the reduction INSIDE the launch (4-wave tiles: launches of a few dozen tiles, 64 < M <= ~512).
// Workgroup bid = tile * splits + q runs slabs [first, first + count) of ONE segment (the launcher's plan in a.split_first, as for
// the two-launch split-K of the 128-row tiles), writes its fp32 accumulators to a.ws (write-through stores), and takes a ticket
// of the tile.  The workgroup that draws the LAST ticket adds the partial sums of all splits IN SPLIT ORDER (so the result does
// not depend on which one it is), applies the rounding chain D = bf16(N); D = bf16(S + D); D = bf16(O + D) and writes the tile.
// No second launch, no spinning: nothing waits for another workgroup.
// Ticket = one 32-bit counter per tile at the head of the workspace.  The counters must be ZERO when the launch starts and are zero
// again when it ends (the last workgroup of a tile puts its counter back): the caller clears them once, when it creates the
// workspace, and says so with MM_WS_TICKETS_ZEROED (micromix_hip.h); without that flag this path is not taken.
// Visibility across the eight L2s (not coherent with each other for plain accesses): the partial sums leave by device-scope
// (sc1, write-through) stores, every wave waits for its stores before the workgroup's barrier, then one lane performs the
// device-scope atomic; the reader fetches them with device-scope loads.  (Putting a tile's splits on one XCD -- workgroups go to
// the XCDs round-robin -- and using plain accesses was tried: wrong results on this pool, and no faster.)
// ---------------------------------------------------------------------------------------------------------
// Slab range of split q inside segment sg (128-deep K units relative to the segment).  The launcher cuts the K axis N | S | O into
// a.splits ranges of equal length (a.split_cut[q] .. a.split_cut[q + 1], in 128-deep units from the start of N; a split may span two
// or three segments and then leaves one partial sum per segment it touches).  The same function serves the producers and the
// reducing workgroup.
__device__ __forceinline__ void split_range(const GemmArgs &a, int q, int sg, int &lo, int &hi) {
    const int n0s = a.K[0] >> 7, n1s = a.K[1] >> 7, n2s = a.K[2] >> 7;
    const int off = sg == 0 ? 0 : sg == 1 ? n0s : n0s + n1s, len = sg == 0 ? n0s : sg == 1 ? n1s : n2s;
    const int g0 = a.split_cut[q], g1 = a.split_cut[q + 1];
    lo = __builtin_amdgcn_readfirstlane((g0 > off ? g0 : off) - off);
    hi = __builtin_amdgcn_readfirstlane((g1 < off + len ? g1 : off + len) - off);
}

template <bool W4>
__device__ __forceinline__ void split_tile_reduce(const GemmArgs &a, const int bid, Acc &acc, uint8_t *smem) {
#if MM_SMALL
    constexpr int NF = TM * TN;                 // MFMA tiles per wave = 16-float groups per lane
    constexpr int CHUNKS = 4 * NF;              // 16-byte chunks per lane
    constexpr int PART_BYTES = CHUNKS * NT * 16;
    const int tiles_n = (a.N + BN - 1) / BN;
    const int q = bid % a.splits, tile = bid / a.splits;
    const int m0 = __builtin_amdgcn_readfirstlane((tile / tiles_n) * BM);
    const int n0 = __builtin_amdgcn_readfirstlane((tile % tiles_n) * BN);
#if MM_CLOCKS
    // per workgroup (100 MHz ticks): [0] start (absolute), [1] slabs done, [2] partial sums acknowledged, [3] ticket drawn;
    // the reducing workgroup adds 1 << 40 to [3] and stores [4] = partial sums read, [5] = tile written (8 words per workgroup)
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long *ck = a.clock_out != nullptr ? a.clock_out + 8 * (size_t)bid : nullptr;
#endif
    // ---- this split's slab range, segment by segment: one partial-sum slot per (split, segment) ----
    // slots of a tile: split q's first partial sum at a.split_slot[q], one more per further segment it touches (<= splits + 2 in all)
    const int nslots = a.split_slot[a.splits];
    const uint8_t *ws_tile = reinterpret_cast<const uint8_t *>(a.ws) + (size_t)tile * nslots * PART_BYTES;
    const __amdgpu_buffer_rsrc_t rs = make_brsrc(ws_tile, (unsigned)nslots * (unsigned)PART_BYTES);
    constexpr int AUX_SC = MM_SPLIT_AUX;     // cache policy of the partial-sum stores and loads (see below)
    const int tofs = (int)(mm_tid() & (NT - 1)) * 16;
    bool any = false;
    int slot = a.split_slot[q];
    auto piece = [&](auto SG) {
        constexpr int sg = decltype(SG)::value;
        int lo, hi;
        split_range(a, q, sg, lo, hi);
        if (hi <= lo) return;
        if (any) barrier_lds_only();       // every wave is past the previous piece's LDS reads before the stages are refilled
        any = true;
#pragma unroll
        for (int t = 0; t < NF; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc.t[t][i] = 0.0f;
        run_segment<W4, sg>(acc, a, a.K[sg] >> 7, lo, hi - lo, m0, n0, smem, [] {});
        if (mm_tid() < NT) {
            // chunk c of thread t at (c * NT + t) * 16: whole lines per wave instruction
            const int soff = __builtin_amdgcn_readfirstlane(slot * PART_BYTES);
#pragma unroll
            for (int t = 0; t < NF; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const v4i v = {__float_as_int(acc.t[t][4 * g]), __float_as_int(acc.t[t][4 * g + 1]),
                                     __float_as_int(acc.t[t][4 * g + 2]), __float_as_int(acc.t[t][4 * g + 3])};
                    __builtin_amdgcn_raw_buffer_store_b128(v, rs, tofs + (4 * t + g) * (NT * 16), soff, AUX_SC);
                }
        }
        ++slot;
    };
    piece(std::integral_constant<int, 0>{});
    piece(std::integral_constant<int, 1>{});
    piece(std::integral_constant<int, 2>{});
#if MM_CLOCKS
    if (ck != nullptr && mm_tid() == 0) { ck[0] = r0; ck[1] = __builtin_amdgcn_s_memrealtime() - r0; }
#endif
    // Release side of the hand-over, at the ISA level (MM_SPLIT_FENCES = 0, the default):
    //   1. the partial sums leave by `buffer_store_dwordx4 ... sc1` (MM_SPLIT_AUX): device-scope write-through stores, which this
    //      XCD's L2 passes on to memory instead of keeping them dirty;
    //   2. `s_waitcnt vmcnt(0)`: the wave does not go on until every one of those stores has been ACKNOWLEDGED, and a write-through
    //      store is acknowledged from the memory side of the L2;
    //   3. the workgroup barrier: that holds for every wave of the workgroup;
    //   4. only then ONE lane performs the agent-scope atomic add on the tile's ticket (executed at the device coherence point).
    // So every partial sum of this workgroup is in memory before its ticket can be observed.  Acquire side: the workgroup that
    // draws the last ticket does so after the atomics of all others (the counter says so), its loads are issued after the atomic has
    // RETURNED (the flag travels through LDS behind a barrier) and are device-scope (sc1) loads, which are not served from a line this
    // XCD's L2 might still hold.  MM_SPLIT_FENCES = 1 spells the same thing with __builtin_amdgcn_fence(release / acquire,
    // "agent") and an acq_rel ticket; its buffer_wbl2 / buffer_inv cost 7 us per launch of ~9 (mx_gemm256.hip), and there is nothing
    // for them to write back or invalidate.  What the scheme cannot survive is a launch that dies between a ticket and its reset:
    // mm_matmul_ws_reset re-arms the workspace (tests/test_matmul_gpu.py::test_poisoned_ticket_and_ws_reset).
#if MM_SPLIT_FENCES
    MM_DEVICE_ONLY(__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");)
#else
    MM_DEVICE_ONLY(asm volatile("s_waitcnt vmcnt(0)" ::: "memory");)   // this wave's partial sums have left
#endif
    __syncthreads();                       // ... every wave's; and every wave is done with the operand stages
    if (mm_tid() >= NT) return;         // the loader waves have no accumulators
    unsigned *flag = reinterpret_cast<unsigned *>(smem);
#if MM_CLOCKS
    if (ck != nullptr && mm_tid() == 0) ck[2] = __builtin_amdgcn_s_memrealtime() - r0;
#endif
    if (mm_tid() == 0) {
        // one fetch-add per workgroup (a compare-and-swap loop serialises its retries: ~2 us per contender, measured)
        unsigned *tk = a.tickets + tile;
        const unsigned old = __hip_atomic_fetch_add(tk, 1u, MM_SPLIT_FENCES ? __ATOMIC_ACQ_REL : __ATOMIC_RELAXED, MM_SPLIT_SCOPE);
        const bool last = old + 1u == (unsigned)a.splits;
        if (last) __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, MM_SPLIT_SCOPE);   // the tickets are zero again when the launch ends
        *flag = last ? 1u : 0u;
#if MM_CLOCKS
        if (ck != nullptr) ck[3] = (__builtin_amdgcn_s_memrealtime() - r0) + (last ? (1ull << 40) : 0ull);
#endif
    }
    __syncthreads();                       // (the compute waves: the loaders have left)
    const unsigned is_last = *flag;
    __syncthreads();                       // the flag word lies in the LDS range the epilogue reuses
    if (is_last == 0u) return;
    // Acquire side: the last ticket was drawn after every other split's release (above); the reader's loads below are device-scope
    // (sc1) loads behind an agent-scope acquire fence (buffer_inv sc1), so they cannot be served from a stale line of this XCD's L2.
#if MM_SPLIT_FENCES
    MM_DEVICE_ONLY(__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");)
#endif
    // ---- last arrival: the tile's slots in order = split order inside a segment, segments in order N, S, O (the K ranges of
    // the splits are consecutive, so slot order IS that order; a.slot_seg holds each slot's segment, two bits each).  Sum in that
    // order, with the rounding chain at every change of segment.  The loads of B slots are in flight at once: one round trip to
    // memory (~2.5 us: the partial sums were written through to HBM) per batch, not per slot. ----
    constexpr int B = NF == 1 ? 8 : 2;
    float run[NF][16], sum[NF][16];
#pragma unroll
    for (int t = 0; t < NF; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) run[t][i] = sum[t][i] = 0.0f;
    // the segment whose partial sums are in `sum` is complete: D = bf16(sum + D) (reference chain) or D = sum + D (fused)
    auto fold = [&] {
#pragma unroll
        for (int t = 0; t < NF; ++t)
#pragma unroll
            for (int i = 0; i < 16; i += 2) {
                const float t0 = sum[t][i] + run[t][i], t1 = sum[t][i + 1] + run[t][i + 1];
                sum[t][i] = sum[t][i + 1] = 0.0f;
                if (a.round_per_segment) {
                    unsigned pk = 0;
                    MM_DEVICE_ONLY(asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(pk) : "v"(t0), "v"(t1));)
                    run[t][i] = __uint_as_float(pk << 16);
                    run[t][i + 1] = __uint_as_float(pk & 0xFFFF0000u);
                } else {
                    run[t][i] = t0;
                    run[t][i + 1] = t1;
                }
            }
    };
    int cur_seg = (int)(a.slot_seg & 3ull);
    for (int sb = 0; sb < nslots; sb += B) {
        v4i v[B][CHUNKS];
#pragma unroll
        for (int b = 0; b < B; ++b)
            if (sb + b < nslots) {
                const int soff = __builtin_amdgcn_readfirstlane((sb + b) * PART_BYTES);
#pragma unroll
                for (int c = 0; c < CHUNKS; ++c) v[b][c] = __builtin_amdgcn_raw_buffer_load_b128(rs, tofs + c * (NT * 16), soff, AUX_SC);
            }
#pragma unroll
        for (int b = 0; b < B; ++b)
            if (sb + b < nslots) {
                const int sg = (int)((a.slot_seg >> (2 * (sb + b))) & 3ull);
                if (sg != cur_seg) {
                    fold();
                    cur_seg = sg;
                }
#pragma unroll
                for (int c = 0; c < CHUNKS; ++c)
#pragma unroll
                    for (int e = 0; e < 4; ++e) sum[c >> 2][4 * (c & 3) + e] += __int_as_float(v[b][c][e]);
            }
    }
    fold();
#pragma unroll
    for (int t = 0; t < NF; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc.t[t][i] = run[t][i];
#if MM_CLOCKS
    if (ck != nullptr && mm_tid() == 0) ck[4] = __builtin_amdgcn_s_memrealtime() - r0;
#endif
    write_tile(a, acc, m0, n0, smem);
#if MM_CLOCKS
    if (ck != nullptr && mm_tid() == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ck[5] = __builtin_amdgcn_s_memrealtime() - r0;
    }
#endif
#endif
}

// SPLITK: workgroup blockIdx.x = tile * a.splits + q runs slabs [first, first + count) of ONE segment (the plan in
// a.split_first, see launch_mx_gemm256) and leaves its raw fp32 accumulators in a.ws; splitk_reduce_kernel adds the
// partial sums in a fixed order and applies the rounding chain.  With q = blockIdx.x % splits the workgroups of one XCD
// (blockIdx.x % 8) all walk the same K range when splits is a multiple of 8, so each L2 holds one K slice of X and W.
// `bid` = index of this workgroup among the workgroups of problem `a` (its block index, or the block index minus the first block
// of the group in a grouped launch)
// TAIL: the tile-major tail writes the output under the last slabs' MFMAs (run_tail; bf16 output, the launcher's rule)
// PP: the launch is one fp8 x fp4 segment of >= 2 slabs (K[0] = K[1] = 0), walked by the ping-pong loop (run_pingpong) into the tail
// BF16H: the fused gate / up epilogue in the MoE experts' bits (write_tile_act)
template <bool W4, bool SPLITK, bool ACT = false, bool TAIL = false, bool PP = false, bool BF16H = false>
__device__ __forceinline__ void tile_body(const GemmArgs &a, const int bid) {
    static_assert(!TAIL || (!SPLITK && !ACT), "the tail replaces the plain bf16 epilogue only");
    static_assert(!PP || (W4 && TAIL), "the ping-pong loop hands over to the tile-major tail");
    extern __shared__ __attribute__((aligned(128))) uint8_t smem[];   // 128: FragOfsC relies on it
    Acc acc;   // empty for the 8-wave tiles (their accumulators are the AGPRs a[0 : NACC-1])

    const int tiles_m = (a.M + BM - 1) / BM, tiles_n = a.n_tiles ? a.n_tiles : (a.N + BN - 1) / BN;
    const int n0s = a.K[0] >> 7, n1s = a.K[1] >> 7, n2s = a.K[2] >> 7;
    if constexpr (SPLITK && SMALL) {
        split_tile_reduce<W4>(a, bid, acc, smem);
        return;
    } else if constexpr (SPLITK) {
        const int q = bid % a.splits, tile = bid / a.splits;
        const int m0 = __builtin_amdgcn_readfirstlane((tile / tiles_n) * BM);
        const int n0 = __builtin_amdgcn_readfirstlane((tile % tiles_n) * BN);
        const int seg = (q >= a.split_first[1]) + (q >= a.split_first[2]);
        const int j = q - a.split_first[seg], parts = a.split_first[seg + 1] - a.split_first[seg];
        const int ns = a.K[seg] >> 7;
        const int first = __builtin_amdgcn_readfirstlane(ns * j / parts);
        const int count = __builtin_amdgcn_readfirstlane(ns * (j + 1) / parts - first);
        AccLoop<0, NACC>::zero();
        if (seg == 0) run_segment<W4, 0>(acc, a, ns, first, count, m0, n0, smem, [] {});
        else if (seg == 1) run_segment<W4, 1>(acc, a, ns, first, count, m0, n0, smem, [] {});
        else run_segment<W4, 2>(acc, a, ns, first, count, m0, n0, smem, [] {});
        acc_settle();
        AccLoop<0, NACC>::store(a.ws + (size_t)bid * (NACC * NT) + 4 * mm_tid());
        return;
    }

#if MM_PRIO && MM_WM == 4
    // Static priority for the second-dispatched half of the workgroup (MI355X_MICROARCH.md, "Two waves per SIMD", item 4): waves
    // w and w + 4 share a SIMD, the younger one loses every issue arbitration; one s_setprio for waves 4-7, never changed again.
    // Round 4, alternating processes on one box, us: headline 53.76 -> 52.5, (2048,128,1920) 47.8 -> 46.6, all-fp4 37.6 -> 37.1,
    // (3072,896,128) unchanged; priority 3 the same as 1 (profiles/notes_r04.md section 7).
    // (the test must be provably wave-uniform -- s_setprio ignores EXEC: through readfirstlane it becomes a scalar branch)
    if (__builtin_amdgcn_readfirstlane(mm_tid()) >= 256) { MM_DEVICE_ONLY(asm volatile("s_setprio %0" ::"n"(MM_PRIO));) }
#endif
    // (the loader / compute tiles: priority 1 for the loader waves, or for the compute waves, changed nothing -- notes_r04.md section 7)
    // ---- tile mapping: blocks that share an XCD (blockIdx % 8) get a contiguous chunk of a grouped order ----
    const int ntiles = tiles_m * tiles_n;
    auto map_tile = [&](int id, int &m0_, int &n0_) {
        {
            const int q = ntiles >> 3, r = ntiles & 7, xcd = id & 7, j = id >> 3;
            id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
        }
#ifdef MM_GH
        constexpr int GH = MM_GH;   // developer probe (tools/delivery_probes.sh): other shapes of the XCD's chunk of the tile order
#else
        constexpr int GH = 4;  // tiles of a group share their weight panels; 4 x 8 tiles per XCD chunk at 16 x 16
#endif
        const int per_group = GH * tiles_n;
        const int grp = id / per_group;
        const int first_m = grp * GH;
        const int gh = (tiles_m - first_m) < GH ? (tiles_m - first_m) : GH;
        const int in = id - grp * per_group;
        m0_ = __builtin_amdgcn_readfirstlane((first_m + in % gh) * BM);
        n0_ = __builtin_amdgcn_readfirstlane((a.n_tile0 + in / gh) * BN);
    };
    // Between two segments the reference rounds D through bf16 (gemm.cu:75-77: each segment is its own kernel).  Here the
    // accumulators are rounded in place, AFTER the next segment's first DMAs have been issued (run_slabs' `pre` hook): the
    // rounding is ~1 us of VALU work that needs neither LDS nor the matrix pipe, the DMAs need ~1-2 us to land.
    auto round_acc = [&] {
        if (a.round_per_segment) {
#if MM_SMALL
            // two values per v_cvt_pk_bf16_f32 (RNE, a NaN stays a NaN), as AccLoop::round_bf16 does on the AGPR accumulators
#pragma unroll
            for (int t = 0; t < TM * TN; ++t)
#pragma unroll
                for (int i = 0; i < 16; i += 2) {
                    unsigned pk = 0;
                    MM_DEVICE_ONLY(asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(pk) : "v"(acc.t[t][i]), "v"(acc.t[t][i + 1]));)
                    acc.t[t][i] = __uint_as_float(pk << 16);
                    acc.t[t][i + 1] = __uint_as_float(pk & 0xFFFF0000u);
                }
#else
            acc_settle();
            AccLoop<0, NACC>::round_bf16();
#endif
        }
    };
    // exactly one tile per workgroup; the epilogue's LDS staging starts at offset 0 (the operand stages are free by then)
    {
        int m0, n0;
        map_tile(bid, m0, n0);
#if MM_CLOCKS
        unsigned long long t0 = 0, r0 = 0;
        const bool stamp = a.clock_out != nullptr;
        if (stamp) {
            t0 = __builtin_amdgcn_s_memtime();
            r0 = __builtin_amdgcn_s_memrealtime();
        }
#endif
#if MM_SMALL
#pragma unroll
        for (int t = 0; t < TM * TN; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc.t[t][i] = 0.0f;
#else
        // (the ping-pong kernel never zeroes: the first K step of every accumulator writes it, run_pingpong)
        if constexpr (!PP) AccLoop<0, NACC>::zero();
#endif
        // ablation 4096: every workgroup loads tile (0, 0)'s operands (all of L2's misses disappear, the L2 -> LDS traffic stays);
        // ablation 8192: every workgroup of an XCD loads the operands of the XCD's first tile
#if (MM_DBG & 4096)
        const int lm0 = 0, ln0 = 0;
#elif (MM_DBG & 8192)
        const int lm0 = __builtin_amdgcn_readfirstlane((bid & 7) * BM), ln0 = __builtin_amdgcn_readfirstlane((bid & 7) * BN);
#else
        const int lm0 = m0, ln0 = n0;
#endif
        [[maybe_unused]] HeadStamps hs;
        if constexpr (PP) run_pingpong<typename Segs<W4>::O>(a, n2s, lm0, ln0, smem, hs);
        else run_all_segments<W4, TAIL>(acc, a, n0s, n1s, n2s, lm0, ln0, smem, round_acc);
        if constexpr (TAIL) {
#if MM_CLOCKS
            // run_tail stamped its loop end (the last MFMA) as raw counters; its stores are the last it issued
            if (stamp && mm_tid() == 0) {
                a.clock_out[4 * bid] -= t0;
                a.clock_out[4 * bid + 1] -= r0;
                a.clock_out[4 * bid + 2] = r0;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores have left
                a.clock_out[4 * bid + 3] = __builtin_amdgcn_s_memrealtime() - r0;
                // the ping-pong kernel's head: shader cycles from the start stamp to wave 0's first DMA request and to its first
                // MFMA, in row MM_HEAD_ROW0 + bid of the buffer (a launch of more workgroups than that leaves them out)
                if (PP && bid < MM_HEAD_ROW0) {
                    a.clock_out[4 * (MM_HEAD_ROW0 + bid)] = hs.dma - t0;
                    a.clock_out[4 * (MM_HEAD_ROW0 + bid) + 1] = hs.mfma > t0 ? hs.mfma - t0 : 0;
                }
            }
#endif
            return;
        }
        __syncthreads();  // every wave is done with the operand stages: LDS is reused for the transpose (no DMA is in flight here)
        if constexpr (SMALL) {
            if (mm_tid() >= NT) return;   // the loader waves have no accumulators
        } else {
            acc_settle();
        }
#if MM_CLOCKS
        if (stamp && mm_tid() == 0) {
            a.clock_out[4 * bid] = __builtin_amdgcn_s_memtime() - t0;
            a.clock_out[4 * bid + 1] = __builtin_amdgcn_s_memrealtime() - r0;
            a.clock_out[4 * bid + 2] = r0;  // absolute start (100 MHz ticks)
        }
#endif
#if MM_WM == 4 && MM_TN == 4
        if constexpr (ACT) write_tile_act<BF16H>(a, m0, n0, smem);
        else
#endif
            write_tile(a, acc, m0, n0, smem);
#if MM_CLOCKS
        if (stamp && mm_tid() == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores have left
            a.clock_out[4 * bid + 3] = __builtin_amdgcn_s_memrealtime() - r0;
        }
#endif
    }
}

template <bool W4, bool SPLITK>
__global__ void __launch_bounds__(NTHREADS) mx_gemm256_kernel(GemmArgs a) {
    tile_body<W4, SPLITK>(a, blockIdx.x);
}
#if MM_WM == 4 && MM_TM == 2
// fp4 weights, no split-K, bf16 output, at least two slabs in the O segment: the tile-major tail (run_tail).  An overload with a
// third parameter: mx_gemm256_kernel<true, false, true>, while the two-parameter kernels keep their names.
template <bool W4, bool SPLITK, bool TAIL>
__global__ void __launch_bounds__(NTHREADS) mx_gemm256_kernel(GemmArgs a) {
    static_assert(W4 && !SPLITK && TAIL, "the tail kernel exists for fp4 weights without split-K");
    tile_body<W4, SPLITK, false, TAIL>(a, blockIdx.x);
}
// ... and, when the launch is one fp8 x fp4 segment (K[0] = K[1] = 0), the ping-pong K loop in front of the tail (run_pingpong):
// mx_gemm256_kernel<true, false, true, true>
template <bool W4, bool SPLITK, bool TAIL, bool PP>
__global__ void __launch_bounds__(NTHREADS) mx_gemm256_kernel(GemmArgs a) {
    static_assert(W4 && !SPLITK && TAIL && PP, "the ping-pong kernel exists for fp4 weights without split-K, with the tail");
    tile_body<W4, SPLITK, false, TAIL, PP>(a, blockIdx.x);
}
#endif
#if MM_WM == 4 && MM_TN == 4
// fp4 weights, no split-K, the fused gate / up epilogue (write_tile_act)
__global__ void __launch_bounds__(NTHREADS) mx_gemm256_act_kernel(GemmArgs a) {
    tile_body<true, false, true>(a, blockIdx.x);
}
#endif

// Grouped launch (MoE experts with more than 64 token rows each, SURVEY.md section 8f rank 4): the workgroups of up to
// MM_MAX_GROUPS problems that share N, the K split and the weight mode in one grid; first_block[] is the prefix sum of their
// tile counts.
template <bool W4>
__global__ void __launch_bounds__(NTHREADS) mx_gemm256_grouped_kernel(GroupedTileArgs ga) {
    int g = 0;
#pragma unroll
    for (int i = 1; i < MM_MAX_GROUPS; ++i) g += (i < ga.ngroups && (int)blockIdx.x >= ga.first_block[i]) ? 1 : 0;
    tile_body<W4, false>(ga.g[g], (int)blockIdx.x - ga.first_block[g]);
}

// Device-sized grouped launch (mm_moe_matmul): the groups are the experts with 65 .. max_rows rows, their tile counts are worked out
// from the offsets by every workgroup (a scalar walk over <= 64 experts), and the grid is a host bound on the sum; a workgroup past
// the real total leaves before it touches memory.  The expert's argument block: moe_group_args.
template <bool W4>
__global__ void __launch_bounds__(NTHREADS) mx_gemm256_moe_kernel(GemmArgs a, MoeGroups mg) {
    const int tiles_n = (a.N + BN - 1) / BN;
    int bid = blockIdx.x, e = 0, lo = 0, M = 0;
    for (; e < mg.E; ++e) {
        lo = mg.offsets[e];
        M = mg.offsets[e + 1] - lo;
        const int t = (lo >= 0 && M > 64 && M <= mg.max_rows && M <= mg.n - lo) ? ((M + BM - 1) / BM) * tiles_n : 0;
        if (bid < t) break;
        bid -= t;
    }
    if (e >= mg.E) return;
    moe_group_args(a, mg, e, lo, M);
    tile_body<W4, false>(a, bid);
}

#if MM_WM == 4 && MM_TN == 4
// mm_moe_gate_up_activate: the walk of mx_gemm256_moe_kernel, but EVERY expert of 1 .. max_rows rows gets row tiles (one of at most 64
// rows runs on this tile with its missing rows masked, as write_tile_act masks the rows past a.M), the weight is the expert's packed
// w1 | w3 (fp4, N = 2 I rows in w2's reordered feature order, interleaved per 128) and the epilogue is write_tile_act in the MoE block's
// bits.  A workgroup past the real total, or one whose expert's offsets are negative, decreasing or past n, leaves before it touches memory.
__global__ void __launch_bounds__(NTHREADS) mx_gemm256_moe_act_kernel(GemmArgs a, MoeGroups mg) {
    const int tiles_n = (a.N + BN - 1) / BN;
    int bid = blockIdx.x, e = 0, lo = 0, M = 0;
    for (; e < mg.E; ++e) {
        lo = mg.offsets[e];
        M = mg.offsets[e + 1] - lo;
        const int t = (lo >= 0 && M >= 1 && M <= mg.max_rows && M <= mg.n - lo) ? ((M + BM - 1) / BM) * tiles_n : 0;
        if (bid < t) break;
        bid -= t;
    }
    if (e >= mg.E) return;
    moe_group_args<true>(a, mg, e, lo, M);
    tile_body<true, false, true, false, false, true>(a, bid);
}
#endif

}  // namespace MM_NS
#undef MM_SMALL
