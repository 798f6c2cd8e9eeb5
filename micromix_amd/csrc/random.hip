// Uniform numbers keyed by request seed and position (mm_uniform_rows, include/micromix_random.h, which states the rule): Philox4x32-10
// over counter (pos, sub, block, domain) and key = the seed's two halves.  No state, no atomic, no workspace: a lane computes one block
// of four words from what it reads and stores them.
//
// uniform_rows_kernel: one lane per (row, block), rows fastest: lane idx has r = idx % rows, j = idx / rows, so the 64 lanes of a wave
// hold 64 neighbouring rows of one block (but where a wave straddles the end of the rows) and each of the up to four stores of a lane,
// to the stream rows 4 j .. 4 j + 3, is one coalesced 256-byte store of the wave.  The ten rounds are twenty 32 x 32 -> 64 products:
// __umulhi and a 32-bit multiply each.  A row whose sequence is outside [0, batch) stores zeros.
#include "../../include/micromix_random.h"
#include "mx_kernels.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

constexpr int UR_THREADS = 256;
constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
static_assert(MM_UNIFORM_MAX_N % 4 == 0 && (long long)MM_UNIFORM_MAX_ROWS * (MM_UNIFORM_MAX_N / 4) < (1LL << 31) - UR_THREADS,
              "a lane index (row, block) fits an int, the grid's last workgroup included");

__global__ __launch_bounds__(UR_THREADS) void uniform_rows_kernel(const UniformRows s) {
    const int idx = blockIdx.x * UR_THREADS + threadIdx.x, blocks = (s.n + 3) >> 2;
    if (idx >= s.rows * blocks) return;
    const int j = idx / s.rows, r = idx - j * s.rows;
    const int q = s.row_seq ? s.row_seq[r] : r;
    const bool inside = q >= 0 && q < s.B;
    unsigned c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    if (inside) {
        const unsigned long long seed = (unsigned long long)s.seed[q];
        unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
        c0 = (unsigned)s.pos[r], c1 = s.sub ? (unsigned)s.sub[q] : 0u, c2 = (unsigned)j, c3 = s.domain;
#pragma unroll
        for (int round = 0; round < 10; ++round) {
            const unsigned hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0, hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
            c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
            k0 += PHILOX_W0, k1 += PHILOX_W1;                  // the bump after the last round is dead code
        }
    }
    const unsigned w[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int i = 4 * j + t;
        if (i < s.n) {
            const long long at = i * s.ld_out + r;             // r < rows <= ld_out, i < n: inside [n, ld_out]
            if (s.bits) s.bits[at] = w[t];
            if (s.out) s.out[at] = (float)(w[t] >> 8) * 0x1p-24f;          // a 24-bit integer times a power of two: exact
        }
    }
}

hipError_t launch_uniform_rows(const UniformRows &s, hipStream_t stream) {
    const int lanes = s.rows * ((s.n + 3) >> 2);
    uniform_rows_kernel<<<(lanes + UR_THREADS - 1) / UR_THREADS, UR_THREADS, 0, stream>>>(s);
    return hipGetLastError();
}

}  // namespace mm
