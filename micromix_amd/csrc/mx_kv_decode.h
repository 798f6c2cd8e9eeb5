// What the decode walks over the 128-wide paged cache share between their translation units (kv_cache.hip: the four walks and the chunk
// merge; decode_step.hip: the walk that also appends the step's token): the argument blocks, the tile constants and the kinds of walk that
// kv_decode_tiles.inc is written for.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mx_kernels.h"

namespace mm {
namespace kv {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int DEC_WAVES = 4;
constexpr int TILE = 32;           // tokens per wave iteration

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
//   WALK_STEP    WALK_ALL with the A operand taken from the including kernel's registers (step_q: decode_step.hip rotates q itself)
// A member index outside [0, B) is a row without a query and without an output; a bad first member makes the slab's walk empty.
enum { WALK_ALL = 0, WALK_WINDOW = 1, WALK_PREFIX = 2, WALK_SUFFIX = 3, WALK_STEP = 4 };

}  // namespace kv

// the launch that combines the a.nc > 1 chunk partials of every (sequence, query head) into a.o (kv_cache.hip)
hipError_t launch_paged_decode_merge(const kv::DecodeArgs &a, hipStream_t stream);

}  // namespace mm
