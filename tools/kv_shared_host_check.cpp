// Stand-alone check of the host side of mm_paged_decode_shared (micromix_amd/csrc/mx_kv_shared_host.h: the size rules, the two splits,
// the workspace size and the workspace rules) over the edge values of its arguments, meant to run under the host sanitizers on a
// machine without a GPU -- it makes no HIP call:
//   hipcc --offload-arch=gfx950 -std=c++20 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/kv_shared_host_check.cpp micromix_amd/csrc/kv_cache.hip -o kv_shared_host_check && ./kv_shared_host_check
// (kv_cache.hip supplies mm::kv_chunks, the chunk arithmetic every split-KV launch shares.)  Exit status 0: every invariant held.
#include <limits.h>
#include <stdio.h>

#include "../micromix_amd/csrc/mx_kv_shared_host.h"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main() {
    const int bounds[] = {-1, 0, 1, 127, 128, 129, 255, 256, 257, 4096, 65535, 65536, (1 << 29) - 1, 1 << 29, (1 << 29) + 1, 1 << 30, INT_MAX};
    const int batches[] = {-1, 0, 1, 7, 64, 65535, 65536, INT_MAX};
    const int heads[][2] = {{1, 1}, {32, 8}, {16, 1}, {17, 1}, {6, 2}, {7, 2}, {0, 1}, {8, 0}, {-8, 8}, {INT_MAX, 1}, {INT_MAX, INT_MAX},
                            {65535 * 16, 65535}, {65536, 65536}};
    long long accepted = 0, refused = 0, overflowed = 0;
    for (int B : batches)
        for (const auto &h : heads)
            for (int a : bounds)
                for (int b : bounds) {
                    const int Hq = h[0], Hkv = h[1];
                    const int st = mm::kv_shared_sizes_status(B, Hq, Hkv, a, b);
                    const size_t bytes = mm::kv_shared_workspace_bytes(B, Hq, Hkv, a, b);
                    if (st != MM_OK || B <= 0) {
                        EXPECT(bytes == 0, "B %d Hq %d Hkv %d bounds %d %d: %zu bytes for sizes that are refused", B, Hq, Hkv, a, b, bytes);
                        EXPECT(st == MM_OK || st == MM_ERR_BAD_ARG || st == MM_ERR_UNSUPPORTED, "status %d", st);
                        if (st == MM_ERR_UNSUPPORTED) EXPECT(Hkv > 0 && Hq > 0 && Hq % Hkv == 0 && Hq / Hkv > 16, "Hq %d Hkv %d", Hq, Hkv);
                        ++refused;
                        continue;
                    }
                    const mm::KvSharedSplit s = mm::kv_shared_split(B, Hq, Hkv, a, b);
                    const int nc[2] = {s.ncA, s.ncB}, chunk[2] = {s.chunkA, s.chunkB}, bound[2] = {a, b};
                    for (int k = 0; k < 2; ++k) {
                        EXPECT(nc[k] >= 1 && chunk[k] >= 128 && chunk[k] % 128 == 0, "bound %d: %d chunks of %d", bound[k], nc[k], chunk[k]);
                        EXPECT((long long)nc[k] * chunk[k] >= bound[k], "bound %d: %d chunks of %d do not cover it", bound[k], nc[k], chunk[k]);
                        EXPECT((long long)(nc[k] - 1) * chunk[k] < (bound[k] > 0 ? bound[k] : 1), "bound %d: chunk %d of %d starts past it",
                               bound[k], nc[k] - 1, chunk[k]);
                        EXPECT(nc[k] <= (bound[k] + 255) / 256 + (bound[k] < 256), "bound %d: %d chunks are shorter than 256 tokens", bound[k], nc[k]);
                    }
                    const unsigned __int128 want = (unsigned __int128)B * Hq * (s.ncA + s.ncB) * 520;
                    if (want > SIZE_MAX) {
                        EXPECT(bytes == 0, "a size past SIZE_MAX gave %zu", bytes);
                        ++overflowed;
                    } else {
                        EXPECT(bytes == (size_t)want && bytes > 0, "B %d Hq %d Hkv %d bounds %d %d: %zu bytes", B, Hq, Hkv, a, b, bytes);
                        alignas(16) static char ws[64];
                        EXPECT(mm::kv_shared_workspace_status(ws, bytes, bytes) == MM_OK, "an exact workspace");
                        EXPECT(mm::kv_shared_workspace_status(ws, bytes - 1, bytes) == MM_ERR_BAD_ARG, "a workspace one byte short");
                        EXPECT(mm::kv_shared_workspace_status(ws + 8, bytes, bytes) == MM_ERR_BAD_ARG, "a misaligned workspace");
                        EXPECT(mm::kv_shared_workspace_status(nullptr, bytes, bytes) == MM_ERR_BAD_ARG, "no workspace");
                        ++accepted;
                    }
                }
    EXPECT(mm::kv_shared_workspace_status((void *)16, 0, 0) == MM_ERR_BAD_ARG, "a size of 0 is not a case of this call");
    printf("%lld size sets accepted, %lld refused, %lld past SIZE_MAX; %d failures\n", accepted, refused, overflowed, failures);
    return failures ? 1 : 0;
}
