// The tile loop of the four decode walks (kv_cache.hip: WALK_ALL, WALK_WINDOW, WALK_PREFIX, WALK_SUFFIX), the body of each of its kernels.
// The including kernel provides: the constants KIND, GP and WALK, `a` (DecodeArgs) and `sh` (SharedArgs; read by the shared walks only).
// A textual include rather than a device function: the un-shared kernels then compile to the instructions they had before the shared
// walks existed, which an inlined function did not give (DESIGN 7i).
    __shared__ float s_p[DEC_WAVES][TILE][16];        // (p * scale) of the tile, [token][head]
    __shared__ float s_alpha[DEC_WAVES][16];
    __shared__ int64_t s_row[DEC_WAVES][TILE];        // V row of each token of the tile (-1: past the chunk)
    __shared__ float s_o[DEC_WAVES][GP][HD];
    __shared__ float s_ml[DEC_WAVES][GP][2];

    const int chunk = blockIdx.x, kvh = blockIdx.y;
    int b = blockIdx.z;                                // the sequence whose page list is walked
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, kq = l >> 4;
    const PagedKV &kv = a.kv;
    const int g = a.g;
    int t0, t1, cidx = chunk;                          // cidx: this walk's place among the partials of a (sequence, query head)
    int slab = 0, members = 1;                         // WALK_PREFIX: the slab is group_members[slab .. slab + members)
    if constexpr (WALK == WALK_PREFIX) {
        slab = blockIdx.z;
        const int j = find_seq(sh.group_indptr, kv.B, slab), per = 16 / g;
        const int lo = sh.group_indptr[j], hi = min(sh.group_indptr[j + 1], kv.B);
        if (slab < lo || slab >= hi || (slab - lo) % per) return;            // a dead slot (the whole workgroup)
        members = min(per, hi - slab);
        const int lead = sh.group_members[slab];
        const bool lead_ok = lead >= 0 && lead < kv.B;
        b = lead_ok ? lead : 0;
        const int end = lead_ok ? min(max(sh.shared_len[b], 0), seq_len(kv, b)) : 0;   // never past the length of the list that is read
        t0 = chunk * sh.chunkA;
        t1 = chunk == sh.ncA - 1 ? end : min(end, t0 + sh.chunkA);
    } else if constexpr (WALK == WALK_SUFFIX) {
        const int len = seq_len(kv, b), lo = min(max(sh.shared_len[b], 0), len);
        t0 = lo + min(chunk * sh.chunkB, len - lo);
        t1 = chunk == sh.ncB - 1 ? len : t0 + min(sh.chunkB, len - t0);
        cidx = sh.ncA + chunk;
    } else {
        const int len = seq_len(kv, b);
        t0 = (WALK == WALK_WINDOW ? window_begin(len - 1, a.window) : 0) + chunk * a.chunk;
        t1 = chunk == a.nc - 1 ? len : min(len, t0 + a.chunk);   // the last chunk runs to the end, whatever max_seq_len said
    }
    const int *pages = kv.indices + kv.indptr[b];

    // q as the MFMA A operand: lane (c, kq) holds head c (WALK_PREFIX: member c / g, head c % g), dims 32 kq + 8 s + j in step s
    v8bf qa[4];
    float qsum = 0.0f;
    {
        int qb = b, qh = c;
        bool live = false;                             // WALK_PREFIX: this lane's row has a query
        if constexpr (WALK == WALK_PREFIX) {
            const int mi = c / g;
            const int mb = mi < members ? sh.group_members[slab + mi] : -1;
            live = mb >= 0 && mb < kv.B;
            qb = live ? mb : 0;
            qh = c - mi * g;
        }
        const v4u *qrow = (const v4u *)(a.q + ((int64_t)qb * a.Hq + (int64_t)kvh * g + qh) * HD + 32 * kq);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            v4u w = (WALK == WALK_PREFIX ? live : c < g) ? qrow[s] : v4u{0, 0, 0, 0};
            qa[s] = __builtin_bit_cast(v8bf, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) qsum += bf16f(w[j] & 0xffffu) + bf16f(w[j] >> 16);
        }
    }
    qsum += __shfl_xor(qsum, 16);
    qsum += __shfl_xor(qsum, 32);
    float sq[4];                                       // sum(q) of the heads this lane's scores belong to (4 kq + r)
#pragma unroll
    for (int r = 0; r < 4; ++r) sq[r] = __shfl(qsum, 4 * kq + r);

    float m[4], lsum[4], pz[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; lsum[r] = 0.0f; pz[r] = 0.0f; }
    float acc[GP][8];
#pragma unroll
    for (int h = 0; h < GP; ++h)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[h][e] = 0.0f;

    const int dg = l & 15, tq = l >> 4;                // p.V layout: dims 8 dg .. 8 dg + 7 of tokens 4 i + tq
    for (int tb = t0 + TILE * wave; tb < t1; tb += TILE * DEC_WAVES) {
        // ---- scores of tokens tb + 16 G + c for heads 4 kq + r
        float sc[2][4], sv[2], zv[2];                  // sv, zv: the V row's (scale, zero) of the token
#pragma unroll
        for (int G = 0; G < 2; ++G) {
            int64_t rk;
            const bool ok = k_row(kv, pages, tb + 16 * G + c, t1, kvh, rk);
            if (kq == 0) s_row[wave][16 * G + c] = ok ? rk + v_offset(kv) : -1;
            v4f d = {0.0f, 0.0f, 0.0f, 0.0f};
            if (KIND == KV_INT4) {
                v4u kc = *(const v4u *)(kv.data + rk * (HD / 2) + 16 * kq);
                const uint32_t pk = *(const uint32_t *)(kv.param + rk * 2);
                const uint32_t pv = *(const uint32_t *)(kv.param + (rk + v_offset(kv)) * 2);
                if (!ok) kc = v4u{0, 0, 0, 0};
                // the conversions stay inside the selects: which of the products below the compiler fuses follows this shape
                const float sk = ok ? scale_of(pk) : 0.0f, zk = ok ? zero_of(pk) : 0.0f;
                sv[G] = ok ? scale_of(pv) : 0.0f;
                zv[G] = ok ? zero_of(pv) : 0.0f;
#pragma unroll
                for (int s = 0; s < 4; ++s) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[s], codes_to_bf16(kc[s]), d, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[G][r] = sk * d[r] - (16.0f * sk + zk) * sq[r];
            } else if (KIND == KV_FP8) {
                const v4u *kr = (const v4u *)(kv.data + rk * HD + 32 * kq);      // dims 32 kq .. 32 kq + 31: step s is dwords 2 s, 2 s + 1
                v4u kc[2];
                kc[0] = ok ? kr[0] : v4u{0, 0, 0, 0};
                kc[1] = ok ? kr[1] : v4u{0, 0, 0, 0};
                const uint32_t pk = *(const uint32_t *)(kv.param + rk * 2);
                const uint32_t pv = *(const uint32_t *)(kv.param + (rk + v_offset(kv)) * 2);
                const float sk = ok ? scale_of(pk) : 0.0f;
                sv[G] = ok ? scale_of(pv) : 0.0f;
                zv[G] = 0.0f;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const v2u lo = fp8x4_to_bf16(kc[s >> 1][2 * (s & 1)]), hi = fp8x4_to_bf16(kc[s >> 1][2 * (s & 1) + 1]);
                    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[s], __builtin_bit_cast(v8bf, (v4u{lo.x, lo.y, hi.x, hi.y})), d, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[G][r] = sk * d[r];
            } else {
                const v4u *kr = (const v4u *)(kv.data + rk * (HD * 2) + 64 * kq);
                v4u kb[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) kb[s] = ok ? kr[s] : v4u{0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < 4; ++s) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[s], __builtin_bit_cast(v8bf, kb[s]), d, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[G][r] = d[r];
                sv[G] = 1.0f;
                zv[G] = 0.0f;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) sc[G][r] = ok ? sc[G][r] * a.scale_log2 : -INFINITY;
        }
        // ---- online softmax (log2 domain); the tile always holds a valid token, so the new max is finite
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mt = fmaxf(sc[0][r], sc[1][r]);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) mt = fmaxf(mt, __shfl_xor(mt, o));
            const float mn = fmaxf(m[r], mt), alpha = exp2f(m[r] - mn);
            const float p0 = exp2f(sc[0][r] - mn), p1 = exp2f(sc[1][r] - mn);
            m[r] = mn;
            lsum[r] = lsum[r] * alpha + p0 + p1;
            pz[r] = pz[r] * alpha + p0 * zv[0] + p1 * zv[1];
            s_p[wave][c][4 * kq + r] = p0 * sv[0];
            s_p[wave][16 + c][4 * kq + r] = p1 * sv[1];
            if (c == 0) s_alpha[wave][4 * kq + r] = alpha;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's own LDS exchange (LDS operations of a wave run in order)
        // ---- p.V
#pragma unroll
        for (int h = 0; h < GP; ++h) {
            const float al = s_alpha[wave][h];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[h][e] *= al;
        }
        int64_t rv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) rv[i] = s_row[wave][4 * i + tq];
        if (KIND == KV_INT4) {
            uint32_t vc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) vc[i] = *(const uint32_t *)(kv.data + (rv[i] < 0 ? 0 : rv[i]) * (HD / 2) + 4 * dg);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (rv[i] < 0) continue;
                float cv[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    cv[2 * j] = (float)((vc[i] >> (8 * j)) & 15u);
                    cv[2 * j + 1] = (float)((vc[i] >> (8 * j + 4)) & 15u);
                }
#pragma unroll
                for (int h = 0; h < GP; ++h) {
                    const float p = s_p[wave][4 * i + tq][h];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[h][e] = fmaf(p, cv[e], acc[h][e]);
                }
            }
        } else if (KIND == KV_FP8) {
            v2u vc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) vc[i] = *(const v2u *)(kv.data + (rv[i] < 0 ? 0 : rv[i]) * HD + 8 * dg);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (rv[i] < 0) continue;
                float cv[8];
                fp8x4_to_f32(vc[i].x, cv);
                fp8x4_to_f32(vc[i].y, cv + 4);
#pragma unroll
                for (int h = 0; h < GP; ++h) {
                    const float p = s_p[wave][4 * i + tq][h];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[h][e] = fmaf(p, cv[e], acc[h][e]);
                }
            }
        } else {
            v4u vb[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) vb[i] = *(const v4u *)(kv.data + (rv[i] < 0 ? 0 : rv[i]) * (HD * 2) + 16 * dg);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (rv[i] < 0) continue;
                float vv[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    vv[2 * j] = bf16f(vb[i][j] & 0xffffu);
                    vv[2 * j + 1] = bf16f(vb[i][j] >> 16);
                }
#pragma unroll
                for (int h = 0; h < GP; ++h) {
                    const float p = s_p[wave][4 * i + tq][h];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[h][e] = fmaf(p, vv[e], acc[h][e]);
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads of this tile's exchange done before the next tile writes it
    }

    // ---- wave totals: acc over the four token lanes tq, l and sum(p z) over the 16 token lanes c
#pragma unroll
    for (int h = 0; h < GP; ++h)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            acc[h][e] += __shfl_xor(acc[h][e], 16);
            acc[h][e] += __shfl_xor(acc[h][e], 32);
        }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            lsum[r] += __shfl_xor(lsum[r], o);
            pz[r] += __shfl_xor(pz[r], o);
        }
    if (c == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * kq + r < GP) {
                s_ml[wave][4 * kq + r][0] = m[r];
                s_ml[wave][4 * kq + r][1] = lsum[r];
                s_alpha[wave][4 * kq + r] = pz[r];
            }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (tq == 0) {
#pragma unroll
        for (int h = 0; h < GP; ++h) {
            const float zsum = s_alpha[wave][h];
#pragma unroll
            for (int e = 0; e < 8; ++e) s_o[wave][h][8 * dg + e] = acc[h][e] - zsum;
        }
    }
    __syncthreads();

    // ---- merge the four waves: thread -> (head, 128 / 2 dims pair)
    const bool single = WALK <= WALK_WINDOW && a.nc == 1;
    int rows = g;                                      // the rows with an output
    if constexpr (WALK == WALK_PREFIX) rows = members * g;
    for (int idx = threadIdx.x; idx < rows * (HD / 2); idx += 256) {
        const int row = idx / (HD / 2), d = 2 * (idx % (HD / 2));
        int h = row;                                   // the head within the sequence b that owns the row
        if constexpr (WALK == WALK_PREFIX) {
            const int mi = row / g;
            b = sh.group_members[slab + mi];
            if (b < 0 || b >= kv.B) continue;
            h = row - mi * g;
        }
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < DEC_WAVES; ++w) M = fmaxf(M, s_ml[w][row][0]);
        float ls = 0.0f, o0 = 0.0f, o1 = 0.0f;
        if (M != -INFINITY) {
#pragma unroll
            for (int w = 0; w < DEC_WAVES; ++w) {
                const float f = exp2f(s_ml[w][row][0] - M);    // 0 for a wave without tokens
                ls += f * s_ml[w][row][1];
                o0 += f * s_o[w][row][d];
                o1 += f * s_o[w][row][d + 1];
            }
        }
        const int hq = kvh * g + h;
        if (single) {
            const float inv = ls > 0.0f ? 1.0f / ls : 0.0f;
            *(uint32_t *)(a.o + ((int64_t)b * a.Hq + hq) * HD + d) = pack_bf(o0 * inv, o1 * inv);
        } else {
            const int64_t part = (((int64_t)b * kv.Hkv + kvh) * a.nc + cidx) * g + h;
            *(float2 *)(a.ws + part * HD + d) = make_float2(o0, o1);
            if (d == 0) *(float2 *)(a.ws + (int64_t)kv.B * a.Hq * a.nc * HD + part * 2) = make_float2(M, ls);
        }
    }
