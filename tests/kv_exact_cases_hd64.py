"""tests/kv_exact_cases.py for the paged cache of 64-wide heads (include/micromix_kv_hd64.h, micromix_kv_prefill_hd64.h): inputs whose
answer is known exactly, for tests/test_kv_exact_hd64_cpu.py (which proves every statement below) and test_kv_exact_hd64_gpu.py.

Plain numpy.  Every builder returns K / V as float32 [tokens, Hkv, 64] holding bf16 values, the sequences one after the other, and what
the answer must be.  Every row is exact in BOTH cache kinds, bf16 and fp8 (e4m3 codes under a power-of-two scale per row), so one K / V
serves both and the fp8 result has to equal the bf16 one bit for bit.  sm_scale is 1/8 throughout.

grid     V rows are multiples of 1/8 in [-1, 0.875] with both ends present: fp8 gives e = -8 and x * 256 has at most four significant
         bits.  v_grid(seq, pos, head) writes the bits of its arguments into the signs of the row, two dims per bit; v_decode reads them back.
needle   K of position t is the +-1 code codebook(h)[t, :64] (e = -8, exact); the query is 16 u(target): the score is 2 (u . u'), 128 on
         the target and at most 2 * 42 elsewhere among 4608 tokens, a lead of 44 nats (asserted from the code book), so o = V[target]
         within 2^-20.
ramp     K of position t holds t's base-16 digits (kv_exact_cases.ramp_k's first 64 dims: e = -4, digit * 16 has four bits);
         q = +-512 (1, 16, 256, 4096, 0 ...): 64 nats per token.  Rising returns V of the query's position, falling V[0].
count    q = 0 and V[t, d] = 1.875 [d == t % 64] (e = -7, 240): o[d] = 1.875 count_d / n to 1 bf16 ulp.

The shapes stand where the 64-wide kernels can go wrong: page sizes that do not divide the 64-token tile (3, 24), equal it (64) and
exceed it (100); every g of G_VALUES (the decode kernel's GP = 4 / 8 / 16 instantiations change at 4 | 5 and 8 | 9); lengths and priors
on both sides of every tile edge and of every chunk edge that the library's plan reports -- the builders take the plan as a function,
nothing here restates it.
"""
from __future__ import annotations

import functools

import numpy as np

import kv_exact_cases as kc
from kv_exact_cases import EXACT_BOUND, G_VALUES, MARGIN_NATS, bf16_bits, bf16_ulp, codebook, indptr_of, page_table, prefix_table  # noqa: F401

HD = 64
TILE = 64                                   # MM_KV_HD64_DECODE_TILE = MM_KV_PREFILL_HD64_TILE (asserted in the CPU test)
PAGE_SIZES = (1, 3, 16, 24, 64, 100)
SM_SCALE = 0.125
MAX_LEN = 4608                              # the longest sequence: 72 tiles, 18 rounds of the decode kernel's four waves
DECODE_GROUP = 8                            # sequences per decode launch: few enough that the library splits 4608 tokens into chunks


def empty_host_cache(kind, max_pages, L, Hkv, P, poison=True):
    """host image (data, param) of an empty 64-wide cache: zeros, or (poison) bf16 NaN 0x7FC0 / e4m3 NaN codes 0x7F with fp16 NaN params"""
    shape = (max_pages, L, 2, Hkv, P)
    if kind == "bf16":
        return np.full(shape + (HD,), 0x7FC0 if poison else 0, dtype=np.uint16), None
    return (np.full(shape + (HD,), 0x7F if poison else 0, dtype=np.uint8),
            np.full(shape + (2,), 0x7E00 if poison else 0, dtype=np.uint16).view(np.float16))


# ---- value grid ------------------------------------------------------------------------------------------------------------
_FIELDS = ((15, "pos"), (3, "head"), (4, "seq"))        # bits of each argument, 2 dims per bit, from dim 2 on: 44 dims
_REP = 2


def v_grid(seq, pos, head):
    """float32 [..., 64]: dim 0 = -1, dim 1 = 0.875, then +-0.5 for every bit of pos (15), head (3), seq (4), 2 dims each; the last 18
    dims are 0.  Two rows of different (seq % 16, pos, head % 8) differ in at least 2 dims by 1.0."""
    seq, pos, head = np.broadcast_arrays(np.asarray(seq, dtype=np.int64), np.asarray(pos, dtype=np.int64), np.asarray(head, dtype=np.int64))
    out = np.zeros(pos.shape + (HD,), dtype=np.float32)
    out[..., 0], out[..., 1] = -1.0, 0.875
    d = 2
    for (nb, _), val in zip(_FIELDS, (pos, head, seq)):
        for i in range(nb):
            out[..., d:d + _REP] = np.where((val >> i) & 1, 0.5, -0.5)[..., None]
            d += _REP
    return out


def v_decode(row):
    """'seq s pos p head h' read back from an output row (the dims' signs), for failure messages"""
    row, d, vals = np.asarray(row, dtype=np.float64), 2, {}
    for nb, name in _FIELDS:
        vals[name] = sum(int(row[d + _REP * i: d + _REP * i + _REP].mean() > 0) << i for i in range(nb))
        d += _REP * nb
    return f"seq {vals['seq']} pos {vals['pos']} head {vals['head']}"


def describe_mismatch(got, want, labels, bound, grid=True):
    """kv_exact_cases.describe_mismatch for rows of 64"""
    return kc.describe_mismatch(got, want, labels, bound, grid, decode=v_decode)


# ---- needle ----------------------------------------------------------------------------------------------------------------
def code(h, n):
    """the +-1 codes of kv head h for positions 0 .. n - 1, int8 [n, 64]: the first 64 dims of kv_exact_cases.codebook"""
    assert n <= MAX_LEN
    return codebook(h)[:n, :HD]


@functools.lru_cache(maxsize=None)
def worst_correlation(h):
    """max over t != t' < MAX_LEN of u_h(t) . u_h(t'): an upper bound for every shorter sequence"""
    u = code(h, MAX_LEN).astype(np.float32)
    gm = u @ u.T                                           # exact: integers up to 64
    np.fill_diagonal(gm, -HD)
    return int(gm.max())


def needle_margin_nats(heads):
    """the least lead, in nats of score at sm_scale = 1/8, of a query 16 u(target) over any other of MAX_LEN tokens; both cache kinds hold
    +-1 exactly, so no factor is taken off"""
    worst = max(worst_correlation(h) for h in range(heads))
    margin = (HD - worst) * 16.0 * SM_SCALE
    assert margin >= MARGIN_NATS, f"code book margin {margin:.1f} nats (worst correlation {worst} of 64)"
    return margin


def edge_positions(pmax, P, page_lo=0):
    """position 0 and both sides of every multiple of 64 and of every page edge >= page_lo, within 0 .. pmax"""
    e = {0}
    m = np.arange(TILE, pmax + 1, TILE)
    e.update(m.tolist(), (m - 1).tolist())
    m = np.arange(P, pmax + 1, P)
    m = m[m >= page_lo]
    e.update(m.tolist(), (m - 1).tolist())
    return sorted(e)


def _needle_q(targets, g):
    kvh = np.arange(targets.shape[1]) // g
    return np.stack([16.0 * codebook(h)[targets[:, hq], :HD] for hq, h in enumerate(kvh)], 1).astype(np.float32), kvh


def needle_prefill(g, Hkv, P, prior, new, seed, cover=None):
    """targets[token, head] <= the token's position: one head of every query names its own position, the next p - 1.  The free heads
    of sequence `cover` take every edge position below it that nobody's diagonal holds (so that, over the batch, every edge up to
    the cover sequence's last position is somebody's target); those of every other sequence the edges nearest below it, then random
    positions.  cover None: the sequence with the most free heads."""
    Hq, rng = g * Hkv, np.random.default_rng(seed)
    assert Hq >= 3
    lens = [a + n for a, n in zip(prior, new)]
    assert max(lens) <= MAX_LEN
    needle_margin_nats(Hkv)
    K = np.concatenate([np.stack([code(h, n) for h in range(Hkv)], 1) for n in lens]).astype(np.float32)
    V = np.concatenate([v_grid(b, np.arange(n)[:, None], np.arange(Hkv)[None, :]) for b, n in enumerate(lens)])
    cover = int(np.argmax(new)) if cover is None else cover
    diagonal = set()
    for a, n in zip(prior, new):
        diagonal.update(range(max(a - 1, 0), a + n))
    targets, seqs = [], []
    for b, (a, n) in enumerate(zip(prior, new)):
        tg = np.full((n, Hq), -1, dtype=np.int64)
        p = a + np.arange(n)
        tg[np.arange(n), np.arange(n) % Hq] = p
        tg[np.arange(n), (np.arange(n) + 1) % Hq] = np.maximum(p - 1, 0)
        free = np.argwhere(tg < 0)
        below = [e for e in edge_positions(a + n - 1, P) if e <= a][::-1] if n else []
        rest = [e for e in below if e not in diagonal] if b == cover else below
        for (j, hq), e in zip(free, rest):
            tg[j, hq] = e
        for j, hq in free[len(rest):]:
            tg[j, hq] = rng.integers(0, a + j + 1)
        targets.append(tg)
        seqs.append(np.full((n, Hq), b))
    targets, seqs = np.concatenate(targets), np.concatenate(seqs)
    q, kvh = _needle_q(targets, g)
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, prior=list(prior), new=list(new), lens=lens, K=K, V=V, q=q, targets=targets, cover=cover,
                expect=v_grid(seqs, targets, kvh[None, :]).astype(np.float64))


def needle_prefill_uncovered(c):
    """what the targets of a needle_prefill case fail to cover, from its shapes alone (empty: full coverage): every query's own position
    and p - 1, and -- over the batch -- position 0 and both sides of every multiple of 64 and of every page edge up to the cover
    sequence's last position"""
    missing, seen, t0 = [], set(), 0
    for a, n in zip(c["prior"], c["new"]):
        tg = c["targets"][t0:t0 + n]
        t0 += n
        for j in range(n):
            p = a + j
            assert (tg[j] >= 0).all() and (tg[j] <= p).all(), "a target after its query"
            if p not in tg[j] or max(p - 1, 0) not in tg[j]:
                missing.append(("diagonal", a, j))
        seen.update(tg.ravel().tolist())
    b = c["cover"]
    return missing + [e for e in edge_positions(c["prior"][b] + c["new"][b] - 1, c["P"]) if e not in seen]


def decode_required(n, N, P):
    """the targets a decode length n must cover: n - 1, n - 2, position 0, both sides of every multiple of 64 below n, and both sides of
    every page edge within the last two tiles (the full length N: of every page edge)"""
    return sorted(set(edge_positions(n - 1, P, 0 if n == N else max(n - 1 - 2 * TILE, 0))) | {n - 1, max(n - 2, 0)})


def needle_decode(g, Hkv, P, lengths, seed):
    """ONE physical sequence of max(lengths) tokens and many single-token queries over prefixes of it (lens[b] tokens each, sharing
    its pages): for every length n the targets cover decode_required(n), Hq per sequence"""
    Hq, rng, N = g * Hkv, np.random.default_rng(seed), max(lengths)
    needle_margin_nats(Hkv)
    K = np.stack([code(h, N) for h in range(Hkv)], 1).astype(np.float32)
    V = v_grid(0, np.arange(N)[:, None], np.arange(Hkv)[None, :])
    lens, targets = [], []
    for n in lengths:
        req = decode_required(n, N, P)[::-1]
        req += rng.integers(0, n, (-len(req)) % Hq).tolist()                   # fill the last sequence
        targets += [req[i:i + Hq] for i in range(0, len(req), Hq)]
        lens += [n] * (len(req) // Hq)
    targets = np.array(targets, dtype=np.int64)
    order = rng.permutation(len(lens))                                         # lengths mixed within every launch
    lens, targets = [lens[i] for i in order], targets[order]
    q, kvh = _needle_q(targets, g)
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, N=N, lengths=list(lengths), lens=lens, K=K, V=V, q=q, targets=targets,
                expect=v_grid(0, targets, kvh[None, :]).astype(np.float64))


def needle_decode_uncovered(c):
    missing = []
    for n in c["lengths"]:
        rows = [i for i, m in enumerate(c["lens"]) if m == n]
        assert (c["targets"][rows] < n).all() and (c["targets"][rows] >= 0).all()
        seen = set(c["targets"][rows].ravel().tolist())
        missing += [(n, e) for e in decode_required(n, c["N"], c["P"]) if e not in seen]
    return missing


# ---- ramp and count --------------------------------------------------------------------------------------------------------
def ramp_k(pos):
    """float32 [..., 64]: base-16 digits of pos in dims 0..3, 0 in dim 4, 15 in dim 5 (fp8: e = -4 in every row)"""
    return kc.ramp_k(pos)[..., :HD]


def ramp_q(sign=1.0):
    return kc.ramp_q(sign)[:HD]


def ramp_prefill(g, Hkv, P, sign, prior, new):
    """every head of every new token asks the same: rising -> V of its own position, falling -> V[0]"""
    Hq = g * Hkv
    lens = [a + n for a, n in zip(prior, new)]
    K = np.concatenate([np.repeat(ramp_k(np.arange(n))[:, None], Hkv, 1) for n in lens])
    V = np.concatenate([v_grid(b, np.arange(n)[:, None], np.arange(Hkv)[None, :]) for b, n in enumerate(lens)])
    q = np.broadcast_to(ramp_q(sign), (sum(new), Hq, HD)).copy()
    pos = np.concatenate([a + np.arange(n) for a, n in zip(prior, new)] + [np.zeros(0, np.int64)]).astype(np.int64)
    seq = np.repeat(np.arange(len(new)), new)
    want_pos = pos if sign > 0 else np.zeros_like(pos)
    expect = v_grid(seq[:, None], want_pos[:, None], (np.arange(Hq) // g)[None, :]).astype(np.float64)
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, prior=list(prior), new=list(new), lens=lens, K=K, V=V, q=q, pos=pos, expect=expect)


def ramp_decode(g, Hkv, P, sign, lengths):
    """single-token queries over prefixes of one ramp of max(lengths) tokens: rising -> V[len - 1], falling -> V[0]"""
    Hq, N = g * Hkv, max(lengths)
    K = np.repeat(ramp_k(np.arange(N))[:, None], Hkv, 1)
    V = v_grid(0, np.arange(N)[:, None], np.arange(Hkv)[None, :])
    q = np.broadcast_to(ramp_q(sign), (len(lengths), Hq, HD)).copy()
    want_pos = np.array(lengths) - 1 if sign > 0 else np.zeros(len(lengths), dtype=np.int64)
    expect = v_grid(0, want_pos[:, None], (np.arange(Hq) // g)[None, :]).astype(np.float64)
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, N=N, lengths=list(lengths), lens=list(lengths), K=K, V=V, q=q, expect=expect)


def count_v(pos):
    """float32 [..., 64]: 1.875 where d == pos % 64, else 0"""
    pos = np.asarray(pos, dtype=np.int64)
    return np.where(np.arange(HD) == (pos % HD)[..., None], np.float32(1.875), np.float32(0.0)).astype(np.float32)


def count_expect(p, present=None):
    """float64 [..., 64]: the mean of count_v over positions 0..p, 1.875 count_d(p) / (p + 1); p = -1: zeros.  present (bool [n], one
    p): the mean over the positions <= p that are present only -- what a sequence with pages off the cache must give"""
    if present is not None:
        t = np.flatnonzero(present[: int(p) + 1])
        return 1.875 * np.bincount(t % HD, minlength=HD) / max(len(t), 1)
    p = np.asarray(p, dtype=np.int64)[..., None]
    cnt = np.where(np.arange(HD) <= p, (p - np.arange(HD)) // HD + 1, 0)
    return 1.875 * cnt / np.maximum(p + 1.0, 1.0)


def count_prefill(g, Hkv, P, prior, new):
    Hq = g * Hkv
    lens = [a + n for a, n in zip(prior, new)]
    K = np.concatenate([np.repeat(ramp_k(np.arange(n))[:, None], Hkv, 1) for n in lens])
    V = np.concatenate([np.repeat(count_v(np.arange(n))[:, None], Hkv, 1) for n in lens])
    pos = np.concatenate([a + np.arange(n) for a, n in zip(prior, new)] + [np.zeros(0, np.int64)]).astype(np.int64)
    expect = np.repeat(count_expect(pos)[:, None], Hq, 1)
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, prior=list(prior), new=list(new), lens=lens, K=K, V=V,
                q=np.zeros((sum(new), Hq, HD), dtype=np.float32), pos=pos, expect=expect)


def count_decode(g, Hkv, P, lengths):
    Hq, N = g * Hkv, max(lengths)
    K = np.repeat(ramp_k(np.arange(N))[:, None], Hkv, 1)
    V = np.repeat(count_v(np.arange(N))[:, None], Hkv, 1)
    expect = np.repeat(count_expect(np.array(lengths) - 1)[:, None], Hq, 1)
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, N=N, lengths=list(lengths), lens=list(lengths), K=K, V=V,
                q=np.zeros((len(lengths), Hq, HD), dtype=np.float32), expect=expect)


# ---- shapes ----------------------------------------------------------------------------------------------------------------
# (g, Hkv, P): every g of G_VALUES, every page size; Hkv = 4 at g = 1 so that a query has heads left beyond p and p - 1
SHAPES = [(1, 4, 16), (2, 2, 3), (3, 2, 24), (4, 2, 64), (5, 2, 100), (7, 2, 1), (8, 2, 3), (12, 2, 100), (16, 2, 24)]
BASE_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)     # the tile, two tiles, a round of the decode kernel's four waves


def decode_bounds(N=MAX_LEN):
    """the three max_seq_len a decode case runs under: one chunk (a sequence longer than the bound is attended in full all the same),
    tight, loose"""
    return (4 * TILE, N, 4 * N)


def decode_lengths(plan, Hkv, N=MAX_LEN):
    """the lengths of a decode case: BASE_LENGTHS, N, and both sides of every chunk edge of plan(DECODE_GROUP, Hkv, bound) ->
    (chunks, chunk_len) under each bound of decode_bounds (a length c * chunk_len ends a chunk, + 1 starts the next, - 1 leaves a hole)"""
    out = set(BASE_LENGTHS) | {N}
    for bound in decode_bounds(N):
        nc, cl = plan(DECODE_GROUP, Hkv, bound)
        out |= {c * cl + s for c in range(1, nc) for s in (-1, 0, 1)}
    return sorted(n for n in out if 1 <= n <= N)


def decode_groups(B):
    """the launches of a decode case: DECODE_GROUP sequences each, the last one wrapping round to the first sequences"""
    assert B >= DECODE_GROUP
    return [[(i + j) % B for j in range(DECODE_GROUP)] for i in range(0, B, DECODE_GROUP)]


def prefill_batch(g, Hkv, P, rows, plan):
    """(prior, new) of the ragged batch of one workgroup shape, `rows` = 128 or 64 (token, head) rows, bq = rows / g query tokens per tile:
    new-token counts 0, 1, bq - 1, bq, bq + 1, several tiles and one sequence with the heads to cover every edge below it (index 6:
    the cover sequence); for 64 rows, which the library picks for few tokens per sequence, 64 one-token sequences at priors 0 .. 63;
    one sequence that ends at MAX_LEN; and a sequence whose first new token sits on each side of every chunk edge of
    plan(T, B, Hq, Hkv, MAX_LEN) -> (rows, tile_tokens, tiles, chunks, chunk_len), found by iterating: the plan depends on T and B"""
    bq, Hq = rows // g, g * Hkv
    big = max(2 * bq + 5, -(-len(edge_positions(299, P)) // (Hq - 2)) + 8)
    base = list(zip([5, 0, 200, 0, 200, 77, 300], [0, 1, bq - 1, bq, bq + 1, 2 * bq + 3, big]))
    edge_new = bq + 1 if rows == 128 else 1
    if rows == 64:
        base += [(a, 1) for a in range(64)]
    base.append((MAX_LEN - edge_new, edge_new))
    pairs, edges = base, set()
    for _ in range(16):                      # more sequences can mean fewer chunks: edges are only ever added, so this settles
        p = plan(sum(n for _, n in pairs), len(pairs), Hq, Hkv, MAX_LEN)
        more = {c * p[4] + s for c in range(1, p[3]) for s in (-1, 0) if c * p[4] + s + edge_new <= MAX_LEN}
        if more <= edges:
            break
        edges |= more
        pairs = base + [(a, edge_new) for a in sorted(edges)]
    else:
        raise AssertionError("the chunk edges of the plan did not settle")
    return [a for a, _ in pairs], [n for _, n in pairs]


def every_alignment(g, rows=128):
    """priors 0 .. 63 with three query tiles and one token each: every row of a query tile at every position within a 64-token kv tile"""
    return list(range(64)), [3 * (rows // g) + 1] * 64


def softmax_fp64(q, K, V, g, scale=SM_SCALE):
    """plain attention of q [Hq, 64] over K, V [n, Hkv, 64] in fp64 -> [Hq, 64]; n = 0: zeros"""
    q, K, V = (np.asarray(x, dtype=np.float64) for x in (q, K, V))
    if K.shape[0] == 0:
        return np.zeros(q.shape)
    s = np.einsum("hd,nhd->hn", q, np.repeat(K, g, axis=1)) * scale
    p = np.exp(s - s.max(-1, keepdims=True))
    return np.einsum("hn,nhd->hd", p / p.sum(-1, keepdims=True), np.repeat(V, g, axis=1))
