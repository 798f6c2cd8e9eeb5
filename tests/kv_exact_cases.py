"""Inputs for which paged attention and kv_append have an exactly known answer (tests/test_kv_exact_cpu.py, test_kv_exact_gpu.py).

Plain numpy, no torch, no GPU.  Every builder returns K / V as float32 [tokens, Hkv, 128] holding bf16 values, the tokens of the
sequences one after the other, plus what the answer must be.

grids    V rows are multiples of 1/8 in [-1, 0.875] with both ends present: the int4 rule gives scale 0.125, zero 1.0 and the codes
         reproduce the row bit for bit, so one V serves both cache kinds.  v_grid(seq, pos, head) writes the bits of its three
         arguments into the row (v_decode reads them back), so a wrong output names the token it came from.
needle   K of position t is a fixed +-1 code u_h(t); the query of (position p, head r) is 8 u(target): the target's score leads every
         other by >= 40 nats (asserted from the code book), so o = V[target] within 2^-20.
ramp     K of position t holds t's base-16 digits; q = +-512 (1, 16, 256, 4096, 0 ...): the score is +-512 t / sqrt(128), 45 nats
         per token, so a query returns V of its own position (rising) or of position 0 (falling).
count    q = 0 and V[t, d] = 1.875 [d == t % 128]: o[d] = 1.875 count_d(p) / (p + 1).
edge     rows that reach the clamps, ties, floor and saturation of the int4 rule.
"""
from __future__ import annotations

import functools

import numpy as np

HD = 128
PAGE_SIZES = (1, 16, 24, 64)
G_VALUES = (1, 2, 3, 4, 5, 7, 8, 12, 16)
EXACT_BOUND = 2.0 ** -20          # needle / ramp: p = 1, l = 1 and V on the 1/8 grid; the rest weighs <= 32768 e^-40 < 2e-13
MARGIN_NATS = 40.0
MAX_POS = 32768


def bf16_bits(x):
    """float32 values that ARE bf16 values -> their uint16 bit patterns"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    assert not (b & 0xFFFF).any(), "not a bf16 value"
    return (b >> 16).astype(np.uint16)


def to_bf16(x):
    """round float values to bf16 (half to even), returned as float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def indptr_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def page_table(lens, P, seed, spare=3, free_page0=True):
    """shuffled pages for sequences of the given lengths -> (kv_indptr, kv_indices, last_page_len, max_pages); with free_page0 no
    sequence owns page 0 (the kernels form the addresses of invalid slots from row 0, so page 0 should hold poison)"""
    npg = [-(-n // P) for n in lens]
    max_pages = sum(npg) + spare + 1
    first = 1 if free_page0 else 0
    perm = np.random.default_rng(seed).permutation(np.arange(first, max_pages))[: sum(npg)].astype(np.int32)
    last = np.array([n - (k - 1) * P if k else 0 for n, k in zip(lens, npg)], dtype=np.int32)
    return indptr_of(npg), perm, last, max_pages


def prefix_table(pages, P, lens):
    """page table of sequences that are all prefixes (lens[b] tokens) of ONE physical sequence whose pages are `pages`"""
    npg = [-(-n // P) for n in lens]
    indices = np.concatenate([pages[:k] for k in npg] + [np.zeros(0, np.int32)]).astype(np.int32)
    last = np.array([n - (k - 1) * P if k else 0 for n, k in zip(lens, npg)], dtype=np.int32)
    return indptr_of(npg), indices, last


def empty_host_cache(kind, max_pages, L, Hkv, P, poison):
    """host image of an empty cache: zeros, or (poison) bf16 NaN 0x7FC0 / 0xFF codes with fp16 NaN 0x7E00 parameters everywhere"""
    if kind == "int4":
        data = np.full((max_pages, L, 2, Hkv, P, 64), 0xFF if poison else 0, dtype=np.uint8)
        param = np.full((max_pages, L, 2, Hkv, P, 2), 0x7E00 if poison else 0, dtype=np.uint16).view(np.float16)
        return data, param
    return np.full((max_pages, L, 2, Hkv, P, HD), 0x7FC0 if poison else 0, dtype=np.uint16), None


# ---- value grids -----------------------------------------------------------------------------------------------------------
_FIELDS = ((15, "pos"), (3, "head"), (4, "seq"))         # bits of each argument, 5 dims per bit, from dim 2 on


def v_grid(seq, pos, head):
    """float32 [..., 128]: dim 0 = -1, dim 1 = 0.875, then +-0.5 for every bit of pos (15), head (3), seq (4), 5 dims each; the
    last 16 dims are 0.  Two rows of different (seq % 16, pos, head % 8) differ in at least 5 dims by 1.0."""
    seq, pos, head = np.broadcast_arrays(np.asarray(seq, dtype=np.int64), np.asarray(pos, dtype=np.int64), np.asarray(head, dtype=np.int64))
    out = np.zeros(pos.shape + (HD,), dtype=np.float32)
    out[..., 0], out[..., 1] = -1.0, 0.875
    d = 2
    for (nb, _), val in zip(_FIELDS, (pos, head, seq)):
        for i in range(nb):
            out[..., d:d + 5] = np.where((val >> i) & 1, 0.5, -0.5)[..., None]
            d += 5
    return out


def v_decode(row):
    """'seq s pos p head h' read back from an output row (the dims' signs), for failure messages"""
    row, d, vals = np.asarray(row, dtype=np.float64), 2, {}
    for nb, name in _FIELDS:
        vals[name] = sum(int(row[d + 5 * i: d + 5 * i + 5].mean() > 0) << i for i in range(nb))
        d += 5 * nb
    return f"seq {vals['seq']} pos {vals['pos']} head {vals['head']}"


def describe_mismatch(got, want, labels, bound, grid=True):
    """None if |got - want| <= bound everywhere, else a message naming the first bad row and (grid: V rows of v_grid) the token its
    output holds, otherwise its worst dimension; got, want [rows, 128], bound a scalar or an array that broadcasts, labels(i) -> str"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    bad = np.flatnonzero(((err > bound) | ~np.isfinite(err)).any(-1))
    if bad.size == 0:
        return None
    i = int(bad[0])
    if not grid:
        d = int(np.nanargmax(np.where(np.isfinite(err[i]), err[i], np.inf)))
        return (f"{bad.size} of {err.shape[0]} rows outside the bound; first: {labels(i)} dim {d} expects {want[i, d]!r}, got "
                f"{got[i, d]!r} (bound {np.broadcast_to(bound, err.shape)[i, d]:.3e})")
    return (f"{bad.size} of {err.shape[0]} rows outside the bound, worst err {np.nanmax(err):.3e}; first: {labels(i)} expects "
            f"{v_decode(want[i])}, got {v_decode(got[i])} (err {np.nanmax(err[i]):.3e})")


# ---- needle ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def codebook(h):
    """the +-1 codes of kv head h, int8 [32768, 128]; a shorter sequence uses the first rows"""
    return (np.random.default_rng(1000 + h).integers(0, 2, (MAX_POS, HD), dtype=np.int8) * 2 - 1).astype(np.int8)


@functools.lru_cache(maxsize=None)
def _worst_correlation(h, n):
    u = codebook(h)[:n].astype(np.float32)
    worst = -HD
    for i in range(0, n, 2048):
        gm = u[i:i + 2048] @ u.T                       # exact: integers up to 128
        k = np.arange(gm.shape[0])
        gm[k, i + k] = -HD
        worst = max(worst, int(gm.max()))
    return worst


def worst_correlation(h, n):
    """max over t != t' < n of u_h(t) . u_h(t') (computed on the next of 512 / 4608 / 32768 rows: an upper bound)"""
    return _worst_correlation(h, next(m for m in (512, 4608, MAX_POS) if m >= n)) if n > 1 else -HD


def needle_margin_nats(heads, n):
    """the least lead, in nats of score at sm_scale = 128^-0.5, of a query 8 u(target) over any other of the first n tokens.
    The int4 cache holds a +-1 row as {0.9331, -1.0664} = 0.99975 u - 0.0667: a per-query shift, and the factor taken here."""
    worst = max(worst_correlation(h, n) for h in range(heads))
    margin = (HD - worst) * 8.0 * 0.9997 / np.sqrt(HD)
    assert margin >= MARGIN_NATS, f"code book margin {margin:.1f} nats (worst correlation {worst} of 128)"
    return margin


def edge_positions(pmax, P):
    """position 0 and both sides of every multiple of 32 and of every page edge, within 0..pmax"""
    e = {0}
    for step in {32, P}:
        m = np.arange(step, pmax + 1, step)
        e.update(m.tolist(), (m - 1).tolist())
    return sorted(e)


def needle_prefill(g, Hkv, P, prior, new, seed):
    """targets[token, head] <= the token's position: one head of every query names its own position, the next p - 1; the others
    take the edge positions below the new tokens (nearest first), then random ones"""
    Hq, rng = g * Hkv, np.random.default_rng(seed)
    assert Hq >= 3
    lens = [a + n for a, n in zip(prior, new)]
    needle_margin_nats(Hkv, max(lens))
    K = np.concatenate([np.stack([codebook(h)[:n] for h in range(Hkv)], 1) for n in lens]).astype(np.float32)
    V = np.concatenate([v_grid(b, np.arange(n)[:, None], np.arange(Hkv)[None, :]) for b, n in enumerate(lens)])
    targets, seqs = [], []
    for b, (a, n) in enumerate(zip(prior, new)):
        tg = np.full((n, Hq), -1, dtype=np.int64)
        p = a + np.arange(n)
        tg[np.arange(n), np.arange(n) % Hq] = p
        tg[np.arange(n), (np.arange(n) + 1) % Hq] = np.maximum(p - 1, 0)
        free = np.argwhere(tg < 0)
        rest = [e for e in edge_positions(a + n - 1, P) if e < a - 1][::-1] if n else []
        for (j, hq), e in zip(free, rest):
            tg[j, hq] = e
        for j, hq in free[len(rest):]:
            tg[j, hq] = rng.integers(0, a + j + 1)
        targets.append(tg)
        seqs.append(np.full((n, Hq), b))
    targets, seqs = np.concatenate(targets), np.concatenate(seqs)
    kvh = np.arange(Hq) // g
    q = np.stack([8.0 * codebook(h)[targets[:, hq]] for hq, h in enumerate(kvh)], 1).astype(np.float32)
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, prior=list(prior), new=list(new), lens=lens, K=K, V=V, q=q, targets=targets,
                expect=v_grid(seqs, targets, kvh[None, :]).astype(np.float64))


def needle_prefill_uncovered(c):
    """what the targets of a needle_prefill case fail to cover, computed from its shapes alone (empty: full coverage)"""
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
    pmax = max((a + n - 1 for a, n in zip(c["prior"], c["new"]) if n), default=-1)
    return missing + [e for e in edge_positions(pmax, c["P"]) if e not in seen]


def needle_decode(g, Hkv, P, lengths, seed):
    """ONE physical sequence of max(lengths) tokens and many single-token queries over prefixes of it (lens[b] tokens each, sharing
    its pages): for every length n the targets cover n - 1, n - 2 and edge_positions(n - 1, P), Hq per sequence"""
    Hq, rng, N = g * Hkv, np.random.default_rng(seed), max(lengths)
    needle_margin_nats(Hkv, N)
    K = np.stack([codebook(h)[:N] for h in range(Hkv)], 1).astype(np.float32)
    V = v_grid(0, np.arange(N)[:, None], np.arange(Hkv)[None, :])
    lens, targets = [], []
    for n in lengths:
        req = sorted(set(edge_positions(n - 1, P)) | {n - 1, max(n - 2, 0)})[::-1]
        req += rng.integers(0, n, (-len(req)) % Hq + Hq).tolist()              # fill the last sequence, plus one random one
        targets += [req[i:i + Hq] for i in range(0, len(req), Hq)]
        lens += [n] * (len(req) // Hq)
    targets, kvh = np.array(targets, dtype=np.int64), np.arange(Hq) // g
    order = rng.permutation(len(lens))                                         # lengths mixed within every launch
    lens, targets = [lens[i] for i in order], targets[order]
    q = np.stack([8.0 * codebook(h)[targets[:, hq]] for hq, h in enumerate(kvh)], 1).astype(np.float32)
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, N=N, lengths=list(lengths), lens=lens, K=K, V=V, q=q, targets=targets,
                expect=v_grid(0, targets, kvh[None, :]).astype(np.float64))


def needle_decode_uncovered(c):
    missing = []
    for n in c["lengths"]:
        rows = [i for i, m in enumerate(c["lens"]) if m == n]
        assert (c["targets"][rows] < n).all() and (c["targets"][rows] >= 0).all()
        seen = set(c["targets"][rows].ravel().tolist())
        missing += [(n, e) for e in set(edge_positions(n - 1, P=c["P"])) | {n - 1, max(n - 2, 0)} if e not in seen]
    return missing


# (g, Hkv, P): every g of the issue, every page size; Hkv = 4 at g = 1 so that a query has heads left beyond p and p - 1
NEEDLE_PREFILL_SHAPES = [(1, 4, 16), (2, 2, 1), (3, 2, 24), (4, 2, 64), (5, 2, 16), (7, 2, 1), (8, 2, 24), (12, 2, 64), (16, 2, 16)]


def needle_prefill_case(i):
    """ragged batch: n_b in {0, 1, BQ - 1, BQ, BQ + 1, several tiles}, priors 0 .. 300; the last sequence is the longest and has the
    heads to cover every edge below it"""
    g, Hkv, P = NEEDLE_PREFILL_SHAPES[i]
    bq, Hq = 64 // g, g * Hkv
    big = max(3 * bq + 5, -(-320 // (Hq - 2)) + 8)
    return needle_prefill(g, Hkv, P, [5, 0, 200, 0, 200, 77, 300], [0, 1, bq - 1, bq, bq + 1, 2 * bq + 3, big], seed=300 + i)


def needle_prefill_every_alignment(i):
    """priors 0 .. 63, three query tiles and one token each: the diagonal and p - 1 targets at every alignment of a query tile's
    rows against the 64-token kv tiles (no edge coverage is claimed here)"""
    g, Hkv, P = NEEDLE_PREFILL_SHAPES[i]
    return needle_prefill(g, Hkv, P, RAMP_RESIDUES, [3 * (64 // g) + 1] * 64, seed=350 + i)


def needle_prefill_32k():
    """768 new tokens that end at position 32767 (g = 4, P = 16): 4608 free heads for the 4094 edges below them"""
    n = 768
    return needle_prefill(4, 2, 16, [MAX_POS - n], [n], seed=399)


# (g, Hkv, P, lengths): the 32k context once, on the usual page size
NEEDLE_DECODE_SHAPES = [(4, 2, 16, (1, 31, 32, 33, 4096, 32768)), (8, 2, 1, (1, 31, 32, 33, 4096)), (5, 2, 24, (1, 31, 32, 33, 4096)),
                        (16, 2, 64, (1, 31, 32, 33, 4096))]


def needle_decode_case(i):
    g, Hkv, P, lengths = NEEDLE_DECODE_SHAPES[i]
    return needle_decode(g, Hkv, P, lengths, seed=400 + i)


# ---- ramp ------------------------------------------------------------------------------------------------------------------
def ramp_k(pos):
    """float32 [..., 128]: base-16 digits of pos in dims 0..3, 0 in dim 4, 15 in dim 5 (int4: scale 1, base 0, exact codes)"""
    pos = np.asarray(pos, dtype=np.int64)
    out = np.zeros(pos.shape + (HD,), dtype=np.float32)
    for i in range(4):
        out[..., i] = (pos >> (4 * i)) & 15
    out[..., 5] = 15.0
    return out


def ramp_q(sign=1.0):
    q = np.zeros(HD, dtype=np.float32)
    q[:4] = sign * 512.0 * 16.0 ** np.arange(4)
    return q


# the diagonal inside a kv tile (37) and on EVERY multiple of 64 up to 1280: split-KV chunks are multiples of 64 tokens, so whatever
# chunk length the library picks below 1280, a diagonal starts on each chunk edge and others on plain tile edges
RAMP_PRIORS = [37] + list(range(0, 1281, 64))


RAMP_RESIDUES = list(range(64))                  # every alignment of a query tile's rows against the 64-token kv tiles


def ramp_prefill(g, Hkv, P, sign, priors=RAMP_PRIORS):
    """every row of three whole query tiles and one more token, per prior; all heads ask the same: rising -> V[p], falling -> V[0]"""
    bq, Hq, priors = 64 // g, g * Hkv, list(priors)
    new = [3 * bq + 1] * len(priors)
    lens = [a + n for a, n in zip(priors, new)]
    K = np.concatenate([np.repeat(ramp_k(np.arange(n))[:, None], Hkv, 1) for n in lens])
    V = np.concatenate([v_grid(b, np.arange(n)[:, None], np.arange(Hkv)[None, :]) for b, n in enumerate(lens)])
    T = sum(new)
    q = np.broadcast_to(ramp_q(sign), (T, Hq, HD)).copy()
    pos = np.concatenate([a + np.arange(n) for a, n in zip(priors, new)])
    seq = np.repeat(np.arange(len(new)), new)
    want_pos = pos if sign > 0 else np.zeros_like(pos)
    expect = v_grid(seq[:, None], want_pos[:, None], (np.arange(Hq) // g)[None, :]).astype(np.float64)
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, prior=priors, new=new, lens=lens, K=K, V=V, q=q, pos=pos, expect=expect)


RAMP_DECODE_LENGTHS = sorted(set(range(1, 131)) | {255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768})


def ramp_decode(g, Hkv, P, sign, lengths=RAMP_DECODE_LENGTHS):
    """single-token queries over prefixes of one 32768-token ramp: rising -> V[len - 1], falling -> V[0]"""
    Hq, N = g * Hkv, max(lengths)
    K = np.repeat(ramp_k(np.arange(N))[:, None], Hkv, 1)
    V = v_grid(0, np.arange(N)[:, None], np.arange(Hkv)[None, :])
    q = np.broadcast_to(ramp_q(sign), (len(lengths), Hq, HD)).copy()
    want_pos = np.array(lengths) - 1 if sign > 0 else np.zeros(len(lengths), dtype=np.int64)
    expect = v_grid(0, want_pos[:, None], (np.arange(Hq) // g)[None, :]).astype(np.float64)
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, N=N, lens=list(lengths), K=K, V=V, q=q, expect=expect)


# ---- counting --------------------------------------------------------------------------------------------------------------
def count_v(pos):
    """float32 [..., 128]: 1.875 where d == pos % 128, else 0 (int4: scale 0.125, base 0, codes 15 / 0)"""
    pos = np.asarray(pos, dtype=np.int64)
    return np.where(np.arange(HD) == (pos % HD)[..., None], np.float32(1.875), np.float32(0.0)).astype(np.float32)


def count_expect(p):
    """float64 [..., 128]: the mean of count_v over positions 0..p, 1.875 count_d(p) / (p + 1)"""
    p = np.asarray(p, dtype=np.int64)[..., None]
    cnt = np.where(np.arange(HD) <= p, (p - np.arange(HD)) // HD + 1, 0)
    return 1.875 * cnt / (p + 1.0)


def bf16_ulp(want):
    """the bf16 ulp at each (fp64) value; 0 at 0, where the answer must be 0 exactly"""
    w = np.abs(np.asarray(want, dtype=np.float64))
    return np.where(w > 0, 2.0 ** (np.floor(np.log2(np.maximum(w, 1e-300))) - 7), 0.0)


# (g, Hkv, P, prior, new): lengths up to 4096, ragged, every page size
COUNT_PREFILL_CASES = [
    (4, 2, 16, [0, 4000, 127, 128, 1000], [300, 96, 2, 1, 17]),
    (1, 2, 1, [0, 129, 63], [130, 64, 65]),
    (5, 2, 24, [0, 3000, 255], [65, 1096, 13]),
    (16, 2, 64, [0, 4090, 500], [20, 6, 9]),
]
COUNT_DECODE_SHAPES = [(4, 2, 16), (2, 2, 1), (7, 2, 24), (12, 2, 64)]
COUNT_DECODE_LENGTHS = sorted(set(range(1, 70)) | {127, 128, 129, 255, 256, 257, 1000, 2047, 2048, 2049, 4095, 4096})


def count_prefill(g, Hkv, P, prior, new):
    Hq = g * Hkv
    lens = [a + n for a, n in zip(prior, new)]
    K = np.concatenate([np.repeat(ramp_k(np.arange(n))[:, None], Hkv, 1) for n in lens])
    V = np.concatenate([np.repeat(count_v(np.arange(n))[:, None], Hkv, 1) for n in lens])
    pos = np.concatenate([a + np.arange(n) for a, n in zip(prior, new)])
    expect = np.repeat(count_expect(pos)[:, None], Hq, 1)
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, prior=list(prior), new=list(new), lens=lens, K=K, V=V,
                q=np.zeros((sum(new), Hq, HD), dtype=np.float32), pos=pos, expect=expect)


def count_decode(g, Hkv, P, lengths=COUNT_DECODE_LENGTHS):
    Hq, N = g * Hkv, max(lengths)
    K = np.repeat(ramp_k(np.arange(N))[:, None], Hkv, 1)
    V = np.repeat(count_v(np.arange(N))[:, None], Hkv, 1)
    expect = np.repeat(count_expect(np.array(lengths) - 1)[:, None], Hq, 1)
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, N=N, lens=list(lengths), K=K, V=V, q=np.zeros((len(lengths), Hq, HD), dtype=np.float32),
                expect=expect)


# ---- edge rows of the int4 rule ------------------------------------------------------------------------------------------------
BF16_MAX = float(np.array([0x7F7F0000], dtype=np.uint32).view(np.float32)[0])       # 3.3895e38


def edge_rows():
    """name -> float32 [128] of bf16 values; no NaN, no Inf"""
    r = {}
    r["zeros"] = np.zeros(HD)
    r["const_pos"] = np.full(HD, 3.0)
    r["const_neg"] = np.full(HD, -3.0)
    r["offset_pos"] = np.linspace(10.0, 11.0, HD)                 # base clamps to 0, every code to 15
    r["offset_neg"] = -np.linspace(10.0, 11.0, HD)                # base 15, every code 0
    r["halves"] = np.arange(HD) % 16 - 8 + 0.5                    # -7.5 .. 7.5: scale 1, x / s ties on every element
    r["tiny_range"] = (np.arange(HD) % 5) * 2.0e-6              # range 8e-6 < 1e-5: the floor, an fp16 subnormal scale
    r["tiny_single"] = np.where(np.arange(HD) == 77, 1e-7, 0.0)
    r["bf16_max"] = np.where(np.arange(HD) < 64, BF16_MAX, -BF16_MAX)   # max - min overflows fp32: scale and zero saturate
    r["outlier"] = np.where(np.arange(HD) == 5, 1e4, 1e-3)
    r["neg_zero"] = np.where(np.arange(HD) % 2 == 0, -0.0, 0.75 * (np.arange(HD) % 7))
    r["neg_zero_only"] = np.where(np.arange(HD) % 2 == 0, -0.0, 0.0)
    sub = np.array([0x0001, 0x8001, 0x007F, 0x0040], dtype=np.uint16)    # bf16 subnormals of both signs
    r["subnormal"] = (sub[np.arange(HD) % 4].astype(np.uint32) << 16).view(np.float32)
    r["subnormal_mixed"] = np.where(np.arange(HD) % 2 == 0, r["subnormal"], np.linspace(-2.0, 1.0, HD))
    return {k: to_bf16(np.asarray(v, dtype=np.float32)) for k, v in r.items()}


def edge_batch(Hkv, seed):
    """k, v float32 [T, Hkv, 128]: every edge row once as K and once as V, on rotating heads, between Gaussian rows"""
    rows, rng = list(edge_rows().values()), np.random.default_rng(seed)
    T = 2 * len(rows) + 3
    k = to_bf16(rng.standard_normal((T, Hkv, HD)).astype(np.float32) * 2.0)
    v = to_bf16(rng.standard_normal((T, Hkv, HD)).astype(np.float32) * 0.5)
    for i, row in enumerate(rows):
        k[2 * i, i % Hkv] = row
        v[2 * i + 1, (i + 1) % Hkv] = row
        v[2 * i, (i + 2) % Hkv] = row
    return k, v
