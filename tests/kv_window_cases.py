"""Inputs with an exactly known answer for sliding-window attention (tests/test_kv_window_cpu.py, test_kv_window_gpu.py), built from
the helpers of tests/kv_exact_cases.py.  Plain numpy.  A query at position p with window W attends positions max(0, p - W + 1) .. p.

count   q = 0 and V[t, d] = 1.875 [d == t % 128] (kc.count_v): o[d] = 1.875 (positions of the window congruent to d) / (its size).  One
        lost or extra token moves its dimension by about 1.875 / W, 29 bf16 ulps or more of the expected value at the windows used
        here (W <= 1024; asserted in test_kv_window_cpu.py), so the 1-ulp bound tells the window's two ends from their neighbours.
twin    the needle code is planted at TWO positions of a sequence with different grid-valued V rows; every query asks for it.  A query
        whose window holds one plant returns that plant's row (2^-20); one that holds both returns their exact mean, a multiple of 1/16
        in [-1, 0.875] and so a bf16 value (1 ulp); one that holds neither is not checked.  The rows of one query tile step the window's
        lower edge over a plant, so "p - W is outside, p - W + 1 is inside" is asked at consecutive positions.
"""
from __future__ import annotations

import numpy as np

import kv_exact_cases as kc

HD = 128
WINDOWS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300, 1024)
HEADS = ((1, 1), (4, 1), (5, 1), (16, 1), (8, 2))             # (Hq, Hkv)
PAGE_SIZES = (1, 16, 24)
EDGE_MAX = 520                                                # window starts up to here: past 2 chunk edges of 256 tokens


def window_begin(p, W):
    return np.maximum(np.asarray(p, dtype=np.int64) - W + 1, 0)


def count_window_expect(p, W):
    """float64 [..., 128]: the mean of kc.count_v over positions window_begin(p, W) .. p"""
    p = np.asarray(p, dtype=np.int64)[..., None]
    lo = window_begin(p, W)
    d = np.arange(HD)
    upto = lambda x: np.where(x >= d, (x - d) // HD + 1, 0)          # positions 0 .. x congruent to d (x = -1: none)
    return 1.875 * (upto(p) - upto(lo - 1)) / (p - lo + 1.0)


def window_starts(P):
    """the window starts a count case visits: position 0, every position up to 70, and both sides of every multiple of 32 (so of 64
    and of the 256-token chunks too) and of every page edge up to EDGE_MAX"""
    return sorted(set(kc.edge_positions(EDGE_MAX, P if P > 1 else 32)) | set(range(70)))


def count_decode_lengths(W, P):
    """sequence lengths for window W: shorter than the window, equal to it, and W + e for every window start e > 0"""
    return sorted({1, max(W - 1, 1), W} | {W + e for e in window_starts(P)})


def count_decode(Hq, Hkv, P, W, lengths=None):
    """single-token queries over prefixes of one physical sequence"""
    lengths = count_decode_lengths(W, P) if lengths is None else list(lengths)
    N = max(lengths)
    K = np.repeat(kc.ramp_k(np.arange(N))[:, None], Hkv, 1)
    V = np.repeat(kc.count_v(np.arange(N))[:, None], Hkv, 1)
    expect = np.repeat(count_window_expect(np.array(lengths) - 1, W)[:, None], Hq, 1)
    return dict(g=Hq // Hkv, Hq=Hq, Hkv=Hkv, P=P, W=W, N=N, lens=lengths, K=K, V=V, q=np.zeros((len(lengths), Hq, HD), dtype=np.float32),
                expect=expect)


def count_prefill_shape(g, W):
    """(prior, new): n_b in {1, BQ - 1, BQ, BQ + 1, several tiles, 70, a few}; the first token's window starts at 31, 63, 64, just below
    128, 0 (a sequence that outgrows the window within the tile) and 250 -- whose 70 tokens step it over 256, a tile, page and chunk
    edge; the last sequence stays within the window"""
    bq = 64 // g
    new = [1, max(bq - 1, 1), bq, bq + 1, 3 * bq + 1, 70, min(W, 9)]
    start = [31, 63, 64, 127 - bq, None, 250]
    prior = [max(W - 4, 0) if e is None else e + W - 1 for e in start] + [0]
    return prior, new


def count_prefill(Hq, Hkv, P, W):
    g = Hq // Hkv
    prior, new = count_prefill_shape(g, W)
    lens = [a + n for a, n in zip(prior, new)]
    K = np.concatenate([np.repeat(kc.ramp_k(np.arange(n))[:, None], Hkv, 1) for n in lens])
    V = np.concatenate([np.repeat(kc.count_v(np.arange(n))[:, None], Hkv, 1) for n in lens])
    pos = np.concatenate([a + np.arange(n) for a, n in zip(prior, new)])
    expect = np.repeat(count_window_expect(pos, W)[:, None], Hq, 1)
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, W=W, prior=prior, new=new, lens=lens, K=K, V=V, q=np.zeros((sum(new), Hq, HD), dtype=np.float32),
                pos=pos, expect=expect)


# ---- twin needle ---------------------------------------------------------------------------------------------------------------
TWIN_WINDOWS = (1, 2, 32, 33, 64, 65, 128, 300, 1024)


def twin_shape(g, W, decode):
    """(prior, new, plants) per sequence.  Plants a < b, both inside one window when W >= 2.  Sequence 0 steps the lower edge over
    plant a (queries p = a + W - 2 .. a + W + 1: both plants, both, both with a the first token inside, then b alone with a at p - W),
    sequence 1 over plant b as well, sequence 2 is shorter than the window; decode takes one query per sequence instead."""
    bq = 64 // g
    gap = max(1, min(W - 1, 5))                                   # b = a + gap: inside a window that starts at a (W = 1: never both)
    out = []
    if decode:
        a = 37 if W < 64 else 200                                 # a window start inside a 32-token tile / past a chunk edge
        for p in (a + W - 2, a + W - 1, a + W, a + gap + W - 1, a + gap + W):
            if p >= a + gap:                                      # both plants written
                out.append((p, 1, (a, a + gap)))
        out.append((max(W - 2, 1), 1, (0, min(gap, max(W - 2, 1)))))       # shorter than the window: position 0 is attended
        return out
    for a, n in ((37, 8), (63, 2 * bq + 3), (250, 12)):
        b = a + gap
        first = max(a + W - 3, b)                                 # the first query: two positions before a becomes the window's start
        out.append((first, n + gap, (a, b)))
    out.append((0, max(min(W - 1, 9), 1), (0, 0)))               # one plant at position 0, the sequence within the window
    return out


def twin(Hq, Hkv, P, W, decode):
    g = Hq // Hkv
    shape = twin_shape(g, W, decode)
    prior, new = [s[0] for s in shape], [s[1] for s in shape]
    lens = [a + n for a, n in zip(prior, new)]
    N = max(lens)
    kc.needle_margin_nats(Hkv, N + 1)
    Ks, Vs, expect, checked = [], [], [], []
    kvh = np.arange(Hq) // g
    for s, ((a0, n, plants), L) in enumerate(zip(shape, lens)):
        K = np.stack([kc.codebook(h)[:L] for h in range(Hkv)], 1).astype(np.float32)
        for t in set(plants):
            K[t] = np.stack([kc.codebook(h)[N] for h in range(Hkv)])               # the needle: row N of the code book, used by no token
        Ks.append(K)
        Vs.append(kc.v_grid(s, np.arange(L)[:, None], np.arange(Hkv)[None, :]))
        for j in range(n):
            p = a0 + j
            seen = sorted({t for t in plants if window_begin(p, W) <= t <= p})
            checked.append(len(seen))
            rows = [kc.v_grid(s, t, kvh) for t in seen] or [np.zeros((Hq, HD), dtype=np.float32)]
            expect.append(np.mean(np.stack(rows).astype(np.float64), axis=0))
    q = np.broadcast_to(np.stack([8.0 * kc.codebook(h)[N] for h in kvh]).astype(np.float32), (sum(new), Hq, HD)).copy()
    return dict(g=g, Hq=Hq, Hkv=Hkv, P=P, W=W, N=N, prior=prior, new=new, lens=lens, K=np.concatenate(Ks), V=np.concatenate(Vs), q=q,
                expect=np.stack(expect), plants_seen=np.array(checked))


def twin_bound(c):
    """[T, 1, 1]-broadcastable bound per query: one plant 2^-20 (kc.EXACT_BOUND: p = 1, the rest weighs < n e^-40); two plants 1 bf16
    ulp of the mean (and 2^-20 where the mean is 0, for the same rest); no plant: not checked (inf)"""
    ulp = np.maximum(kc.bf16_ulp(c["expect"]), kc.EXACT_BOUND)
    seen = c["plants_seen"][:, None, None]
    return np.where(seen == 0, np.inf, np.where(seen == 1, kc.EXACT_BOUND, ulp))


# ---- released pages ------------------------------------------------------------------------------------------------------------
def released_entries(kv_indptr, lens, new, P, W):
    """indices into kv_indices of the pages whose positions all lie below len_b - n_b - W + 1 (n_b = 0: below len_b - W)"""
    out = []
    for b, (L, n) in enumerate(zip(lens, new)):
        bound = L - max(n, 1) - W + 1
        out += [int(kv_indptr[b]) + i for i in range(max(bound, 0) // P)]
    return out
