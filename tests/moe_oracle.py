"""Numpy restatements of the sparse-MoE entries (include/micromix_hip.h, mm_moe_*), on bf16 bit patterns (uint16).

route     fp64: the top_k largest logits in descending order, equal logits in ascending expert index; w_j = exp(l_j - m) / sum over
          the selected, rounded once from fp64 to bf16 (nearest even)
plan      the stable counting sort of the (token, k-slot) pairs by expert; ids outside [0, E) uncounted, slot_of = -1, and
          sorted_token = -1 in the slots that no pair owns then
combine   per token in ascending expert id: c = bf16(y * w), acc = bf16(acc + c) from +0.0, fp32 arithmetic (the product of two bf16
          values is exact there), every rounding to nearest even; slot_of outside [0, n) skipped
inputs    the routing inputs shared by tests/test_moe_cpu.py and tests/test_moe_gpu.py
"""
from __future__ import annotations

import numpy as np

from oracle import mx_oracle as o


def f64_to_bf16(x):
    """float64, 0 or positive and normal as a bf16 -> bf16 bits, ONE rounding to nearest even (no detour over float32); 0 gives +0.0
    (frexp(0) = (0, 0))"""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)                                         # x = m * 2^e, m in [0.5, 1)
    q = np.rint(m * 256.0)                                     # 8 significant bits; rint rounds halves to even
    v = np.ldexp(q, e - 8).astype(np.float32)                  # exact: 8 bits, and the exponent is in range for these inputs
    assert np.all(v.view(np.uint32) & np.uint32(0xFFFF) == 0)
    return (v.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def route(logit_bits, top_k):
    """uint16 [T, E] -> (ids int32 [T, top_k], w bits uint16 [T, top_k], w float64 [T, top_k] before the rounding)"""
    l = o.bf16_to_f32(logit_bits).astype(np.float64)
    ids = np.argsort(-l, axis=1, kind="stable")[:, :top_k]     # stable: equal logits (and -0.0 = +0.0) keep the ascending index
    sel = np.take_along_axis(l, ids, axis=1)
    ex = np.exp(sel - sel[:, :1])
    w = ex / ex.sum(axis=1, keepdims=True)
    return ids.astype(np.int32), f64_to_bf16(w), w


def plan(ids, E):
    """int [T, top_k] -> (expert_offsets int32 [E + 1], sorted_token int32 [n], slot_of int32 [T, top_k])"""
    ids = np.asarray(ids)
    T, k = ids.shape
    flat = ids.reshape(-1).astype(np.int64)
    pairs = np.flatnonzero((flat >= 0) & (flat < E))
    order = pairs[np.argsort(flat[pairs], kind="stable")]      # the pairs in slot order
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat[pairs], minlength=E))]).astype(np.int32)
    sorted_token = np.full(T * k, -1, dtype=np.int32)
    sorted_token[: len(order)] = order // k
    slot_of = np.full(T * k, -1, dtype=np.int32)
    slot_of[order] = np.arange(len(order), dtype=np.int32)
    return offsets, sorted_token, slot_of.reshape(T, k)


def _round(x):
    return o.bf16_to_f32(o.f32_to_bf16(x))


def combine(y_bits, ids, w_bits, slot_of):
    """y uint16 [n, H], ids / w bits / slot_of [T, top_k] -> out bits uint16 [T, H]"""
    y, w = o.bf16_to_f32(y_bits), o.bf16_to_f32(w_bits)
    ids, slot_of = np.asarray(ids).astype(np.int64), np.asarray(slot_of)
    T, k = ids.shape
    order = np.argsort(ids * 8 + np.arange(k)[None, :], axis=1, kind="stable")      # ascending expert id, then k-slot
    acc = np.zeros((T, y.shape[1]), dtype=np.float32)
    rows = np.arange(T)
    for r in range(k):
        j = order[:, r]
        s = slot_of[rows, j]
        ok = (s >= 0) & (s < y.shape[0])
        c = _round(y[np.where(ok, s, 0)] * w[rows, j][:, None])
        acc = np.where(ok[:, None], _round(acc + c), acc)
    return o.f32_to_bf16(acc)


ROUTE_SHAPES = ((8, 2), (8, 1), (4, 4), (16, 8), (64, 8), (3, 2))
ROUTE_TOKENS = (1, 5, 64, 257)


def route_inputs(E, k, T):
    """{name: logits bits uint16 [T, E]}: Gaussian at scale 1 and 8 and rows with one dominant logit -- all three redrawn until the
    k-th and (k + 1)-th largest logits of every row differ (bf16 Gaussians collide now and then), so that the top-k SET does not hang
    on the tie rule -- and rows of equal logits, which test the tie rule itself"""
    rng = np.random.default_rng(1000 * E + 10 * k + T)

    def no_tie_at_k(draw):
        bits = o.f32_to_bf16(draw())
        for _ in range(200):
            s = -np.sort(-o.bf16_to_f32(bits), axis=1)
            bad = s[:, k - 1] == s[:, k] if k < E else np.zeros(T, dtype=bool)
            if not bad.any():
                return bits
            bits[bad] = o.f32_to_bf16(draw())[bad]
        raise AssertionError("could not draw rows without a tie at the k-th logit")

    def dominant():
        x = rng.standard_normal((T, E)).astype(np.float32)
        x[np.arange(T), rng.integers(0, E, T)] += 20.0
        return x

    return {"scale 1": no_tie_at_k(lambda: rng.standard_normal((T, E)).astype(np.float32)),
            "scale 8": no_tie_at_k(lambda: (8.0 * rng.standard_normal((T, E))).astype(np.float32)),
            "dominant": no_tie_at_k(dominant),
            "equal": o.f32_to_bf16(np.repeat(rng.standard_normal((T, 1)).astype(np.float32), E, axis=1))}


ROUTE_EDGE_SHAPES = ((8, 2), (64, 8), (3, 2))
ROUTE_EDGE_TOKENS = (5, 257)
FAR_GAPS = (20.0, 40.0, 60.0, 80.0, 30.0, 50.0, 70.0)


def route_edge_inputs(E, k, T):
    """{name: logits bits uint16 [T, E]} at the edges of the routing rule, 2 <= k < E:

    tie of 2 / of 3 at k   otherwise distinct logits (multiples of 0.5 around the tied value) whose k-th and (k + 1)-th largest are
                           equal, two or three experts sharing that value (three: the ranks k-1, k, k+1, or the last three where E
                           ends before that).  The tied experts sit at the lowest indices, at the highest, or at both ends (row mod 3);
                           in every other triple of rows the tied value is zero, -0.0 and +0.0 alternating over the tied experts, from
                           either sign.  The lower index wins.
    masked                 Gaussian logits, 1 .. E - k experts per row at -inf: every selected logit is finite
    k - 1 finite           exactly k - 1 finite logits per row: the k-th pick is the -inf expert of the lowest index, its weight +0.0
    far                    the selected logits 20 .. 80 below the row's largest (FAR_GAPS; all values integers, exact in bf16), the
                           others 100 below: weights down to e^-80 = 1.8e-35, still normal bf16 numbers, so f64_to_bf16 holds

    Out of contract and not generated: rows that are all -inf (the softmax is 0 / 0), NaN logits (no order), and weights in the
    bf16 subnormal range (gaps beyond ~87; the kernel's fp32 expf and f64_to_bf16 both stop being defined to the last bit there)."""
    assert 2 <= k < E
    rng = np.random.default_rng(7000 * E + 70 * k + T)
    ninf = np.float32(-np.inf)

    def tie(n):
        r0 = k - 1 if k - 1 + n <= E else E - n                # the first tied rank; the ranks r0 .. r0 + n - 1 straddle k - 1 | k
        assert r0 <= k - 1 and r0 + n - 1 >= k
        x = np.zeros((T, E), dtype=np.float32)
        for t in range(T):
            zero = (t // 3) % 2 == 1
            c = 0.0 if zero else (1.25, -3.0)[t % 2]
            ranks = np.arange(E)
            v = np.where(ranks < r0, c + 0.5 * (r0 - ranks), np.where(ranks < r0 + n, c, c - 0.5 * (ranks - (r0 + n - 1)))).astype(np.float32)
            tied = ([0, 1, 2][:n], [E - 3, E - 2, E - 1][-n:], [0, E // 2, E - 1] if n == 3 else [0, E - 1])[t % 3]
            assert len(set(tied)) == n
            rest = rng.permutation(np.setdiff1d(np.arange(E), tied))
            x[t, rest] = np.concatenate([v[:r0], v[r0 + n:]])
            x[t, tied] = [c if not zero else (-0.0, 0.0)[(i + t // 6) % 2] for i in range(n)]
            assert len(np.unique(x[t])) == E - n + 1
        bits = o.f32_to_bf16(x)
        assert np.array_equal(o.bf16_to_f32(bits), x) and np.array_equal(np.signbit(o.bf16_to_f32(bits)), np.signbit(x))
        return bits

    def masked():
        x = rng.standard_normal((T, E)).astype(np.float32)
        for t in range(T):
            x[t, rng.choice(E, 1 + t % (E - k), replace=False)] = ninf
        return o.f32_to_bf16(x)

    def few_finite():
        x = np.full((T, E), ninf, dtype=np.float32)
        for t in range(T):
            x[t, rng.choice(E, k - 1, replace=False)] = rng.standard_normal(k - 1).astype(np.float32)
        return o.f32_to_bf16(x)

    def far():
        x = np.zeros((T, E), dtype=np.float32)
        for t in range(T):
            top = (0.0, 50.0, 3.0)[t % 3]
            v = np.full(E, top - 100.0, dtype=np.float32)
            v[0] = top
            v[1:k] = [top - FAR_GAPS[(t + j) % len(FAR_GAPS)] for j in range(k - 1)]
            x[t] = v[rng.permutation(E)]
        bits = o.f32_to_bf16(x)
        assert np.array_equal(o.bf16_to_f32(bits), x)
        return bits

    return {"tie of 2 at k": tie(2), "tie of 3 at k": tie(3), "masked": masked(), "k - 1 finite": few_finite(), "far": far()}
