"""numpy fp64 oracle of mm_logprob_rows (include/micromix_logprob.h): the rule, the integer outputs from the bf16 bits alone, and the
bound on the values.  Nothing here shares code with the kernels.

t_prime(T)                         the temperature the rule uses: T if T > 0, else (None, T <= 0, NaN) 1
integers(bits, target, top_n)      (rank, top_idx): exact, from the order of the bits (sample_oracle.rank: any NaN above +inf, +0 == -0)
values(bits, T)                    (lse, logprob of every token) of one row in fp64: log_softmax(l / T'), NaN for a degenerate row
row(bits, target, T, top_n)        all five outputs of one row: logprob, rank, lse, top_idx, top_logprob
bound(bits, T, value)              how far the device's value may lie from the oracle's

The bound.  The device reports fl32(x - L~) with x = (l - m) / T' formed in fp64 from exact differences, and L~ = ln(S~ 2^-43) in fp64,
S~ the integer sum of sample.hip's masses W.  sample_oracle.mass_error bounds |S~ 2^-43 - S| by E(row), S = sum_i w_i >= 1, so
|L~ - L| <= E / S to first order.  The fp64 conversion of S~, the logarithm (a few ulp of a double near |L| < 14), the division
and the subtraction get the allowance 2^-40: thousands of times what they need and 2^-16 of the fp32 rounding that follows -- an
allowance, not a measurement.  The last rounding to fp32 is half an ulp, at most 2^-24 |value|; 2^-23 |value| covers it at the
oracle's value as well as at the device's, and 2^-126 keeps the term from vanishing at 0:

    B = E(row) / S + 2^-40 + 2^-23 max(|value|, 2^-126)

So that the bound cannot hide an error: E / S is at most sample_oracle's stated worst case 8e-6 on every row the tests use it on (it
computes to between 0.6e-6 and 1.4e-6 for Gaussian logits of standard deviation 3 at T from 0.5 to 2, the more the higher T);
tests/test_logprob_cpu.py asserts the cap on every such row.
"""
import functools
import math

import numpy as np

import sample_oracle as so

E_OVER_S_CAP = 8e-6


def t_prime(T):
    if T is None:
        return 1.0
    T = float(np.float32(T))
    return T if T > 0.0 else 1.0                               # NaN > 0 is false


def integers(bits, target, top_n):
    """(rank, top_idx [top_n]): the count of tokens above the target in the order (-1 for an ignored target, None for none), and the
    top_n tokens by descending order then ascending index, -1 beyond the vocabulary"""
    k = so.rank(bits)
    vocab = len(k)
    rank = None if target is None else -1 if not 0 <= int(target) < vocab else int((k > k[int(target)]).sum())
    top = np.full(top_n, -1, dtype=np.int64)
    first = np.argsort(-k, kind="stable")[:top_n]
    top[:len(first)] = first
    return rank, top


def values(bits, T=None):
    """(lse, logprob [vocab]) in fp64; every one NaN when the row's maximum is -inf, +inf or NaN"""
    v = so.values(bits)
    m, Tp = v[so.argmax(bits)], t_prime(T)
    if not np.isfinite(m):
        return math.nan, np.full(len(v), math.nan)
    with np.errstate(invalid="ignore"):
        x = np.where(v == -np.inf, -np.inf, (v - m) / Tp)     # -inf stays -inf whatever T'
    L = math.log(math.fsum(np.exp(x).tolist()))
    return m / Tp + L, x - L


def row(bits, target=None, T=None, top_n=0):
    """dict(logprob, rank, lse, top_idx, top_logprob) of one row as the header states them, the values in fp64"""
    rank, top = integers(bits, target, top_n)
    lse, lp = values(bits, T)
    ignored = rank is not None and rank < 0
    return dict(logprob=None if target is None else 0.0 if ignored else float(lp[int(target)]), rank=rank, lse=lse, top_idx=top,
                top_logprob=np.array([lp[i] if i >= 0 else -np.inf for i in top.tolist()], dtype=np.float64))


def e_over_s(bits, T=None):
    """E(row) / S of the docstring, for a row with a finite maximum"""
    w, t = so.weights(bits, t_prime(T))
    return so.mass_error(w, t) / float(w.sum())


def bound(e_s, value):
    """B for one value of a row whose E / S is e_s"""
    return e_s + 2.0 ** -40 + 2.0 ** -23 * max(abs(float(value)), 2.0 ** -126)


def check_value(got, want, e_s):
    """None when the device's fp32 `got` is within B of the oracle's `want` (NaN for NaN, an infinity for itself), else a message"""
    got, want = float(got), float(want)
    if math.isnan(want) or math.isinf(want):
        same = math.isnan(got) if math.isnan(want) else got == want
        return None if same else f"got {got}, want {want}"
    err = abs(got - want)
    return None if err <= bound(e_s, want) else f"got {got!r}, want {want!r}: off by {err:.3e}, bound {bound(e_s, want):.3e}"


# ---- inputs shared by the CPU and the GPU tests -----------------------------------------------------------------------------------------
GAUSSIAN_ROWS = 16


def gaussian_case(vocab, rows=GAUSSIAN_ROWS):
    """Gaussian logits of standard deviation 3 rounded to bf16, per-row temperatures that all differ (0.5 .. 2), a target per row"""
    rng = np.random.default_rng(1000 + vocab)
    bits = so.bf16_bits(rng.standard_normal((rows, vocab)) * 3.0)
    T = (0.5 + 1.5 * np.arange(rows) / max(rows - 1, 1)).astype(np.float32)
    target = rng.integers(0, vocab, rows).astype(np.int32)
    target[0] = so.argmax(bits[0])                             # one greedy target
    return bits, T, target


def long_row(vocab):
    bits, _, target = gaussian_case(vocab, 1)
    return bits, np.array([0.8], dtype=np.float32), target


TOP_N = 20


@functools.lru_cache(maxsize=None)
def gaussian_expected(vocab, rows=GAUSSIAN_ROWS):
    """[(oracle row, E / S)] of every row of the case: computed once, shared by the tests, left unchanged"""
    bits, T, target = long_row(vocab) if rows == 1 else gaussian_case(vocab, rows)
    return [(row(bits[r], int(target[r]), T[r], TOP_N), e_over_s(bits[r], T[r])) for r in range(rows)]


def random_bits(rows, vocab, seed):
    """rows of random bf16 bits with heavy ties: a handful of values, +0 with -0, NaNs of both signs and +-inf in some rows"""
    rng = np.random.default_rng(seed)
    pool = np.array([0x0000, 0x8000, 0x3F80, 0xBF80, 0x4000, 0x4040, 0xC040, 0x0001, 0x8001, 0x7F7F, 0xFF7F, 0xFF80], dtype=np.uint16)
    bits = pool[rng.integers(0, len(pool), (rows, vocab))]
    for r in range(rows):
        kind = r % 5
        n = max(1, vocab // 50)
        at = rng.integers(0, vocab, n)
        if kind == 1:
            bits[r, at] = 0x7F80                               # +inf, several times
        elif kind == 2:
            bits[r, at] = rng.choice(np.array([0x7FC0, 0xFFC0, 0x7F81, 0xFFFF], dtype=np.uint16), n)   # NaNs of both signs
        elif kind == 3:
            bits[r] = rng.integers(0, 1 << 16, vocab).astype(np.uint16)                                # every kind of value
        elif kind == 4:
            bits[r] = np.where(rng.random(vocab) < 0.9, 0xFF80, bits[r])                               # mostly -inf
    return bits
