"""numpy fp64 oracle of mm_sample_rows (include/micromix_hip.h): the rule, the error bound of the device's masses, and from the two the
admissible set of a row.  Nothing here shares code with the kernels.

sample(bits, u, T, k, p, q)        the rule, in plain loops over classes and tokens: the token of one row
kept_mask(bits, T, k, p, q)        the kept set of one row (None for a greedy row)
admissible(bits, u, T, k, p, q)    every token a device within the bound below may return; the rule's own token is among them

The bound.  Per token the device computes (csrc/sample.hip)
    c~ = fl(fl(log2 e) / T)          the constant is rounded to fp32 (2^-24 relative), the division is IEEE (2^-24)
    t~ = fl(fl(l - m) * c~)          the difference of two bf16 values is rounded to fp32 (2^-24), and so is the product (2^-24)
    w~ = V_EXP_F32(t~)               "1 ULP accuracy, denormals are flushed" (CDNA3 / CDNA4 instruction set reference): 2^-23 relative
    W  = trunc(w~ * 2^43)            a 64-bit integer: 0 <= w~ - W / 2^43 < 2^-43
so with t = (l - m) log2 e / T, |t~ - t| <= |t| 2^-22 to first order and
    |w~ - w| <= w * e(t),   e(t) = (|t| ln 2 * 2^-22 + 2^-23) * (1 + 2^-10)          (the last factor covers the second-order terms;
                                                                                      |t| < 44 wherever W can be non-zero)
An exp2 result below 2^-126 is flushed to 0, as is W for w~ < 2^-43: both inside the 2^-43 of the truncation.  Every mass the device
compares is an INTEGER sum of W's -- exact, in any order, at any depth: the fp32 summation depth is 0 and contributes nothing -- so for
any set S of tokens
    | sum_S W / 2^43 - sum_S w |  <=  E(S) = sum_{i in S} w_i e(t_i) + |S| 2^-43                                        (mass_error)
The targets u * Z and p * Z_k are formed in fp64 from an integer Z and truncated: 2^-52 relative and 2^-43 absolute more.  A comparison
"prefix mass against target" over the set S therefore cannot be decided wrongly unless the two are within
    D(S) = 2 E(S) + 2^-42 + Z 2^-50                                                                                      (margin)
of each other, and eps = D(S) / Z is the bound on a prefix mass relative to Z.  For Gaussian logits of standard deviation 3 at T = 1
the mass-weighted mean of |t| ln 2 is about 3.6, so eps is about 2e-6; the worst case over all rows is e(44) = 7.4e-6 a side.
top-k compares integer counts and has no error.  min-p compares w~ with q in fp32: a class is undecided when |w - q| <= w e(t).
"""
import functools
import math

import numpy as np

ONE_MINUS = 1.0 - 2.0 ** -24


def values(bits):
    """fp64 values of bf16 bits"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def rank(bits):
    """mm_argmax_rows' order: any NaN above +inf, +0 == -0, otherwise the order of the reals"""
    bits = np.asarray(bits, dtype=np.uint16).astype(np.int64)
    mag, negative = bits & 0x7FFF, (bits >> 15) == 1
    return np.where(mag > 0x7F80, 1 << 20, np.where(negative, -mag, mag))


def argmax(bits):
    r = rank(bits)
    return int(np.flatnonzero(r == r.max())[0])


def clamp_u(u):
    u = float(np.float32(u))
    return 0.0 if math.isnan(u) else min(max(u, 0.0), ONE_MINUS)


def is_greedy(bits, T):
    m = values(bits)[argmax(bits)]
    T = float(np.float32(T))
    return bool(not np.isfinite(m) or math.isnan(T) or T <= 0.0)


def weights(bits, T):
    """(w, t) of a row that is not greedy: w_i = exp((l_i - m) / T) with -inf -> 0, t_i = (l_i - m) log2 e / T (-inf -> -inf)"""
    v = values(bits)
    m, T = v[argmax(bits)], float(np.float32(T))
    w, t = np.zeros(len(v)), np.full(len(v), -np.inf)
    for i, l in enumerate(v.tolist()):
        if l == m:
            w[i], t[i] = 1.0, 0.0
        elif l != -np.inf:
            w[i] = math.exp((l - m) / T) if not math.isinf(T) else 1.0
            t[i] = (l - m) / T / math.log(2.0) if not math.isinf(T) else 0.0
    return w, t


def filters(k, p, q, vocab):
    """the three parameters as the rule reads them: None where a filter is off"""
    k = None if k is None or not 1 <= int(k) < vocab else int(k)
    p = None if p is None or math.isnan(float(np.float32(p))) or float(np.float32(p)) >= 1.0 else max(float(np.float32(p)), 0.0)
    q = None if q is None or not 0.0 < float(np.float32(q)) <= 1.0 else float(np.float32(q))
    return k, p, q


def classes(bits):
    """the classes of a row in descending order: (value, indices) with +0 and -0 in one"""
    v = values(bits)
    order = np.argsort(-v, kind="stable")                    # descending values, ascending index inside a class; -0.0 == 0.0
    out, start = [], 0
    for i in range(1, len(order) + 1):
        if i == len(order) or v[order[i]] != v[order[start]]:
            out.append((float(v[order[start]]), np.sort(order[start:i])))
            start = i
    return out


def prefix_ends(bits, T, k, p, q):
    """(cls, w, t, end_k, end_p, end_q, mass): the classes, and for each filter the number of classes its prefix holds (len(cls) when
    off); mass[c] the total weight of the first c classes"""
    w, t = weights(bits, T)
    cls = classes(bits)
    k, p, q = filters(k, p, q, len(w))
    count, mass = [0], [0.0]
    for _, idx in cls:
        count.append(count[-1] + len(idx))
        mass.append(mass[-1] + float(w[idx].sum()))
    n = len(cls)
    end_k = n if k is None else next(c for c in range(1, n + 1) if count[c] >= k)
    zk = mass[end_k]
    end_p = n if p is None else next(c for c in range(1, n + 1) if mass[c] >= p * zk)
    end_q = n if q is None else max(c for c in range(1, n + 1) if w[cls[c - 1][1][0]] >= q)
    return cls, w, t, end_k, end_p, end_q, mass


def mask_of(cls, end, vocab):
    keep = np.zeros(vocab, dtype=bool)
    for _, idx in cls[:end]:
        keep[idx] = True
    return keep


def kept_mask(bits, T, k=None, p=None, q=None):
    if is_greedy(bits, T):
        return None
    cls, w, _, end_k, end_p, end_q, _ = prefix_ends(bits, T, k, p, q)
    return mask_of(cls, min(end_k, end_p, end_q), len(w))


def draw(w, keep, u):
    """the first kept index whose cumulative kept mass exceeds u * Z; if rounding leaves none, the last kept index with w > 0"""
    Z = float(w[keep].sum())
    run, last = 0.0, -1
    for i in np.flatnonzero(keep).tolist():
        run += w[i]
        if w[i] > 0:
            last = i
        if run > u * Z:
            return i
    return last


def sample(bits, u, T=1.0, k=None, p=None, q=None):
    if is_greedy(bits, T):
        return argmax(bits)
    w, _ = weights(bits, T)
    return draw(w, kept_mask(bits, T, k, p, q), clamp_u(u))


# ---- the bound --------------------------------------------------------------------------------------------------------------------
def rel_error(t):
    """e(t): the relative error of the device's weight of a token at exponent t"""
    return (np.abs(np.where(np.isfinite(t), t, 0.0)) * math.log(2.0) * 2.0 ** -22 + 2.0 ** -23) * (1.0 + 2.0 ** -10)


def mass_error(w, t, keep=None):
    """E(S): how far the device's mass of the tokens S (a mask; None: all) can lie from the exact one"""
    keep = np.ones(len(w), dtype=bool) if keep is None else keep
    return float((w[keep] * rel_error(t[keep])).sum()) + int(keep.sum()) * 2.0 ** -43


def margin(w, t, keep=None):
    """D(S): two masses over S, or a mass and a target formed from one, closer than this may compare either way on the device"""
    keep = np.ones(len(w), dtype=bool) if keep is None else keep
    return 2.0 * mass_error(w, t, keep) + 2.0 ** -42 + float(w[keep].sum()) * 2.0 ** -50


def admissible_ends(bits, T, k=None, p=None, q=None):
    """the numbers of classes a device within the bound may keep (a sorted list; the rule's own is among them), and what prefix_ends
    returned"""
    pe = prefix_ends(bits, T, k, p, q)
    cls, w, t, end_k, end_p, end_q, mass = pe
    k, p, q = filters(k, p, q, len(w))
    n = len(cls)
    ends_p, ends_q = [end_p], [end_q]
    if p is not None:
        d = margin(w, t, mask_of(cls, end_k, len(w)))
        tgt = max(p * mass[end_k], 2.0 ** -43)
        ends_p = [c for c in range(1, end_k + 1) if mass[c] >= tgt - d and mass[c - 1] < tgt + d]
    if q is not None:
        def undecided(c):
            i = cls[c - 1][1][0]
            return abs(w[i] - q) <= w[i] * rel_error(t[i])
        lo = end_q
        while lo > 1 and undecided(lo):
            lo -= 1
        hi = end_q
        while hi < n and undecided(hi + 1):
            hi += 1
        ends_q = list(range(lo, hi + 1))
    return sorted({min(end_k, a, b) for a in ends_p for b in ends_q}), pe


def admissible_many(bits, us, T=1.0, k=None, p=None, q=None):
    """the tokens a device within the bound may return for the row, for each u of `us` (a list of sets): for every admissible kept set
    K, every kept token i with w_i > 0 and u * Z inside [C(i - 1) - D(K), C(i) + D(K)], C the cumulative kept mass in index order"""
    if is_greedy(bits, T):
        return [{argmax(bits)} for _ in us]
    ends, (cls, w, t, *_rest) = admissible_ends(bits, T, k, p, q)
    out = [set() for _ in us]
    for end in ends:
        keep = mask_of(cls, end, len(w))
        idx = np.flatnonzero(keep & (w > 0))
        C = np.cumsum(w[idx])
        Z, d = float(C[-1]), margin(w, t, keep)
        before = np.concatenate([[0.0], C[:-1]])
        for n, u in enumerate(us):
            x = clamp_u(u) * Z
            first, last = np.searchsorted(C + d, x, side="left"), np.searchsorted(before - d, x, side="right")
            out[n] |= set(idx[first:last].tolist())          # C(i) + d >= x and C(i - 1) - d <= x
    return out


def admissible(bits, u, T=1.0, k=None, p=None, q=None):
    return admissible_many(bits, [u], T, k, p, q)[0]


def eps_of(bits, T, k=None, p=None, q=None):
    """the bound of the docstring for one row: D(kept set) / Z"""
    cls, w, t, end_k, end_p, end_q, _ = prefix_ends(bits, T, k, p, q)
    keep = mask_of(cls, min(end_k, end_p, end_q), len(w))
    return margin(w, t, keep) / float(w[keep].sum())


# ---- inputs shared by the CPU and the GPU tests -----------------------------------------------------------------------------------------
def bf16_bits(x):
    """round-to-nearest-even bf16 bits of finite float32 values"""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


GAUSSIAN_ROWS = 64


def gaussian_case(vocab, rows, seed):
    """Gaussian logits of standard deviation 3 rounded to bf16, and per-row parameters that all differ within the call: rows 0 .. 3
    of every 8 without one filter each (None = off for the row: k 0, p 1, q 0), the others with all three"""
    rng = np.random.default_rng(seed)
    bits = bf16_bits(rng.standard_normal((rows, vocab)) * 3.0)
    r = np.arange(rows)
    par = dict(u=((r * 0.6180339887 + 0.05) % 1.0).astype(np.float32), T=(0.5 + 0.7 * r / rows).astype(np.float32),
               k=np.where(r % 8 == 0, 0, 5 + 3 * r).astype(np.int32), p=np.where(r % 8 == 1, 1.0, 0.55 + 0.4 * r / rows).astype(np.float32),
               q=np.where(r % 8 == 2, 0.0, 0.002 + 0.05 * r / rows).astype(np.float32))
    par["k"][r % 8 == 3] = vocab                             # off by being too large
    return bits, par


@functools.lru_cache(maxsize=None)
def gaussian_admissible(vocab):
    """the admissible set of every row of gaussian_case(vocab, GAUSSIAN_ROWS, vocab): computed once, shared by the tests, left unchanged"""
    bits, par = gaussian_case(vocab, GAUSSIAN_ROWS, vocab)
    return [admissible(bits[r], par["u"][r], par["T"][r], par["k"][r], par["p"][r], par["q"][r]) for r in range(GAUSSIAN_ROWS)]


STRATIFIED_ROWS = 4096


def stratified_case():
    """one 1 000-token row, to be repeated 4 096 times with u_r = (r + 0.5) / 4096; T = 1, top-k 300, top-p 0.98"""
    bits = bf16_bits(np.random.default_rng(77).standard_normal(1000) * 3.0)
    u = ((np.arange(STRATIFIED_ROWS) + 0.5) / STRATIFIED_ROWS).astype(np.float32)
    return bits, u, dict(T=1.0, k=300, p=0.98, q=None)


def long_row(vocab):
    bits = bf16_bits(np.random.default_rng(vocab).standard_normal(vocab) * 3.0)
    return bits, dict(u=0.37, T=0.8, k=64, p=0.9, q=0.01)


@functools.lru_cache(maxsize=None)
def stratified_admissible():
    bits, u, par = stratified_case()
    return admissible_many(bits, u.tolist(), par["T"], par["k"], par["p"], par["q"])
