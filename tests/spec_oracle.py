"""The rule of mm_spec_sample_rows (include/micromix_spec.h) in Python integers: the only source of expected values of
tests/test_spec_sample_cpu.py and tests/test_spec_sample_gpu.py.  Nothing here shares code with the kernels.

The masses come from tests/sample_oracle.py's weight model:
  exact rows     a row that holds one finite value m and -inf has weights exactly 1 and 0 on any hardware, so P_i = 2^43 on the kept
                 tokens and 0 elsewhere: masses(bits, ...) returns them as Python integers, and spec_sample() is then the whole rule,
                 bit for bit
  Gaussian rows  the device's weight of a token lies within sample_oracle.rel_error of the exact one (the 1-ulp V_EXP_F32), so a
                 comparison of the rule can fall either way only inside a band: admissible() returns, for one row, every decision and
                 every redrawn token a device within that bound may give

U24, mulshift, accept, residual     the integer pieces, as the header states them
spec_sample(P, Q, x, ua, ur, ...)   (out, accepted) of one row from integer masses (Q None: one-hot)
chain_walk(...)                     the speculative-sampling algorithm over chains, as `verify_greedy` must report it
"""
import functools

import numpy as np

import sample_oracle as so

ONE = 1 << 43
CHUNK = 8192


# ---- the integer pieces -------------------------------------------------------------------------------------------------------------------
def U24(u):
    """trunc(u * 2^24) of u as mm_sample_rows reads it"""
    return int(so.clamp_u(u) * (1 << 24))


def mulshift(z, U):
    """floor(U * z / 2^24): Python integers have no width, so this is the definition and not the device's split form"""
    return (U * z) >> 24


def mulshift_split(z, U):
    """the form the header prescribes for 128-bit registers"""
    return (z >> 24) * U + (((z & ((1 << 24) - 1)) * U) >> 24)


def accept(Px, Zp, Qx, Zq, Ua):
    return mulshift(Qx * Zp, Ua) < Px * Zq


def residual(P, Zp, Q, Zq):
    return [max(0, p * Zq - q * Zp) for p, q in zip(P, Q)]


def first_past(masses, want):
    """the first index whose inclusive prefix sum exceeds `want`"""
    run = 0
    for i, m in enumerate(masses):
        run += m
        if run > want:
            return i
    raise AssertionError("want is not below the total mass")


def spec_sample(P, Q, x, ua, ur, *, fallback=None):
    """(out, accepted) of a row that is not greedy, from its integer masses P (target) and Q (draft; None: one-hot at x).
    x None or outside the row: no candidate, mm_sample_rows' draw from P"""
    Zp = sum(P)
    if x is None or not 0 <= x < len(P):
        want = min(int(float(so.clamp_u(ur)) * float(Zp)), Zp - 1)               # mm_sample_rows' fp64 place
        return first_past(P, want), -1
    Qx, Zq = (1, 1) if Q is None else (Q[x], sum(Q))
    if accept(P[x], Zp, Qx, Zq, U24(ua)):
        return x, 1
    # R_i > 0 needs P_i > 0: the prefix sums are walked over the target's support alone
    support = [i for i, v in enumerate(P) if v > 0]
    R = residual([P[i] for i in support], Zp, [int(i == x) if Q is None else Q[i] for i in support], Zq)
    ZR = sum(R)
    if ZR == 0:
        return fallback, 0
    return support[first_past(R, mulshift(ZR, U24(ur)))], 0


_MASSES = {}


def masses(bits, T=1.0, k=None, p=None, q=None):
    """the integer masses of a row whose weights are exactly 0 and 1 (asserted), as a list of Python integers that callers leave
    unchanged (one per distinct row and parameters is kept); None for a greedy row"""
    if so.is_greedy(bits, T):
        return None
    key = (np.asarray(bits, dtype=np.uint16).tobytes(), float(T), k, p, q)
    if key not in _MASSES:
        w, _ = so.weights(bits, T)
        assert set(np.unique(w).tolist()) <= {0.0, 1.0}, "not an exact row: use admissible()"
        keep = so.kept_mask(bits, T, k, p, q)
        _MASSES[key] = [ONE if keep[i] and w[i] == 1.0 else 0 for i in range(len(w))]
    return _MASSES[key]


def spec_row(bits, draft_bits, x, ua, ur, T=1.0, k=None, p=None, q=None):
    """(out, accepted) of one row of exact bits: every case of the header"""
    valid = x is not None and 0 <= x < len(bits)
    if so.is_greedy(bits, T):
        best = so.argmax(bits)
        return best, (int(best == x) if valid else -1)
    P = masses(bits, T, k, p, q)
    Q = None if draft_bits is None or not valid or so.is_greedy(draft_bits, T) else masses(draft_bits, T, k, p, q)
    return spec_sample(P, Q, x if valid else None, ua, ur, fallback=so.argmax(bits))


# ---- chains -----------------------------------------------------------------------------------------------------------------------------------
def chain_candidates(draft_tok, qo_indptr):
    cand = [-1] * len(draft_tok)
    for b in range(len(qo_indptr) - 1):
        for t in range(qo_indptr[b], qo_indptr[b + 1] - 1):
            cand[t] = int(draft_tok[t + 1])
    return cand


def chain_walk(row_result, draft_tok, root_tok, qo_indptr):
    """[(k, bonus)] per sequence: the speculative-sampling algorithm over a chain.  row_result(t, x) -> (token, accepted) of row t with
    candidate x (None on a leaf).  A sequence whose first draft token is not the root token keeps nothing and its bonus is the root
    token; root < 0 marks a prompt chunk: all n rows kept, the bonus the plain sample of the last row (-1 for n = 0)"""
    out = []
    for b in range(len(qo_indptr) - 1):
        lo, hi = qo_indptr[b], qo_indptr[b + 1]
        n, root = hi - lo, int(root_tok[b])
        if root < 0:
            out.append((n, row_result(hi - 1, None)[0] if n else -1))
            continue
        if n == 0 or int(draft_tok[lo]) != root:
            out.append((0, root))
            continue
        k = 0
        while True:
            t = lo + k
            k += 1
            leaf = t == hi - 1
            tok, acc = row_result(t, None if leaf else int(draft_tok[t + 1]))
            if leaf or acc != 1:
                out.append((k, tok))
                break
    return out


# ---- the exact family -------------------------------------------------------------------------------------------------------------------------
M_BITS = 0x3FC0        # 1.5
NEG_INF = 0xFF80


def edge_columns(vocab):
    """columns on both sides of every part edge and of 16-byte edges, the row's ends, and a few inside; at least 14 for vocab >= 64"""
    cols = []
    for e in range(CHUNK, vocab, CHUNK):
        cols += [e - 1, e]
    cols += [0, vocab - 1, 7, 8, vocab - 8, vocab - 9, 15, 16, CHUNK - 8, CHUNK - 9, CHUNK + 7, CHUNK + 8, 33, 1000, 4097, vocab // 2, 5, 250]
    seen = []
    for c in cols:
        if 0 <= c < vocab and c not in seen:
            seen.append(c)
    return seen


def exact_sets(vocab, a, b, shared=2):
    """(A, B): a target and a draft support of a and b columns with `shared` in common, taken from edge_columns in turn so that both
    lie on both sides of the edges"""
    cols = edge_columns(vocab)
    assert len(cols) >= a + b - shared
    both, rest = cols[:shared], cols[shared:a + b - shared]
    only_a, only_b = [], []
    for c in rest:                                           # alternately, until one of the two is full
        to_a = len(only_b) == b - shared or (len(only_a) < a - shared and len(only_a) <= len(only_b))
        (only_a if to_a else only_b).append(c)
    assert len(only_a) == a - shared and len(only_b) == b - shared
    return sorted(both + only_a), sorted(both + only_b)


def uniform_row(vocab, cols):
    bits = np.full(vocab, NEG_INF, dtype=np.uint16)
    bits[list(cols)] = M_BITS
    return bits


# ---- Gaussian rows: what a device within the bound may answer -----------------------------------------------------------------------------------
def _sides(bits, T, k, p, q):
    """for every admissible kept set of a row: (keep mask, w, e) with e the per-token absolute error of a kept mass / 2^43"""
    ends, (cls, w, t, *_rest) = so.admissible_ends(bits, T, k, p, q)
    err = w * so.rel_error(t) + 2.0 ** -43
    return [(so.mask_of(cls, end, len(w)), w, err) for end in ends]


def admissible(bits, draft_bits, x, ua, ur, T=1.0, k=None, p=None, q=None):
    """(decisions, tokens, kept): the set of `accepted` values and the set of out_idx values a device within sample_oracle's bound may
    return for a row that is not greedy on either side and has a candidate; kept: the union of the target's admissible kept sets.
    With exact masses p_i, q_i (weights of kept tokens) and their sums, the device holds p_i (1 +- e_i) - [0, 2^-43) and sums within
    E = sum of those: the accept test compares U' q_x z_p with p_x z_q, U' = U / 2^24 exact, so it is decided unless the intervals of
    the two sides meet.  A prefix sum of the residual max(0, p_i z_q - q_i z_p) moves by at most the sum of its terms' errors (max(0, .)
    is 1-Lipschitz), D in all, and so does the place U' ZR: token i can be the redraw when U' ZR lies within 2 D (1 + 2^-10) of its
    interval of the exact prefix sums and its residual can be positive; x itself never is (R_x = 0 on a rejected row, exactly)."""
    Ua, Ur = U24(ua) / 2.0 ** 24, U24(ur) / 2.0 ** 24
    decisions, tokens, kept = set(), set(), np.zeros(len(bits), dtype=bool)
    for keep_p, wp, ep in _sides(bits, T, k, p, q):
        kept |= keep_p & (wp > 0)
        for keep_q, wq, eq in _sides(draft_bits, T, k, p, q):
            pm, qm = np.where(keep_p, wp, 0.0), np.where(keep_q, wq, 0.0)
            dp, dq = np.where(keep_p, ep, 0.0), np.where(keep_q, eq, 0.0)
            zp, zq, Ep, Eq = pm.sum(), qm.sum(), dp.sum(), dq.sum()
            lo = lambda v, d: max(v - d, 0.0) * (1 - 2.0 ** -40)
            hi = lambda v, d: (v + d) * (1 + 2.0 ** -40)
            lhs = (Ua * lo(qm[x], dq[x]) * lo(zp, Ep), Ua * hi(qm[x], dq[x]) * hi(zp, Ep))
            rhs = (lo(pm[x], dp[x]) * lo(zq, Eq), hi(pm[x], dp[x]) * hi(zq, Eq))
            if pm[x] == 0:                                    # x is not kept by the target: P_x = 0 exactly, always rejected
                may_accept, may_reject = False, True
            elif qm[x] == 0:                                  # ... not kept by the draft: Q_x = 0 < P_x, always accepted
                may_accept, may_reject = True, False
            else:
                may_accept, may_reject = lhs[0] < rhs[1], lhs[1] >= rhs[0]
            if may_accept:
                decisions.add(1)
                tokens.add(x)
            if may_reject:
                decisions.add(0)
                r = np.maximum(pm * zq - qm * zp, 0.0)
                d = (dp * zq + pm * Eq + dq * zp + qm * Ep) * (1 + 2.0 ** -10)
                idx = np.flatnonzero(keep_p & (r + d > 0) & (np.arange(len(bits)) != x))
                C = np.cumsum(r[idx])
                D = 2.0 * float(d.sum()) * (1 + 2.0 ** -10) + float(r.sum()) * 2.0 ** -40
                before = np.concatenate([[0.0], C[:-1]])
                place = Ur * float(r.sum())
                first, last = np.searchsorted(C + D, place, side="left"), np.searchsorted(before - D, place, side="right")
                tokens |= set(idx[first:last].tolist())
    return decisions, tokens, kept


GAUSSIAN_VOCAB, GAUSSIAN_ROWS, GAUSSIAN_SEED, GAUSSIAN_NOISE = 20000, 16, 20000, 0.75


def gaussian_case(filters):
    """16 rows of Gaussian target logits (standard deviation 3), the draft the target plus Gaussian noise, both rounded to bf16; every
    candidate drawn from the draft row by the rule of mm_sample_rows under the row's parameters, as a draft model would; per-row
    parameters that all differ.  filters False: temperature alone"""
    rng = np.random.default_rng(GAUSSIAN_SEED + int(filters))
    rows, vocab = GAUSSIAN_ROWS, GAUSSIAN_VOCAB
    target = rng.standard_normal((rows, vocab)) * 3.0
    bits = so.bf16_bits(target)
    draft = so.bf16_bits(target + rng.standard_normal((rows, vocab)) * GAUSSIAN_NOISE)
    r = np.arange(rows)
    par = dict(T=(0.6 + 0.6 * r / rows).astype(np.float32), ua=rng.random(rows).astype(np.float32), ur=rng.random(rows).astype(np.float32))
    if filters:
        par.update(k=(40 + 7 * r).astype(np.int32), p=(0.7 + 0.25 * r / rows).astype(np.float32), q=(0.001 + 0.01 * r / rows).astype(np.float32))
    else:
        par.update(k=None, p=None, q=None)
    ud = rng.random(rows)
    pick = lambda name, i: None if par[name] is None else par[name][i]
    cand = np.array([so.sample(draft[i], ud[i], par["T"][i], pick("k", i), pick("p", i), pick("q", i)) for i in range(rows)], dtype=np.int32)
    return bits, draft, cand, par


@functools.lru_cache(maxsize=None)
def gaussian_admissible(filters):
    """admissible() of every row of gaussian_case(filters): computed once, shared by the tests, left unchanged"""
    bits, draft, cand, par = gaussian_case(filters)
    pick = lambda name, i: None if par[name] is None else par[name][i]
    return [admissible(bits[i], draft[i], int(cand[i]), par["ua"][i], par["ur"][i], par["T"][i], pick("k", i), pick("p", i), pick("q", i))
            for i in range(GAUSSIAN_ROWS)]


def expected_acceptance(p, q):
    """(sum min(p, q), sum p q) of two distributions: what the speculative rule and exact matching keep of a draft token"""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    return float(np.minimum(p, q).sum()), float((p * q).sum())
