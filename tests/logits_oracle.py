"""The rule of mm_process_logits (include/micromix_logits.h) in numpy float32, one operation per line: the only source of expected
values of tests/test_logits_cpu.py and tests/test_logits_gpu.py.  Every fp32 operation of numpy on float32 scalars and arrays is the
correctly rounded IEEE one with subnormals kept, and none is fused with another, so the kernel's bits must equal these bits.

bf16 is carried as uint16 bit patterns; the conversions are integer programs (bf16_to_f32, f32_to_bf16: round to nearest even, every
NaN 0x7FC0)."""
import numpy as np

NAN_BITS, NINF_BITS = 0x7FC0, 0xFF80
F32 = np.float32


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16(x):
    """round to nearest even on the integer bits; every NaN becomes 0x7FC0; overflow goes to inf"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(NAN_BITS), r)


def history(tokens, s, prompt_len, total_len, vocab):
    """(seen [vocab] bool, c [vocab] int64) of sequence s under a row's lengths; tokens [n_seq, ld_tok] int32 or None"""
    seen, c = np.zeros(vocab, dtype=bool), np.zeros(vocab, dtype=np.int64)
    if tokens is None or not 0 <= s < tokens.shape[0]:
        return seen, c
    ld_tok = tokens.shape[1]
    P = min(max(int(prompt_len), 0), ld_tok)
    N = min(max(int(total_len), P), ld_tok)
    ids = tokens[s, :N].astype(np.int64)
    inside = (ids >= 0) & (ids < vocab)
    seen[ids[inside]] = True
    out = ids[P:][inside[P:]]
    np.add.at(c, out, 1)
    return seen, c


def row(bits, *, tokens=None, s=0, prompt_len=0, total_len=0, theta=None, alpha_f=None, alpha_p=None, bias_idx=None, bias_val=None,
        mask_words=None):
    """out bits [vocab] of one row of bf16 bits [vocab]; None is a null array"""
    with np.errstate(all="ignore"):
        vocab = len(bits)
        x = bf16_to_f32(bits).copy()
        seen, c = history(tokens, s, prompt_len, total_len, vocab)
        # 1 repetition
        if tokens is not None and theta is not None:
            theta = F32(theta)
            if np.isfinite(theta) and theta > 0:
                mul = x * theta
                div = x / theta
                x = np.where(seen, np.where(x < 0, mul, div), x).astype(np.float32)
        # 2 frequency, then presence
        hit = c > 0
        if tokens is not None and alpha_f is not None and not np.isnan(F32(alpha_f)):
            fc = c.astype(np.float32)                                               # exact: c <= 2^24
            prod = F32(alpha_f) * fc
            diff = x - prod
            x = np.where(hit, diff, x).astype(np.float32)
        if tokens is not None and alpha_p is not None and not np.isnan(F32(alpha_p)):
            diff = x - F32(alpha_p)
            x = np.where(hit, diff, x).astype(np.float32)
        # 3 bias: the highest j wins
        if bias_idx is not None:
            winner = {}
            for j, i in enumerate(np.asarray(bias_idx).tolist()):
                if 0 <= i < vocab:
                    winner[i] = j
            for i, j in winner.items():
                x[i] = x[i] + F32(bias_val[j])
        # 4 mask
        if mask_words is not None:
            w = np.asarray(mask_words, dtype=np.int32).view(np.uint32)
            i = np.arange(vocab)
            allowed = (w[i >> 5] >> (i & 31).astype(np.uint32)) & np.uint32(1)
            x = np.where(allowed == 1, x, F32(-np.inf)).astype(np.float32)
        # 5 output
        return f32_to_bf16(x)


def rows(bits, *, tokens=None, row_seq=None, prompt_len=None, total_len=None, theta=None, alpha_f=None, alpha_p=None, bias_idx=None,
         bias_val=None, mask=None):
    """out bits [rows, vocab] of bits [rows, vocab]; every parameter as the C entry takes it (per-row arrays, or None)"""
    at = lambda a, r: None if a is None else a[r]
    return np.stack([row(bits[r], tokens=tokens, s=r if row_seq is None else int(row_seq[r]), prompt_len=0 if tokens is None else prompt_len[r],
                         total_len=0 if tokens is None else total_len[r], theta=at(theta, r), alpha_f=at(alpha_f, r), alpha_p=at(alpha_p, r),
                         bias_idx=at(bias_idx, r), bias_val=at(bias_val, r), mask_words=at(mask, r)) for r in range(bits.shape[0])])


# ---- planted rounding cases ------------------------------------------------------------------------------------------------------------
# the two places where an implementation that is not the rule still agrees on almost every input: a divide that is one fp32 ulp off (a
# reciprocal and a multiply), and x - a c as one fma.  Both show after the bf16 rounding only where the fp32 result sits next to a bf16
# rounding boundary, so such inputs are searched for, with a fixed seed, among DRAWS random ones.
DRAWS, SEED = 1 << 24, 20250


def _draws():
    rng = np.random.default_rng(SEED)
    x = bf16_to_f32(f32_to_bf16((rng.standard_normal(DRAWS) * 8.0).astype(np.float32)))
    return rng, x


_cache = {}


def division_cases():
    """(x bits, theta) where fl32(x / theta) moved by one fp32 ulp either way rounds to another bf16 (x > 0, so the rule divides)"""
    if "div" not in _cache:
        rng, x = _draws()
        x = np.abs(x) + F32(0.0)
        theta = (F32(1.0) + rng.random(DRAWS, dtype=np.float32) * F32(1.5)).astype(np.float32)
        keep = x > 0
        x, theta = x[keep], theta[keep]
        q = x / theta
        up, down = np.nextafter(q, F32(np.inf)), np.nextafter(q, F32(-np.inf))
        b = f32_to_bf16(q)
        hit = (f32_to_bf16(up) != b) | (f32_to_bf16(down) != b)
        _cache["div"] = (f32_to_bf16(x[hit]), theta[hit])
    return _cache["div"]


def fma_cases():
    """(x bits, alpha_f, c) where x - alpha_f c with one rounding gives another bf16 than with the rule's two"""
    if "fma" not in _cache:
        rng, x = _draws()
        alpha = (rng.random(DRAWS, dtype=np.float32) * F32(2.0)).astype(np.float32)
        c = rng.integers(1, 64, DRAWS)
        two = x - alpha * c.astype(np.float32)
        one = (x.astype(np.float64) - alpha.astype(np.float64) * c).astype(np.float32)   # the product and the difference are exact in fp64
        hit = f32_to_bf16(two) != f32_to_bf16(one)
        _cache["fma"] = (f32_to_bf16(x[hit]), alpha[hit], c[hit].astype(np.int32))
    return _cache["fma"]
