"""Numpy float32 oracle of QK-norm (include/micromix_qknorm.h, steps 1 to 4; step 5 is tests/rope_oracle.py's rope): HF's Qwen3RMSNorm
of one 128-element bf16 row, on bf16 bit patterns, with the sum of squares in the header's one tree."""
from __future__ import annotations

import numpy as np

import kv_oracle as ko
import rope_oracle as ro

TREE = (0, 1, 2, 3, 5, 4)          # partners whose index differs in this bit are added, in this order
NATURAL = (0, 1, 2, 3, 4, 5)       # another tree; "linear": left to right.  Both only to show that inputs tell the orders apart


def sum_squares(x_bits, order=TREE):
    """x uint16 [.., 128] -> S float32 [..]"""
    x = ko.bf16_to_f32(x_bits)
    p = x[..., 0::2] * x[..., 0::2] + x[..., 1::2] * x[..., 1::2]      # fp32: the squares are exact, the sum is one rounding
    if order == "linear":
        s = p[..., 0].copy()
        for l in range(1, 64):
            s = s + p[..., l]
        return s
    idx = np.arange(64)
    for bit in order:
        p = p + p[..., idx ^ (1 << bit)]                              # a butterfly: every index ends with the tree's sum
    return p[..., 0]


def qknorm(x_bits, w_bits, eps, order=TREE):
    """x uint16 [.., 128], w uint16 [128] -> y uint16 [.., 128]"""
    r = np.float32(1.0) / np.sqrt(sum_squares(x_bits, order) * np.float32(2.0 ** -7) + np.float32(eps))
    n = ro.f32_to_bf16(ko.bf16_to_f32(x_bits) * r[..., None])
    return ro.f32_to_bf16(ko.bf16_to_f32(w_bits) * ko.bf16_to_f32(n))


def gaussian_case(seed=5, T=1024, Hq=32, Hkv=2):
    """the fixed-seed N(0, 2^2) input of the GPU tests that is large enough to tell the tree from other orders (tests/test_qknorm_cpu.py
    asserts it): q, k, v bits [T, H, 128], the two weights [128] near 1, eps"""
    rng = np.random.default_rng(seed)
    q, k, v = (ro.f32_to_bf16(rng.standard_normal((T, H, 128)).astype(np.float32) * np.float32(2.0)) for H in (Hq, Hkv, Hkv))
    qw, kw = (ro.f32_to_bf16(1.0 + 0.25 * rng.standard_normal(128).astype(np.float32)) for _ in range(2))
    return q, k, v, qw, kw, 1e-6
