"""The activation of mm_moe_activate_quantize (include/micromix_hip.h) on bf16 bit patterns, twice:

h_oracle          what the op is measured against: silu(a) = a / (1 + exp(-a)) in fp64 -> fp32 -> bf16 (to nearest even), times b in
                  fp32 (exact: two 8-bit significands) -> bf16.
h_device_formula  the device's arithmetic restated in fp32 numpy -- exp2 and a reciprocal, the two-range form of silu_mul_bf16
                  (csrc/mx_direct_convert.h), results of exp2 / reciprocal below 2^-126 flushed as v_exp_f32 / v_rcp_f32 flush them.
                  numpy's exp2 and divide are not the hardware's, so this says nothing about the device's bits: it is used on the CPU
                  only, to show that the budgets of tests/test_moe_activate_gpu.py are not broken by the arithmetic itself.

and the inputs and budgets those two test files share."""
from __future__ import annotations

import numpy as np

from oracle import mx_oracle as o

# budgets of h against h_oracle (the issue's): fewer than 1e-3 of the elements differ -- the project's budget for this device exp
# (tests/test_direct_quantize_gpu.py) -- and none by more than MAX_ULP bf16 ulps.  3 is derived, not measured: silu may land on the
# neighbouring bf16 -- 1 ulp, at most 2^-7 relative (a value at the bottom of its binade); the product with b then moves by at most 2^-7
# relative, which is at most 2 ulps where the product sits at the top of its binade (an ulp there is 2^-8 of it); the final rounding
# adds half an ulp on either side.  With b = 1 the product is silu itself: 1 ulp.
MAX_DIFFERING = 1e-3
MAX_ULP = 3


def h_oracle(a_bits, b_bits):
    a = o.bf16_to_f32(a_bits).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = (a / (1.0 + np.exp(-a))).astype(np.float32)
        return o.f32_to_bf16(o.bf16_to_f32(o.f32_to_bf16(s)) * o.bf16_to_f32(b_bits))


def _flush(x):
    return np.where(np.abs(x) < np.float32(2.0 ** -126), np.copysign(np.float32(0), x), x).astype(np.float32)


def h_device_formula(a_bits, b_bits):
    f = np.float32
    x = o.bf16_to_f32(a_bits)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        t = x * f(-1.4426950408889634)
        far = t > f(64.0)
        ex = _flush(np.exp2(_flush(np.where(far, t - f(64.0), t).astype(f))).astype(f))
        r = _flush((f(1.0) / _flush(np.where(far, ex, f(1.0) + ex).astype(f))).astype(f))
        s = (x * r).astype(f)
        s = np.where(far, s * f(2.0 ** -64), s).astype(f)
        return o.f32_to_bf16(o.bf16_to_f32(o.f32_to_bf16(s)) * o.bf16_to_f32(b_bits))


def draw_ab(rows, k, seed):
    """tests/test_direct_quantize_gpu.py::test_activate_quantize_close_to_oracle's choice: a = bf16 of 2 N(0, 1), b = make_inputs"""
    from conftest import make_inputs
    rng = np.random.default_rng(seed)
    a = o.f32_to_bf16((rng.standard_normal((rows, k)) * 2).astype(np.float32))
    return a, make_inputs(rng, rows, k)


# (rows, K, split, seed) of the budgeted comparison: shared by the CPU and the GPU test so that both see exactly the same inputs
BUDGET_CASES = [(37, 384, (128, 128, 128), 11), (130, 1024, (512, 128, 384), 12), (16, 14336, (12288, 1024, 1024), 13)]


def all_finite_bf16():
    """every finite bf16 value, as one [512, 128] matrix (the 65 280 finite patterns, then zeros)"""
    bits = np.arange(65536, dtype=np.uint16)
    fin = bits[np.isfinite(o.bf16_to_f32(bits))]
    out = np.zeros(512 * 128, dtype=np.uint16)
    out[: fin.size] = fin
    return out.reshape(512, 128)


def assert_within_budget(got_bits, want_bits, label, max_ulp=MAX_ULP, max_differing=MAX_DIFFERING):
    ulp = o.bf16_ulp_distance(got_bits, want_bits)
    differing, worst = float((ulp != 0).mean()), int(ulp.max())
    print(f"{label}: {differing:.2e} of the elements differ, at most {worst} bf16 ulp")
    assert differing < max_differing, f"{label}: {differing:.2e} of the elements differ from the oracle (budget {max_differing:.0e})"
    assert worst <= max_ulp, f"{label}: an element is {worst} bf16 ulps off (budget {max_ulp})"
