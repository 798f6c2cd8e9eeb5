"""CPU tests of mm_moe_activate_quantize (include/micromix_hip.h): its status codes, which come without device work, and the budgets of
tests/test_moe_activate_gpu.py held by the device formula restated in fp32 numpy (tests/moe_act_oracle.py) on exactly the inputs the
GPU test draws -- the budgets are not so tight that the arithmetic alone breaks them."""
import numpy as np
import pytest

import moe_act_oracle as ma
from micromix_amd import _lib
from oracle import mx_oracle as o


def test_moe_activate_quantize_status_codes_without_device_work():
    lib = _lib.load()
    z, p = None, 16                                           # p: a non-null, 16-byte aligned pointer that is never dereferenced here
    assert lib.mm_version() >= 650
    S, U, B, OK = _lib.MM_ERR_BAD_SPLIT, _lib.MM_ERR_UNSUPPORTED, _lib.MM_ERR_BAD_ARG, _lib.MM_OK
    act = lambda a=p, b=p, off=p, tab=p, E=8, n=16, K=256, split=(128, 0, 128), o3=(p, p, p), sf3=(p, p, p), h=z: \
        lib.mm_moe_activate_quantize(a, b, off, tab, E, n, K, *split, *o3, *sf3, h, z)
    for E in (0, 65, 1000):                                   # E outside [1, 64]
        assert act(E=E) == U, E
    assert act(E=-1) == B and act(n=-1) == B and act(K=-256) == B                                  # negative sizes
    assert act(split=(128, 0, 64)) == S and act(split=(128, 128, 128)) == S and act(K=0, split=(0, 0, 0)) == S
    assert act(K=32768 + 128, split=(32768, 0, 128)) == B     # a row longer than the quantizer stages
    # n = 0: MM_OK, whatever the pointers
    assert act(a=z, b=z, off=z, tab=z, n=0, o3=(z, z, z), sf3=(z, z, z)) == OK
    # null pointers: h_out alone may be null -- not tried here, it would launch
    assert act(a=z) == B and act(b=z) == B and act(off=z) == B and act(tab=z) == B
    assert act(o3=(z, p, p)) == B and act(o3=(p, p, z)) == B and act(sf3=(z, p, p)) == B and act(sf3=(p, p, z)) == B
    # misaligned: bf16 rows and packed rows move as 16-byte pieces, scales as dwords, the table holds 8-byte addresses
    assert act(a=8) == B and act(b=24) == B and act(h=8) == B and act(h=2) == B
    assert act(o3=(8, p, p)) == B and act(o3=(p, p, 24)) == B and act(sf3=(2, p, p)) == B and act(tab=12) == B
    assert "mm_moe_activate_quantize" in _lib.EXPORTS


@pytest.mark.parametrize("rows,k,split,seed", ma.BUDGET_CASES)
def test_the_formula_alone_stays_inside_the_budgets(rows, k, split, seed):
    a, b = ma.draw_ab(rows, k, seed)
    ma.assert_within_budget(ma.h_device_formula(a, b), ma.h_oracle(a, b), f"{rows} x {k}")


def test_the_formula_alone_is_within_one_ulp_on_every_finite_bf16():
    a = ma.all_finite_bf16()
    b = np.full_like(a, 0x3F80)
    got, want = ma.h_device_formula(a, b), ma.h_oracle(a, b)
    assert np.isfinite(o.bf16_to_f32(want)).all()
    ma.assert_within_budget(got, want, "every finite bf16, b = 1", max_ulp=1, max_differing=1.0)
    assert ((got & 0x7FFF) == 0)[(want & 0x7FFF) == 0].all()
    # the range the two-range form exists for: silu(a) is a nonzero bf16 although 2^(a log2 e) is below every normal fp32
    x = o.bf16_to_f32(a)
    deep = (x < -88.0) & ((want & 0x7FFF) != 0)
    assert deep.sum() >= 8 and ((got & 0x7FFF) != 0)[deep].all()


def test_three_ulps_are_reached_by_the_derivation_not_exceeded():
    """the 3-ulp bound on every pair (silu one bf16 ulp off, b): exhaustive over silu values in one binade and 256 significands of b"""
    s = np.arange(0x3F80, 0x4000, dtype=np.uint16)             # [1, 2)
    bb = np.arange(0x3F80, 0x4000, dtype=np.uint16)
    S, Bv = np.meshgrid(s, bb, indexing="ij")
    prod = lambda sb: o.f32_to_bf16(o.bf16_to_f32(sb) * o.bf16_to_f32(Bv))
    d = np.maximum(o.bf16_ulp_distance(prod(S), prod(S + np.uint16(1))), o.bf16_ulp_distance(prod(S), prod(S - np.uint16(1))))
    assert int(d.max()) <= ma.MAX_ULP
