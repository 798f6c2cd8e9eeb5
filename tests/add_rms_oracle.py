"""The residual add in front of the norm, restated in numpy on uint16 bf16 bit patterns (mm_add_rmsnorm_quantize, include/micromix_hip.h):

    s[i] = bf16_rne(f32(x[i]) + f32(r[i]))

one IEEE fp32 add of the two widened values -- numpy's float32 add: exact up to its single rounding, subnormals kept, inf - inf and
every NaN operand a NaN -- and one rounding to nearest even on the bit pattern; every NaN result is the one pattern 0x7FC0
(torch's own NaN pattern is not one: 0x7FC0 from its scalar conversion, 0xFFFF from its vectorised CPU one).  Everything behind s is `oracle.mx_oracle.rmsnorm_quantize(s, ...)`: the stated expectation for the six buffers."""
import numpy as np

from oracle import mx_oracle as o

CANONICAL_NAN = 0x7FC0


def add_bf16(x_bits, r_bits):
    x = (np.asarray(x_bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)
    r = (np.asarray(r_bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        f = (x + r).astype(np.float32)
    u = f.view(np.uint32)
    rounded = ((u + np.uint32(0x7FFF) + ((u >> 16) & np.uint32(1))) >> 16).astype(np.uint16)
    return np.where(np.isnan(f), np.uint16(CANONICAL_NAN), rounded).astype(np.uint16)


def add_rmsnorm_quantize(x_bits, r_bits, w_bits, eps, idx, kn, ks, ko, integer_round=True):
    """(s, the six buffers of rmsnorm_quantize on s)"""
    s = add_bf16(x_bits, r_bits)
    return s, o.rmsnorm_quantize(s, w_bits, eps, idx, kn, ks, ko, integer_round=integer_round)


def all_finite_bf16():
    b = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    return b[(b & 0x7F80) != 0x7F80]


def partners(b):
    """for every finite bf16 pattern b: the handful of partners the add rule is checked against"""
    f = (b.astype(np.uint32) << 16).view(np.float32)
    def scaled(p):
        with np.errstate(under="ignore"):
            return o.f32_to_bf16((f * np.float32(2.0 ** -p)).astype(np.float32))
    big = np.full_like(b, 0x7F7F)
    return {"+0": np.zeros_like(b), "-0": np.full_like(b, 0x8000), "negation": b ^ np.uint16(0x8000), "2^-8 of it": scaled(8),
            "2^-17 of it": scaled(17), "largest finite, same sign": big | (b & np.uint16(0x8000)), "largest finite": big,
            "smallest subnormal": np.full_like(b, 0x0001), "largest subnormal, negative": np.full_like(b, 0x807F)}
