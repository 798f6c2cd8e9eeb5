"""Numpy oracle of the fp8 (e4m3) kind of the paged KV cache (include/micromix_hip.h, MM_KV_FP8_E4M3), on top of the element codec of
oracle/mx_oracle.py and the page walk of tests/kv_oracle.py.

row_exponent      e of a row by the DEFINITION: the smallest integer in [-14, 15] with amax <= 448 * 2^e (a search in fp64)
row_exponent_bits the same from the bf16 bits of amax, as the kernels do: clamp(E - 135 + (M > 96), -14, 15)
quantize_row      (codes, e): code = e4m3fn(RNE(clamp(x * 2^-e, -448, 448))), the clamp first
param_pair        the fp16 (scale, zero) = (2^e, +0.0) of a row
append            the bytes mm_kv_append writes into host copies of an fp8 cache
dequantize        decode(code) * scale - zero of a whole cache as bf16 bits (every value is exactly a bf16 number)
"""
from __future__ import annotations

import numpy as np

import kv_oracle as ko
from oracle import mx_oracle as mo

HD = 128
E_MIN, E_MAX = -14, 15
FMAX = 448.0


def row_exponent(x):
    """x float [..., 128] -> int64 [...]: by the definition, no bit tricks"""
    amax = np.abs(np.asarray(x, dtype=np.float64)).max(-1)
    e = np.full(amax.shape, E_MAX, dtype=np.int64)
    for cand in range(E_MAX - 1, E_MIN - 1, -1):
        e = np.where(amax <= FMAX * 2.0 ** cand, cand, e)
    return e


def row_exponent_bits(x_bits):
    """x uint16 bf16 bits [..., 128] -> int64 [...]: from the exponent field E and the mantissa M of amax"""
    mag = (np.asarray(x_bits, dtype=np.uint16) & 0x7FFF).max(-1).astype(np.int64)      # bf16 magnitudes order as their bits do
    return np.clip((mag >> 7) - 135 + ((mag & 127) > 96), E_MIN, E_MAX)


def quantize_row(x_bits):
    """x uint16 bf16 bits [..., 128] (finite) -> (codes uint8 [..., 128], e int64 [...])"""
    x = ko.bf16_to_f32(x_bits)
    e = row_exponent(x)
    scaled = x.astype(np.float64) * 2.0 ** (-e[..., None].astype(np.float64))          # exact: |x| 2^-e < 2^143 has 8 significant bits
    # np.clip keeps -0.0.  The cast is exact from 2^-126 up; below, whatever it leaves is far under half the smallest e4m3
    # subnormal (2^-10) and encodes to a signed zero either way
    clamped = np.clip(scaled, -FMAX, FMAX).astype(np.float32)
    return mo.encode(clamped, "fp8"), e


def param_pair(e):
    """e int [...] -> float16 [..., 2] = (2^e, +0.0)"""
    out = np.zeros(np.shape(e) + (2,), dtype=np.float16)
    out[..., 0] = (2.0 ** np.asarray(e, dtype=np.float64)).astype(np.float16)
    return out


def append(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, k, v, append_indptr, layer):
    """apply mm_kv_append to host copies of an fp8 cache (kv_data uint8 [..., 128], kv_param float16 [..., 2]); k, v uint16 bf16 bits
    [T, Hkv, 128].  A token whose page entry lies outside [0, max_pages) writes nothing."""
    P, max_pages = kv_data.shape[4], kv_data.shape[0]
    lens = ko.seq_lens(kv_indptr, last_page_len, P)
    for b in range(len(last_page_len)):
        a0, a1 = int(append_indptr[b]), int(append_indptr[b + 1])
        if a1 == a0:
            continue
        pages, sl = ko.slots(kv_indptr, kv_indices, P, b, np.arange(lens[b] - (a1 - a0), lens[b]))
        ok = (pages >= 0) & (pages < max_pages)
        for which, src in ((0, k), (1, v)):
            codes, e = quantize_row(src[a0:a1][ok])                    # [n, Hkv, 128], [n, Hkv]
            kv_data[pages[ok], layer, which, :, sl[ok]] = codes
            kv_param[pages[ok], layer, which, :, sl[ok]] = param_pair(e)


def dequantize(kv_data, kv_param):
    """the cache's values decode(code) * scale - zero as bf16 bits, uint16, shape of kv_data; each is exactly a bf16 number (asserted
    for the finite ones; a poisoned slot -- NaN code or NaN params -- comes out as the bf16 NaN 0x7FC0)"""
    prm = kv_param.astype(np.float64)
    val = mo.decode(kv_data, "fp8").astype(np.float64) * prm[..., 0:1] - prm[..., 1:2]
    fin = np.isfinite(val)
    f32 = np.where(fin, val, 0.0).astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), np.where(fin, val, 0.0)), "a dequantized value is not a float32"
    u = f32.view(np.uint32)
    assert not (u & 0xFFFF).any(), "a dequantized value is not a bf16 number"
    return np.where(fin, (u >> 16).astype(np.uint16), np.uint16(0x7FC0)).astype(np.uint16)
