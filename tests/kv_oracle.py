"""Numpy oracle of the paged KV cache (include/micromix_hip.h, mm_kv_append / mm_paged_decode).

quantize_row   the int4 rule: quantize_int_group(x, 4, 128) (model/qLlamaLayer.py:13-23) in fp32 with fp16 (scale, zero), round half
               to even throughout, correctly rounded fp32 divides, fp16 conversions saturating at +-65504; a `zero` parameter of
               value 0 (rows with min >= -s / 2, where base = clamp(rint(-min / s)) can come out as -0.0) is +0.0
append         the bytes mm_kv_append writes into a host copy of the cache (FlashInfer paged layout, page.cuh:75-103,180-188)
attention      fp64 single-token GQA attention over the dequantized cache of one layer
"""
from __future__ import annotations

import numpy as np

HD = 128


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def _f16(x):
    return np.clip(np.asarray(x, dtype=np.float32), -65504.0, 65504.0).astype(np.float16)


def quantize_row(x):
    """x float32 [..., 128] (bf16 values) -> (codes uint8 [..., 128], scale fp16 [...], zero fp16 [...])"""
    x = np.asarray(x, dtype=np.float32)
    mn, mx = x.min(-1), x.max(-1)
    s = _f16(np.maximum(mx - mn, np.float32(1e-5)) / np.float32(15.0))
    sf = s.astype(np.float32)
    base = np.clip(np.rint(-mn / sf), 0, 15).astype(np.float32)
    codes = np.clip(np.rint(x / sf[..., None]) + base[..., None], 0, 15).astype(np.uint8)
    zero = np.abs(_f16(base * sf))                     # base * s >= 0; a zero is stored as +0.0, never -0.0
    return codes, s, zero


def pack_codes(codes):
    """[..., 128] codes -> [..., 64] bytes, element 2j in the low nibble of byte j"""
    return (codes[..., 0::2] | (codes[..., 1::2] << 4)).astype(np.uint8)


def unpack_codes(packed):
    out = np.empty(packed.shape[:-1] + (HD,), dtype=np.uint8)
    out[..., 0::2] = packed & 15
    out[..., 1::2] = packed >> 4
    return out


def seq_lens(kv_indptr, last_page_len, P):
    n = np.diff(np.asarray(kv_indptr))
    return np.where(n > 0, (n - 1) * P + np.asarray(last_page_len), 0)


def slots(kv_indptr, kv_indices, P, b, positions):
    """(page, slot) of sequence b's token positions"""
    pos = np.asarray(positions)
    return np.asarray(kv_indices)[kv_indptr[b] + pos // P], pos % P


def append(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, k, v, append_indptr, layer):
    """apply mm_kv_append to host copies (kv_data uint8 [..., 64] + kv_param float16, or kv_data uint16 bf16 bits [..., 128] with
    kv_param None); k, v uint16 bf16 bits [T, Hkv, 128]"""
    P = kv_data.shape[4]
    lens = seq_lens(kv_indptr, last_page_len, P)
    for b in range(len(last_page_len)):
        a0, a1 = append_indptr[b], append_indptr[b + 1]
        if a1 == a0:
            continue
        pages, sl = slots(kv_indptr, kv_indices, P, b, np.arange(lens[b] - (a1 - a0), lens[b]))
        for which, src in ((0, k), (1, v)):
            rows = src[a0:a1]                                         # [n, Hkv, 128]
            if kv_param is None:
                kv_data[pages, layer, which, :, sl] = rows
            else:
                codes, s, z = quantize_row(bf16_to_f32(rows))
                kv_data[pages, layer, which, :, sl] = pack_codes(codes)
                kv_param[pages, layer, which, :, sl, 0] = s
                kv_param[pages, layer, which, :, sl, 1] = z


def dequantized(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer, b):
    """(K, V) float64 [Hkv, len, 128] of sequence b as the cache holds them"""
    P = kv_data.shape[4]
    n = int(seq_lens(kv_indptr, last_page_len, P)[b])
    pages, sl = slots(kv_indptr, kv_indices, P, b, np.arange(n))
    out = []
    for which in (0, 1):
        rows = kv_data[pages, layer, which, :, sl]                    # [n, Hkv, ...]
        if kv_param is None:
            val = bf16_to_f32(rows).astype(np.float64)
        else:
            prm = kv_param[pages, layer, which, :, sl].astype(np.float64)   # [n, Hkv, 2]
            val = unpack_codes(rows).astype(np.float64) * prm[..., 0:1] - prm[..., 1:2]
        out.append(val.transpose(1, 0, 2))
    return out


def attention(q_bits, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer, sm_scale=None):
    """fp64 decode attention: q uint16 bf16 bits [B, Hq, 128] -> float64 [B, Hq, 128]"""
    q = bf16_to_f32(q_bits).astype(np.float64)
    B, Hq, _ = q.shape
    Hkv = kv_data.shape[3]
    g = Hq // Hkv
    scale = HD ** -0.5 if sm_scale is None else sm_scale
    o = np.zeros((B, Hq, HD))
    for b in range(B):
        K, V = dequantized(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer, b)
        if K.shape[1] == 0:
            continue
        Kr, Vr = np.repeat(K, g, axis=0), np.repeat(V, g, axis=0)    # HF repeat_kv
        s = np.einsum("hd,htd->ht", q[b], Kr) * scale
        p = np.exp(s - s.max(-1, keepdims=True))
        o[b] = np.einsum("ht,htd->hd", p / p.sum(-1, keepdims=True), Vr)
    return o
