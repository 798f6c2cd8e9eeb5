"""Numpy oracle of mm_rope_kv_append (include/micromix_hip.h): HF's apply_rotary_pos_emb in bf16 tensor arithmetic on bf16 bit patterns,
then the cache bytes of tests/kv_oracle.py.

rope           y = bf16(bf16(x * cos) + bf16(rotate_half(x) * sin)), rotate_half(x) = cat(-x[64:], x[:64]); every op in fp32 (a product of
               two bf16 values is exact there), rounded to nearest even
rope_append    the rotated q, and mm_kv_append of (rope(k), v) applied to host copies of the cache
llama3_tables  bf16 cos / sin rows of HF's LlamaRotaryEmbedding (rope_theta 5e5, no scaling) at the given positions
"""
from __future__ import annotations

import numpy as np

import kv_oracle as ko

HD = 128


def f32_to_bf16(x):
    """float32 -> bf16 bits, round to nearest even (finite values)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def _round(x):
    return ko.bf16_to_f32(f32_to_bf16(x))


def rope(x_bits, cos_bits, sin_bits):
    """x uint16 [T, H, 128], cos / sin uint16 [T, 128] -> uint16 [T, H, 128]"""
    x = ko.bf16_to_f32(x_bits)
    c, s = ko.bf16_to_f32(cos_bits)[:, None, :], ko.bf16_to_f32(sin_bits)[:, None, :]
    rot = np.concatenate([-x[..., HD // 2:], x[..., : HD // 2]], axis=-1)
    return f32_to_bf16(_round(x * c) + _round(rot * s))


def rope_append(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, q_bits, k_bits, v_bits, cos_bits, sin_bits, append_indptr, layer):
    """applies the op to host copies of the cache (as kv_oracle.append takes them) and returns the rotated q bits"""
    ko.append(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, rope(k_bits, cos_bits, sin_bits), v_bits, append_indptr, layer)
    return rope(q_bits, cos_bits, sin_bits)


def llama3_tables(positions, theta=500000.0):
    """(cos, sin) uint16 [T, 128]: inv_freq = theta ** -(arange(0, 128, 2) / 128), emb = cat(freqs, freqs), in fp32, cast to bf16"""
    inv = (np.float32(1.0) / np.power(np.float32(theta), np.arange(0, HD, 2, dtype=np.float32) / np.float32(HD))).astype(np.float32)
    freqs = np.asarray(positions, dtype=np.float32)[:, None] * inv[None, :]
    emb = np.concatenate([freqs, freqs], axis=-1)
    return f32_to_bf16(np.cos(emb)), f32_to_bf16(np.sin(emb))
