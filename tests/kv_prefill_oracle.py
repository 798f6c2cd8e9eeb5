"""Numpy oracle of causal multi-token attention over the paged KV cache (include/micromix_hip.h, mm_paged_prefill).

attention   fp64 ragged causal GQA attention over the dequantized cache of one layer (tests/kv_oracle.dequantized): sequence b's
            j-th new query token sits at position len_b - n_b + j and attends positions 0 .. that one (bottom-right alignment)
vmax        max|V| over the tokens each query attends, per (token, head): the scale of the tolerance's P-rounding term
"""
from __future__ import annotations

import numpy as np

import kv_oracle as ko

HD = 128


def _sequences(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, layer):
    """yield (first token index, K, V, attended counts) per sequence with queries; K, V float64 [Hkv, len, 128], counts int [n]"""
    P = kv_data.shape[4]
    lens = ko.seq_lens(kv_indptr, last_page_len, P)
    for b in range(len(last_page_len)):
        a0, a1 = int(qo_indptr[b]), int(qo_indptr[b + 1])
        if a1 == a0:
            continue
        K, V = ko.dequantized(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer, b)
        n, L = a1 - a0, int(lens[b])
        yield a0, K, V, np.maximum(L - n + np.arange(n) + 1, 0)


def attention(q_bits, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, layer, sm_scale=None):
    """q uint16 bf16 bits [T, Hq, 128] -> float64 [T, Hq, 128]"""
    q = ko.bf16_to_f32(q_bits).astype(np.float64)
    T, Hq, _ = q.shape
    Hkv = kv_data.shape[3]
    g = Hq // Hkv
    scale = HD ** -0.5 if sm_scale is None else sm_scale
    o = np.zeros((T, Hq, HD))
    for a0, K, V, na in _sequences(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, layer):
        n, L = len(na), K.shape[1]
        if L == 0:
            continue
        keep = np.arange(L)[None, :] < na[:, None]                                 # [n, L] causal, bottom-right
        for h in range(Hkv):                                                       # query heads h g .. h g + g - 1 (HF repeat_kv)
            s = np.einsum("ngd,td->ngt", q[a0:a0 + n, h * g:(h + 1) * g], K[h]) * scale
            s = np.where(keep[:, None, :], s, -np.inf)
            mx = s.max(-1, keepdims=True)
            p = np.where(keep[:, None, :], np.exp(s - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
            den = p.sum(-1, keepdims=True)
            o[a0:a0 + n, h * g:(h + 1) * g] = np.einsum("ngt,td->ngd", p, V[h]) / np.where(den > 0, den, 1.0)
    return o


def vmax(q_shape, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, layer):
    """max|V| over the attended tokens of the query's kv head, float64 [T, Hq, 1] (0 where nothing is attended)"""
    T, Hq = q_shape[0], q_shape[1]
    g = Hq // kv_data.shape[3]
    out = np.zeros((T, Hq, 1))
    for a0, K, V, na in _sequences(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, layer):
        if K.shape[1] == 0:
            continue
        run = np.maximum.accumulate(np.abs(V).max(-1), axis=1)                       # [Hkv, L]: max|V| of positions 0..t
        for j, c in enumerate(na):
            if c:
                out[a0 + j, :, 0] = np.repeat(run[:, c - 1], g)
    return out
