"""Numpy oracle of sliding-window attention over the paged KV cache (include/micromix_hip.h, mm_paged_decode_window /
mm_paged_prefill_window), on top of tests/kv_oracle.py and tests/kv_prefill_oracle.py.

`window` = W >= 1 is HF's sliding_window: the query at position p attends positions max(0, p - W + 1) .. p.  Decode: p = len_b - 1;
prefill: p = len_b - n_b + j (bottom-right).  W None or 0: no window.  A page-table entry of -1 (a released page) may stand below
every window of its sequence: the values read for it are never used.

decode_attention    fp64 single-token GQA attention over the last W tokens of every sequence
prefill_attention   fp64 ragged causal GQA attention, every query over its own window
prefill_vmax        max|V| over the tokens each query attends: the scale of the prefill tolerance's P-rounding term
With W >= the lengths the first two run the operations of kv_oracle.attention / kv_prefill_oracle.attention on the same arrays: equal bit for bit.
"""
from __future__ import annotations

import numpy as np

import kv_oracle as ko

HD = 128


def window_begin(p, W):
    """first attended position of a query at position p (array or int)"""
    p = np.asarray(p, dtype=np.int64)
    return np.maximum(p - W + 1, 0) if W else np.zeros_like(p)


def _dequantized(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer, b):
    """ko.dequantized with released entries pointed at page 0: what comes back for them lies below every window and is sliced away"""
    idx = np.asarray(kv_indices)
    return ko.dequantized(kv_data, kv_param, kv_indptr, np.where(idx < 0, 0, idx), last_page_len, layer, b)


def decode_attention(q_bits, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer, window, sm_scale=None):
    """q uint16 bf16 bits [B, Hq, 128] -> float64 [B, Hq, 128]"""
    q = ko.bf16_to_f32(q_bits).astype(np.float64)
    B, Hq, _ = q.shape
    g = Hq // kv_data.shape[3]
    scale = HD ** -0.5 if sm_scale is None else sm_scale
    o = np.zeros((B, Hq, HD))
    for b in range(B):
        K, V = _dequantized(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer, b)
        n = K.shape[1]
        if n == 0:
            continue
        lo = int(window_begin(n - 1, window))
        if lo:
            K, V = K[:, lo:], V[:, lo:]
        Kr, Vr = np.repeat(K, g, axis=0), np.repeat(V, g, axis=0)    # HF repeat_kv
        s = np.einsum("hd,htd->ht", q[b], Kr) * scale
        p = np.exp(s - s.max(-1, keepdims=True))
        o[b] = np.einsum("ht,htd->hd", p / p.sum(-1, keepdims=True), Vr)
    return o


def _sequences(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, layer, window):
    """yield (first token index, K, V, lo, keep) per sequence with queries: K, V float64 [Hkv, len - lo, 128] from position lo on (the
    lowest any of its queries attends), keep bool [n, len - lo]"""
    P = kv_data.shape[4]
    lens = ko.seq_lens(kv_indptr, last_page_len, P)
    for b in range(len(last_page_len)):
        a0, a1 = int(qo_indptr[b]), int(qo_indptr[b + 1])
        if a1 == a0:
            continue
        K, V = _dequantized(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer, b)
        n, L = a1 - a0, int(lens[b])
        na = np.maximum(L - n + np.arange(n) + 1, 0)                  # attended counts without a window: positions 0 .. na - 1
        first = window_begin(na - 1, window) if window else np.zeros(n, dtype=np.int64)
        lo = int(first.min()) if L else 0
        t = np.arange(lo, L)
        keep = (t[None, :] < na[:, None]) & (t[None, :] >= first[:, None])
        yield a0, (K[:, lo:] if lo else K), (V[:, lo:] if lo else V), lo, keep


def prefill_attention(q_bits, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, layer, window, sm_scale=None):
    """q uint16 bf16 bits [T, Hq, 128] -> float64 [T, Hq, 128]"""
    q = ko.bf16_to_f32(q_bits).astype(np.float64)
    T, Hq, _ = q.shape
    Hkv = kv_data.shape[3]
    g = Hq // Hkv
    scale = HD ** -0.5 if sm_scale is None else sm_scale
    o = np.zeros((T, Hq, HD))
    for a0, K, V, lo, keep in _sequences(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, layer, window):
        n = keep.shape[0]
        if K.shape[1] == 0:
            continue
        for h in range(Hkv):                                                       # query heads h g .. h g + g - 1 (HF repeat_kv)
            s = np.einsum("ngd,td->ngt", q[a0:a0 + n, h * g:(h + 1) * g], K[h]) * scale
            s = np.where(keep[:, None, :], s, -np.inf)
            mx = s.max(-1, keepdims=True)
            p = np.where(keep[:, None, :], np.exp(s - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
            den = p.sum(-1, keepdims=True)
            o[a0:a0 + n, h * g:(h + 1) * g] = np.einsum("ngt,td->ngd", p, V[h]) / np.where(den > 0, den, 1.0)
    return o


def prefill_vmax(q_shape, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, layer, window):
    """max|V| over the attended tokens of the query's kv head, float64 [T, Hq, 1] (0 where nothing is attended)"""
    T, Hq = q_shape[0], q_shape[1]
    g = Hq // kv_data.shape[3]
    out = np.zeros((T, Hq, 1))
    for a0, K, V, lo, keep in _sequences(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, layer, window):
        if V.shape[1] == 0:
            continue
        av = np.abs(V).max(-1)                                                       # [Hkv, len - lo]
        for j in range(keep.shape[0]):
            if keep[j].any():
                out[a0 + j, :, 0] = np.repeat(av[:, keep[j]].max(-1), g)
    return out
