"""Numpy oracle of tree-masked attention over the paged KV cache and of row moves (include/micromix_hip.h, mm_paged_prefill_tree,
mm_kv_move_rows), on top of the page walk and the dequantization of tests/kv_oracle.py.

keep_matrix  the rule, in plain words: with base = len - n, query j of a sequence attends every position < base, and new slot
             base + i exactly when i <= j and bit i of its word is set; a sequence with n > 64 ignores its words and is causal
attention    fp64 ragged GQA attention with that keep matrix over the dequantized cache of one layer
vmax         max|V| over the tokens each query attends (only those), per (token, head): the scale of the tolerance's P-rounding term
chain_words  the words under which the rule is the causal mask: bits 0 .. j for query j
tree_words   (words, depths) of a parent list, by walking every node up to the root (not the recurrence PagedKVCache.tree_mask uses)
move_rows    mm_kv_move_rows applied to host copies of a cache

An fp8 cache is passed as its dequantized bf16 bits (tests/kv_fp8_oracle.dequantize) with kv_param None.
"""
from __future__ import annotations

import numpy as np

import kv_oracle as ko

HD = 128
MAX_NODES = 64
MAX_MOVES = 64


def chain_words(n):
    return [(2 << j) - 1 & (1 << 64) - 1 if j < 64 else (1 << 64) - 1 for j in range(n)]


def tree_words(parents):
    words, depths = [], []
    for i, p in enumerate(parents):
        w, d = 1 << i, 0
        while p >= 0:
            w |= 1 << p
            d += 1
            p = parents[p]
        words.append(w)
        depths.append(d)
    return words, depths


def keep_matrix(length, n, words):
    """bool [n, length]: what query j of a sequence of `length` tokens, the last n of them new, attends; words: n Python ints"""
    base = length - n
    keep = np.zeros((n, max(length, 0)), dtype=bool)
    for j in range(n):
        for t in range(max(length, 0)):
            i = t - base
            if n > MAX_NODES:
                keep[j, t] = i <= j
            elif i < 0:
                keep[j, t] = True
            else:
                keep[j, t] = i <= j and bool((int(words[j]) >> i) & 1)
    return keep


def _sequences(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, words, layer):
    P = kv_data.shape[4]
    lens = ko.seq_lens(kv_indptr, last_page_len, P)
    for b in range(len(last_page_len)):
        a0, a1 = int(qo_indptr[b]), int(qo_indptr[b + 1])
        if a1 == a0:
            continue
        K, V = ko.dequantized(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer, b)
        yield a0, K, V, keep_matrix(int(lens[b]), a1 - a0, [int(w) for w in words[a0:a1]])


def attention(q_bits, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, words, layer, sm_scale=None):
    """q uint16 bf16 bits [T, Hq, 128], words: T unsigned Python ints -> float64 [T, Hq, 128]; a row that attends nothing is 0"""
    q = ko.bf16_to_f32(q_bits).astype(np.float64)
    T, Hq, _ = q.shape
    Hkv = kv_data.shape[3]
    g = Hq // Hkv
    scale = HD ** -0.5 if sm_scale is None else sm_scale
    o = np.zeros((T, Hq, HD))
    for a0, K, V, keep in _sequences(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, words, layer):
        n, L = keep.shape
        if L == 0:
            continue
        for h in range(Hkv):
            s = np.einsum("ngd,td->ngt", q[a0:a0 + n, h * g:(h + 1) * g], K[h]) * scale
            s = np.where(keep[:, None, :], s, -np.inf)
            mx = s.max(-1, keepdims=True)
            p = np.where(keep[:, None, :], np.exp(s - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
            den = p.sum(-1, keepdims=True)
            o[a0:a0 + n, h * g:(h + 1) * g] = np.einsum("ngt,td->ngd", p, np.where(keep.any(0)[:, None], V[h], 0.0)) / np.where(den > 0, den, 1.0)
    return o


def vmax(q_shape, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, words, layer):
    """max|V| over the attended tokens of the query's kv head, float64 [T, Hq, 1] (0 where nothing is attended)"""
    T, Hq = q_shape[0], q_shape[1]
    g = Hq // kv_data.shape[3]
    out = np.zeros((T, Hq, 1))
    for a0, K, V, keep in _sequences(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, words, layer):
        if keep.shape[1] == 0:
            continue
        mag = np.abs(V).max(-1)                                                      # [Hkv, L]
        for j in range(keep.shape[0]):
            if keep[j].any():
                out[a0 + j, :, 0] = np.repeat(mag[:, keep[j]].max(-1), g)
    return out


def move_rows(kv_data, kv_param, kv_indptr, kv_indices, move_indptr, src_pos, dst_pos):
    """mm_kv_move_rows on host copies, in place: per sequence its first 64 moves, all sources read before any destination is written;
    a move with src == dst, a position outside the listed pages or a page outside [0, max_pages) is skipped"""
    max_pages, P = kv_data.shape[0], kv_data.shape[4]
    for b in range(len(move_indptr) - 1):
        first, npg = int(kv_indptr[b]), int(kv_indptr[b + 1] - kv_indptr[b])
        held = []
        for m in range(int(move_indptr[b]), min(int(move_indptr[b + 1]), int(move_indptr[b]) + MAX_MOVES)):
            s, d = int(src_pos[m]), int(dst_pos[m])
            if s == d or min(s, d) < 0 or max(s, d) // P >= npg:
                continue
            ps, pd = int(kv_indices[first + s // P]), int(kv_indices[first + d // P])
            if not (0 <= ps < max_pages and 0 <= pd < max_pages):
                continue
            held.append((pd, d % P, kv_data[ps, :, :, :, s % P].copy(), None if kv_param is None else kv_param[ps, :, :, :, s % P].copy()))
        for pd, slot, data, param in held:
            kv_data[pd, :, :, :, slot] = data
            if param is not None:
                kv_param[pd, :, :, :, slot] = param
