"""Sliding-window dense attention (mixedgemm.dense_attention_window) on the MI355X, against the un-windowed kernel on the same tensors
(the upper reference), mixedgemm.paged_prefill(window=) over a bf16 cache holding the same tokens, and torch SDPA under a band mask; and
PagedKVCache.prefill_fresh(windowed=True) against append_rope + attend_new on a windowed cache.

    python tools/time_dense_window.py [out.txt]            (default: profiles/time_dense_window.txt)

Llama-3-8B heads (Hq 32, Hkv 8, head_dim 128), W = 4 096: one sequence of 8 192 and of 32 768 tokens, and one ragged batch.  q, k, v are
views of one packed projection; the cache of paged_prefill (page size 16, shuffled pages) is filled beforehand and not charged; SDPA
gets K / V already repeated and a boolean band mask, and runs where that [T, T] mask is at most SDPA_MASK_TOKENS on a side.
us per call inside a hipGraph of ITERS calls between device events, after a warm-up; the contenders' graphs are replayed in turn,
REPEATS times: median (min .. max).  "tiles" is the number of (query tile, kv tile, head) visits of the dense kernels' workgroups, from
the header's walk; ns / tile is the median over it.  The outputs are compared first.  Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd import _lib, mixedgemm  # noqa: E402
from micromix_amd.kvcache import PagedKVCache  # noqa: E402

ITERS, WARM, REPEATS, P, HQ, HKV, W, SDPA_MASK_TOKENS = 10, 2, 9, 16, 32, 8, 4096, 8192
BQ, BK = _lib.ATTENTION["MM_DENSE_ATTN_BQ"], _lib.ATTENTION["MM_DENSE_ATTN_BK"]
SHAPES = [("a 1 x 8192", [8192]), ("b 1 x 32768", [32768]), ("c ragged 12000 6000 9000 3000 5000", [12000, 6000, 9000, 3000, 5000])]


def tiles(lens, window):
    """kv tiles the dense kernels' workgroups walk, over all query tiles and heads (include/micromix_attention_window.h, Walk)"""
    return HQ * sum(-(-min(n, i0 + BQ) // BK) - max(0, i0 - window + 1) // BK for n in lens for i0 in range(0, n, BQ))


def graph_of(call):
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(ITERS):
            call()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / ITERS


def contest(calls):
    """{name: (median, min, max) us}: every contender's graph replayed in turn, REPEATS times"""
    graphs = {n: graph_of(c) for n, c in calls.items()}
    us = {n: [] for n in calls}
    for _ in range(REPEATS):
        for n, g in graphs.items():
            us[n].append(replay_us(g))
    return {n: (float(np.median(t)), min(t), max(t)) for n, t in us.items()}


def tables(T, dev):
    """HF LlamaRotaryEmbedding (theta 5e5): bf16 cos, sin [T, 128]"""
    inv = 1.0 / (500000.0 ** (torch.arange(0, 128, 2, device=dev).float() / 128))
    emb = torch.cat([torch.arange(T, device=dev)[:, None].float() * inv] * 2, -1)
    return emb.cos().to(torch.bfloat16), emb.sin().to(torch.bfloat16)


def main():
    dev = torch.device("cuda:0")
    gen, rng = torch.Generator(device="cpu").manual_seed(1), np.random.default_rng(1)
    lines = [f"us per call: median (min .. max) over {REPEATS} alternated replays of a hipGraph of {ITERS} calls; Hq {HQ}, Hkv {HKV}, W {W}"]
    rows = []

    def report(shape, res, visits=None):
        for n, (med, lo, hi) in res.items():
            nt = (visits or {}).get(n)
            rows.append(dict(shape=shape, call=n, median_us=round(med, 1), min_us=round(lo, 1), max_us=round(hi, 1),
                             **({"tiles": nt, "ns_per_tile": round(med * 1e3 / nt, 2)} if nt else {})))
            lines.append(f"    {n:46} {med:9.1f} ({lo:.1f} .. {hi:.1f}) us" + (f"  {nt:9d} tiles  {med * 1e3 / nt:6.2f} ns / tile" if nt else ""))

    for name, lens in SHAPES:
        T, B, g = sum(lens), len(lens), HQ // HKV
        packed = torch.randn((T, (HQ + 2 * HKV) * 128), generator=gen).to(torch.bfloat16).to(dev)
        q, k, v = packed[:, :HQ * 128], packed[:, HQ * 128:(HQ + HKV) * 128], packed[:, (HQ + HKV) * 128:]
        indptr = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)

        # paged_prefill(window=): a bf16 cache that holds the same tokens
        npg = [-(-n // P) for n in lens]
        pages = torch.from_numpy(rng.permutation(sum(npg)).astype(np.int32)).to(dev)
        kv_indptr = torch.tensor(np.concatenate([[0], np.cumsum(npg)]), dtype=torch.int32, device=dev)
        last = torch.tensor([n - (c - 1) * P for n, c in zip(lens, npg)], dtype=torch.int32, device=dev)
        data = torch.zeros((sum(npg), 1, 2, HKV, P, 128), dtype=torch.bfloat16, device=dev)
        mixedgemm.kv_append(data, None, kv_indptr, pages, last, k.reshape(T, HKV, 128).contiguous(), v.reshape(T, HKV, 128).contiguous(), indptr, 0)
        qc = q.reshape(T, HQ, 128).contiguous()
        ws = torch.empty((max(mixedgemm.paged_prefill_workspace_bytes(T, B, HQ, HKV, max(lens), W), 16),), dtype=torch.uint8, device=dev)

        calls = {"dense_attention_window": lambda: mixedgemm.dense_attention_window(q, k, v, W, indptr),
                 "dense_attention (no window)": lambda: mixedgemm.dense_attention(q, k, v, indptr),
                 "paged_prefill(window=) bf16": lambda: mixedgemm.paged_prefill(qc, data, None, kv_indptr, pages, last, indptr, 0, max(lens),
                                                                                workspace=ws, window=W)}
        if T <= SDPA_MASK_TOKENS:                               # torch SDPA: K / V repeated beforehand, [1, Hq, T, 128], a [T, T] band mask
            sq = qc.transpose(0, 1)[None]
            sk, sv = (t.reshape(T, HKV, 128).repeat_interleave(g, 1).transpose(0, 1)[None].contiguous() for t in (k, v))
            seq = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(lens, device=dev))
            pos = torch.arange(T, device=dev)
            mask = (seq[:, None] == seq[None, :]) & (pos[None, :] <= pos[:, None]) & (pos[None, :] > pos[:, None] - W)
            calls["torch SDPA, band mask"] = lambda: torch.nn.functional.scaled_dot_product_attention(sq, sk, sv, attn_mask=mask)
        outs = {n: c().reshape(-1, T, 128).float() if n.startswith("torch") else c().transpose(0, 1).float() for n, c in calls.items()
                if "no window" not in n}
        diffs = {n: float((o - outs["dense_attention_window"]).abs().max()) for n, o in outs.items() if n != "dense_attention_window"}
        assert max(diffs.values()) < 0.05, f"the contenders disagree: {diffs}"
        del outs
        visits = {"dense_attention_window": tiles(lens, W), "dense_attention (no window)": tiles(lens, T)}
        lines.append(f"{name}: T {T}; max |o - dense_attention_window|: " + ", ".join(f"{n} {d:.4f}" for n, d in diffs.items()))
        report(name, contest(calls), visits)
        del calls
        torch.cuda.empty_cache()

    lines.append("one layer's prompt on a cache made with window=: append_rope + attend_new against prefill_fresh(windowed=True)")
    for T in (8192, 32768):
        buf = torch.randn((T, (HQ + 2 * HKV) * 128), generator=gen).to(torch.bfloat16).to(dev)
        q, k, v = buf[:, : HQ * 128], buf[:, HQ * 128: (HQ + HKV) * 128], buf[:, (HQ + HKV) * 128:]
        cos, sin = tables(T, dev)
        for kind in ("int4", "fp8_e4m3", "bf16"):
            cache = PagedKVCache(1, HKV, P, T // P + 2, 1, kind=kind, device=dev, window=W)
            cache.extend(T)
            report(f"T {T} {kind}", contest({f"T {T} {kind} append_rope + attend_new": lambda: cache.attend_new(0, cache.append_rope(0, q, k, v, cos, sin), max_seq_len=T),
                                             f"T {T} {kind} prefill_fresh(windowed=True)": lambda: cache.prefill_fresh(0, q, k, v, cos, sin, windowed=True)}))
        torch.cuda.empty_cache()

    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_dense_window.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows)}\n")


if __name__ == "__main__":
    main()
