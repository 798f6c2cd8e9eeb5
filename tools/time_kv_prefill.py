"""Causal multi-token attention over the paged KV cache on the MI355X: mixedgemm.paged_prefill (int4 and bf16 caches) against torch
SDPA over contiguous bf16 K/V.

    python tools/time_kv_prefill.py [out.txt]

Llama-3-8B attention heads (Hq 32, Hkv 8, head_dim 128), page size 16, shuffled pages, on
  (a) full prefill 1 x 4096 (q_len = kv_len)          (b) a chunk of 512 new tokens over 32768 cached
  (c) 8 ragged prompts of 300-700 tokens               (d) speculative verify: 64 sequences x 5 new over 1024 cached
  (e) 64 x 1 new over 1024, next to paged_decode
Kernel time = device events around ITERS back-to-back calls (the merge launch included) / ITERS.  TFLOP/s on the causal FLOPs:
4 * 128 * Hq * sum over the queries of (p + 1), p the query's position.  Baseline: torch.nn.functional.scaled_dot_product_attention
per sequence over contiguous bf16 K/V after the reference's repeat_kv, is_causal when square and an explicit bottom-right boolean mask
otherwise (the gather / dequantization of the cache is not charged to it).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd import mixedgemm  # noqa: E402

ITERS, WARM = 20, 5
HQ, HKV, P = 32, 8, 16
PEAK_TF = 2500.0


def timed(fn, iters=ITERS):
    for _ in range(WARM):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters     # us


def shapes():
    rng = np.random.default_rng(0)
    return {
        "a_prefill_1x4096": ([0], [4096]),
        "b_chunk_512_over_32k": ([32768], [512]),
        "c_ragged_8x300-700": ([0] * 8, rng.integers(300, 701, 8).tolist()),
        "d_spec_64x5_over_1k": ([1024] * 64, [5] * 64),
        "e_decode_64x1_over_1k": ([1024] * 64, [1] * 64),
    }


def causal_flops(prior, new):
    return sum(4 * 128 * HQ * sum(a + j + 1 for j in range(n)) for a, n in zip(prior, new))


def cache_case(kind, prior, new, dev, rng):
    lens = [a + n for a, n in zip(prior, new)]
    npg = [-(-n // P) for n in lens]
    max_pages = sum(npg)
    pages = torch.from_numpy(rng.permutation(max_pages).astype(np.int32)).to(dev)
    indptr = torch.from_numpy(np.concatenate([[0], np.cumsum(npg)]).astype(np.int32)).to(dev)
    last = torch.tensor([n - (k - 1) * P for n, k in zip(lens, npg)], dtype=torch.int32, device=dev)
    qo = torch.from_numpy(np.concatenate([[0], np.cumsum(new)]).astype(np.int32)).to(dev)
    if kind == "int4":
        data = torch.randint(0, 256, (max_pages, 1, 2, HKV, P, 64), dtype=torch.uint8, device=dev)
        param = torch.stack([torch.rand((max_pages, 1, 2, HKV, P), device=dev) * 0.2 + 0.05,
                             torch.rand((max_pages, 1, 2, HKV, P), device=dev)], -1).to(torch.float16)
    else:
        data = torch.randn((max_pages, 1, 2, HKV, P, 128), device=dev).to(torch.bfloat16)
        param = None
    T, B, msl = sum(new), len(new), max(lens)
    q = torch.randn((T, HQ, 128), device=dev).to(torch.bfloat16)
    ws_bytes = mixedgemm.paged_prefill_workspace_bytes(T, B, HQ, HKV, msl)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    us = timed(lambda: mixedgemm.paged_prefill(q, data, param, indptr, pages, last, qo, 0, msl, workspace=ws))
    extra = {}
    if all(n == 1 for n in new):
        dws = torch.empty((max(mixedgemm.paged_decode_workspace_bytes(B, HQ, HKV, msl), 16),), dtype=torch.uint8, device=dev)
        extra["paged_decode_us"] = round(timed(lambda: mixedgemm.paged_decode(q, data, param, indptr, pages, last, 0, msl, workspace=dws)), 2)
    return us, ws_bytes, extra


def sdpa_case(prior, new, dev):
    """one SDPA call per sequence (ragged lengths), K/V contiguous bf16 after repeat_kv"""
    f = torch.nn.functional.scaled_dot_product_attention
    calls = []
    same = len(set(zip(prior, new))) == 1
    groups = [(prior[0], new[0], len(new))] if same else [(a, n, 1) for a, n in zip(prior, new)]
    for a, n, b in groups:
        L = a + n
        q = torch.randn((b, HQ, n, 128), device=dev).to(torch.bfloat16)
        k = torch.randn((b, HKV, L, 128), device=dev).to(torch.bfloat16).repeat_interleave(HQ // HKV, 1)
        v = torch.randn((b, HKV, L, 128), device=dev).to(torch.bfloat16).repeat_interleave(HQ // HKV, 1)
        if a == 0:
            calls.append((q, k, v, None, True))
        else:
            mask = torch.arange(L, device=dev)[None, :] <= (a + torch.arange(n, device=dev))[:, None]
            calls.append((q, k, v, mask, False))

    def run():
        for q, k, v, m, c in calls:
            f(q, k, v, attn_mask=m, is_causal=c)
    return timed(run)


def main():
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    rows, lines = [], []
    for name, (prior, new) in shapes().items():
        fl = causal_flops(prior, new)
        t_sdpa = sdpa_case(prior, new, dev)
        line = [f"{name:24s} T={sum(new):5d}  {fl / 1e9:8.2f} GFLOP  torch SDPA {t_sdpa:9.1f} us ({fl / t_sdpa / 1e6:6.1f} TF/s)"]
        row = dict(shape=name, T=sum(new), B=len(new), gflop=round(fl / 1e9, 3), sdpa_us=round(t_sdpa, 2))
        for kind in ("int4", "bf16"):
            us, wsb, extra = cache_case(kind, prior, new, dev, rng)
            line.append(f"{kind} {us:9.1f} us ({fl / us / 1e6:6.1f} TF/s, {fl / us / 1e6 / PEAK_TF:5.3f} of peak, x{t_sdpa / us:5.2f})"
                        + (f" [paged_decode {extra['paged_decode_us']:.1f} us]" if extra else ""))
            row[f"{kind}_us"] = round(us, 2)
            row[f"{kind}_tflops"] = round(fl / us / 1e6, 1)
            row[f"{kind}_split"] = wsb > 0
            row.update({f"{kind}_{k}": v for k, v in extra.items()})
        rows.append(row)
        lines.append("\n    ".join(line))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows)}\n")


if __name__ == "__main__":
    main()
