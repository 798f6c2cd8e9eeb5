"""The three kinds of the paged KV cache side by side on the MI355X: int4, bf16 and fp8 (e4m3) in the same run.

    python tools/time_kv_fp8.py [out.txt]

Llama-3-8B attention heads (Hq 32, Hkv 8, head_dim 128), page size 16, shuffled pages.
decode   1 x 32768 and 64 x 1024 tokens
prefill  512 new tokens over 32768
append   rope_kv_append of T = 4096 tokens (from one packed q | k | v projection)
Time = device events around ITERS back-to-back calls (the merge launch included) / ITERS.  The three kinds of a group are timed
REPEATS times in alternation; a line gives the median and the min .. max over the repeats, and for the attention groups the cache
bytes the call reads (codes plus parameters of the attended tokens, K and V) over the median time.  Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd import mixedgemm  # noqa: E402

ITERS, WARM, REPEATS = 50, 10, 7
HQ, HKV, P, LONG, NEW, T_APPEND = 32, 8, 16, 32768, 512, 4096
KINDS = ("int4", "bf16", "fp8")
ROW_BYTES = {"int4": 64 + 4, "bf16": 256, "fp8": 128 + 4}      # one (token, kv head) row of K or of V, parameters included


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / ITERS     # us


def alternate(cases):
    """name -> [us per repeat]; every repeat times every case once, in turn"""
    for fn in cases.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    out = {n: [] for n in cases}
    for _ in range(REPEATS):
        for n, fn in cases.items():
            out[n].append(timed(fn))
    return out


def cache(kind, B, T, dev, rng):
    """B sequences of T tokens on shuffled pages with random contents, and their page table"""
    npg = -(-T // P)
    max_pages = B * npg
    pages = rng.permutation(max_pages).astype(np.int32).reshape(B, npg)
    shape = (max_pages, 1, 2, HKV, P)
    if kind == "bf16":
        data, param = torch.randn(shape + (128,), device=dev).to(torch.bfloat16), None
    else:
        if kind == "int4":
            data = torch.randint(0, 256, shape + (64,), dtype=torch.uint8, device=dev)
            param = (torch.rand(shape + (2,), device=dev) * 0.2 + 0.05).to(torch.float16)
        else:                                   # every code but the two NaNs; scale 2^-7 .. 2^-5, zero 0
            data = torch.randint(0, 127, shape + (128,), dtype=torch.uint8, device=dev) | (torch.randint(0, 2, shape + (128,), dtype=torch.uint8, device=dev) << 7)
            param = torch.zeros(shape + (2,), dtype=torch.float16, device=dev)
            param[..., 0] = 2.0 ** torch.randint(-7, -4, shape, device=dev).to(torch.float16)
    tbl = (torch.arange(0, B + 1, dtype=torch.int32, device=dev) * npg, torch.from_numpy(pages.reshape(-1)).to(dev),
           torch.full((B,), T - (npg - 1) * P, dtype=torch.int32, device=dev))
    return data, param, tbl


def decode_group(B, T, dev, rng):
    q = torch.randn((B, HQ, 128), device=dev).to(torch.bfloat16)
    cases = {}
    for kind in KINDS:
        data, param, tbl = cache(kind, B, T, dev, rng)
        ws = torch.empty((max(mixedgemm.paged_decode_workspace_bytes(B, HQ, HKV, T), 16),), dtype=torch.uint8, device=dev)
        cases[kind] = (lambda d, p, t, w: lambda: mixedgemm.paged_decode(q, d, p, *t, 0, T, workspace=w))(data, param, tbl, ws)
    return alternate(cases)


def prefill_group(dev, rng):
    q = torch.randn((NEW, HQ, 128), device=dev).to(torch.bfloat16)
    qo = torch.tensor([0, NEW], dtype=torch.int32, device=dev)
    cases = {}
    for kind in KINDS:
        data, param, tbl = cache(kind, 1, LONG, dev, rng)
        ws = torch.empty((max(mixedgemm.paged_prefill_workspace_bytes(NEW, 1, HQ, HKV, LONG), 16),), dtype=torch.uint8, device=dev)
        cases[kind] = (lambda d, p, t, w: lambda: mixedgemm.paged_prefill(q, d, p, *t, qo, 0, LONG, workspace=w))(data, param, tbl, ws)
    return alternate(cases)


def append_group(dev, rng):
    qkv = torch.randn((T_APPEND, (HQ + 2 * HKV) * 128), device=dev).to(torch.bfloat16)
    q, k, v = qkv[:, : HQ * 128], qkv[:, HQ * 128: (HQ + HKV) * 128], qkv[:, (HQ + HKV) * 128:]
    cos, sin = (torch.randn((T_APPEND, 128), device=dev).to(torch.bfloat16) for _ in range(2))
    app = torch.tensor([0, T_APPEND], dtype=torch.int32, device=dev)
    cases = {}
    for kind in KINDS:
        data, param, tbl = cache(kind, 1, T_APPEND, dev, rng)
        cases[kind] = (lambda d, p, t: lambda: mixedgemm.rope_kv_append(d, p, *t, q, k, v, cos, sin, app, 0))(data, param, tbl)
    return alternate(cases)


def main():
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lines, rows = [f"{REPEATS} repeats in alternation of {ITERS} calls each; us: median (min .. max)"], []

    def report(group, res, tokens=None):
        for kind, us in res.items():
            med = float(np.median(us))
            row = dict(group=group, kind=kind, median_us=round(med, 2), min_us=round(min(us), 2), max_us=round(max(us), 2))
            line = f"{group:26} {kind:5} {med:9.2f} ({min(us):.2f} .. {max(us):.2f})"
            if tokens:
                tbs = tokens * HKV * 2 * ROW_BYTES[kind] / med * 1e-6
                row["cache_TB_per_s"] = round(tbs, 3)
                line += f"   {tbs:6.3f} TB/s of cache bytes"
            rows.append(row)
            lines.append(line)
        med = {k: float(np.median(u)) for k, u in res.items()}
        lines.append(f"{'':26} fp8 takes {med['fp8'] / med['bf16']:.3f} x the bf16 time and {med['fp8'] / med['int4']:.3f} x the int4 time")

    report(f"decode 1 x {LONG}", decode_group(1, LONG, dev, rng), LONG)
    report("decode 64 x 1024", decode_group(64, 1024, dev, rng), 64 * 1024)
    report(f"prefill {NEW} over {LONG}", prefill_group(dev, rng))
    report(f"rope_kv_append T = {T_APPEND}", append_group(dev, rng))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows)}\n")


if __name__ == "__main__":
    main()
