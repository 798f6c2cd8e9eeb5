"""Sliding-window attention over the paged KV cache on the MI355X: what a window saves over a long sequence.

    python tools/time_kv_window.py [out.txt]

Llama-3-8B attention heads (Hq 32, Hkv 8, head_dim 128), page size 16, shuffled pages, int4 and bf16 caches, W = 4096.
decode   B in {1, 8}: un-windowed over 4096 tokens (what the window should cost), windowed over 32768, un-windowed over 32768.
prefill  512 new tokens over 32768: windowed and un-windowed at the same shape, beside the kv tiles each visits (counted from the shapes).
Time = device events around ITERS back-to-back calls (the merge launch included) / ITERS.  The cases of a group are timed REPEATS
times in alternation; a line gives the median and the min .. max over the repeats.  The verdict of a decode group compares the
windowed median with the 4096-token median plus that case's own spread (max - min) plus one 32-token tile of 4096 (a wave walks
whole tiles); the prefill verdict compares the speed-up with the ratio of visited tiles.
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
HQ, HKV, P, W, LONG, NEW = 32, 8, 16, 4096, 32768, 512


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


def cache(kind, B, dev, rng):
    """B sequences of LONG tokens on shuffled pages, random contents; table(T) is the page table of their first T tokens"""
    npg = LONG // P
    max_pages = B * npg
    pages = rng.permutation(max_pages).astype(np.int32).reshape(B, npg)
    if kind == "int4":
        data = torch.randint(0, 256, (max_pages, 1, 2, HKV, P, 64), dtype=torch.uint8, device=dev)
        param = (torch.rand((max_pages, 1, 2, HKV, P, 2), device=dev) * 0.2 + 0.05).to(torch.float16)
    else:
        data, param = torch.randn((max_pages, 1, 2, HKV, P, 128), device=dev).to(torch.bfloat16), None

    def table(T):
        n = -(-T // P)
        return (torch.arange(0, B + 1, dtype=torch.int32, device=dev) * n, torch.from_numpy(np.ascontiguousarray(pages[:, :n]).reshape(-1)).to(dev),
                torch.full((B,), T - (n - 1) * P, dtype=torch.int32, device=dev))
    return data, param, table


def decode_group(kind, B, dev, rng):
    data, param, table = cache(kind, B, dev, rng)
    q = torch.randn((B, HQ, 128), device=dev).to(torch.bfloat16)

    def call(T, window):
        tbl = table(T)
        ws = torch.empty((max(mixedgemm.paged_decode_workspace_bytes(B, HQ, HKV, T, window), 16),), dtype=torch.uint8, device=dev)
        return lambda: mixedgemm.paged_decode(q, data, param, *tbl, 0, T, workspace=ws, window=window)
    return alternate({f"full {B} x {W}": call(W, None), f"window {B} x {LONG}": call(LONG, W), f"full {B} x {LONG}": call(LONG, None)})


def visited_tiles(window):
    """kv tiles (64 tokens) the query tiles (64 / g tokens) of NEW tokens that end at LONG walk"""
    bq, n = 64 // (HQ // HKV), 0
    for pos0 in range(LONG - NEW, LONG, bq):
        lo = max(0, pos0 - window + 1) // 64 * 64 if window else 0
        n += -(-(pos0 + bq - lo) // 64)
    return n


def prefill_group(kind, dev, rng):
    data, param, table = cache(kind, 1, dev, rng)
    q = torch.randn((NEW, HQ, 128), device=dev).to(torch.bfloat16)
    qo = torch.tensor([0, NEW], dtype=torch.int32, device=dev)
    tbl = table(LONG)

    def call(window):
        ws = torch.empty((max(mixedgemm.paged_prefill_workspace_bytes(NEW, 1, HQ, HKV, LONG, window), 16),), dtype=torch.uint8, device=dev)
        return lambda: mixedgemm.paged_prefill(q, data, param, *tbl, qo, 0, LONG, workspace=ws, window=window)
    return alternate({f"window {NEW} over {LONG}": call(W), f"full {NEW} over {LONG}": call(None)})


def main():
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lines, rows = [f"W = {W}, {REPEATS} repeats in alternation of {ITERS} calls each; us: median (min .. max)"], []

    def report(kind, group, res):
        for name, us in res.items():
            med = float(np.median(us))
            rows.append(dict(group=group, kind=kind, case=name, median_us=round(med, 2), min_us=round(min(us), 2), max_us=round(max(us), 2)))
            lines.append(f"{group:8} {kind:5} {name:22} {med:9.2f} ({min(us):.2f} .. {max(us):.2f})")
        return {n: float(np.median(u)) for n, u in res.items()}

    for kind in ("int4", "bf16"):
        for B in (1, 8):
            res = decode_group(kind, B, dev, rng)
            med = report(kind, "decode", res)
            ref = res[f"full {B} x {W}"]
            allowed = med[f"full {B} x {W}"] * (1 + 32 / W) + (max(ref) - min(ref))
            got = med[f"window {B} x {LONG}"]
            lines.append(f"         {kind:5} window over {LONG} {got:.2f} us against {allowed:.2f} us allowed (full over {W} + its spread + one tile): "
                         f"{'within' if got <= allowed else 'ABOVE'}; full over {LONG} is {med[f'full {B} x {LONG}'] / got:.2f} x the window")
            rows.append(dict(group="decode", kind=kind, B=B, allowed_us=round(allowed, 2), window_us=round(got, 2), within=bool(got <= allowed)))
    tw, tf = visited_tiles(W), visited_tiles(0)
    for kind in ("int4", "bf16"):
        med = report(kind, "prefill", prefill_group(kind, dev, rng))
        speed = med[f"full {NEW} over {LONG}"] / med[f"window {NEW} over {LONG}"]
        lines.append(f"         {kind:5} the window is {speed:.2f} x faster; it visits {tw} kv tiles against {tf}: {tf / tw:.2f} x fewer")
        rows.append(dict(group="prefill", kind=kind, speedup=round(speed, 3), tiles_window=tw, tiles_full=tf, tile_ratio=round(tf / tw, 3)))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows)}\n")


if __name__ == "__main__":
    main()
