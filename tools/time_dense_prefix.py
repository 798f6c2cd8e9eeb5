"""New tokens over a cached prefix on the dense kernels (mixedgemm.kv_gather_dense + dense_attention_prefix, the launches of
PagedKVCache.attend_new_dense) on the MI355X, against mixedgemm.paged_prefill over the same cache.

    python tools/time_dense_prefix.py [out.txt]            (default: profiles/time_dense_prefix.txt)

Llama-3-8B heads (Hq 32, Hkv 8, head_dim 128), page size 16, shuffled pages; the cache is filled beforehand (kv_append, not charged).
"gather + prefix" charges all three launches: the gather of the whole layer, the attention and the merge; the two parts are also timed
alone, the gather in TB/s over the bytes it reads and writes.  The square shape also runs dense_attention on contiguous k, v.
us per call inside a hipGraph of ITERS calls between device events, after a warm-up; the contenders' graphs are replayed in turn,
REPEATS times: median (min .. max).  "tiles" is the number of (query tile, kv tile, head) visits of the attention's workgroups, from the
header's walk; ns / tile is the attention alone over it.  The outputs are compared first.  Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd import _lib, mixedgemm  # noqa: E402

ITERS, WARM, REPEATS, P, HQ, HKV = 10, 2, 9, 16, 32, 8
BQ, BK = _lib.ATTENTION["MM_DENSE_ATTN_BQ"], _lib.ATTENTION["MM_DENSE_ATTN_BK"]
ALL = ("int4", "fp8_e4m3", "bf16")
# (name, sequences, new tokens each, tokens held before them, cache kinds)
SHAPES = [("a 512 new over 32768", 1, 512, 32768, ALL), ("b 2048 new over 8192", 1, 2048, 8192, ("int4", "bf16")),
          ("c 4096 new over 28672", 1, 4096, 28672, ("int4", "bf16")), ("d 1 x 4096 square", 1, 4096, 0, ("int4", "bf16")),
          ("e 64 x 5 new over 1024", 64, 5, 1024, ("int4", "bf16"))]
ROW_BYTES = {"int4": 64 + 4, "fp8_e4m3": 128 + 4, "bf16": 256}          # of one (token, kv head) row of K or V as the cache stores it


def tiles(B, nq, nk):
    """kv tiles the attention's workgroups walk, over all query tiles and heads (include/micromix_attention_prefix.h)"""
    return B * HQ * sum(-(-min(nk, nk - nq + i0 + BQ) // BK) for i0 in range(0, nq, BQ))


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


def cache_of(kind, pages, dev):
    shape = (pages, 1, 2, HKV, P)
    if kind == "bf16":
        return torch.zeros(shape + (128,), dtype=torch.bfloat16, device=dev), None
    return (torch.zeros(shape + (64 if kind == "int4" else 128,), dtype=torch.uint8, device=dev),
            torch.zeros(shape + (2,), dtype=torch.float16, device=dev))


def main():
    dev = torch.device("cuda:0")
    gen, rng = torch.Generator(device="cpu").manual_seed(1), np.random.default_rng(1)
    lines = [f"us per call: median (min .. max) over {REPEATS} alternated replays of a hipGraph of {ITERS} calls; Hq {HQ}, Hkv {HKV}, P {P}"]
    rows = []
    for name, B, nq, prior, kinds in SHAPES:
        nk = prior + nq
        Tq, Tk, npg = B * nq, B * nk, -(-nk // P)
        q = torch.randn((Tq, HQ, 128), generator=gen).to(torch.bfloat16).to(dev)
        k, v = (torch.randn((Tk, HKV, 128), generator=gen).to(torch.bfloat16).to(dev) for _ in "kv")
        qo, kvp = (torch.arange(B + 1, dtype=torch.int32, device=dev) * n for n in (nq, nk))
        indices = torch.from_numpy(rng.permutation(B * npg).astype(np.int32)).to(dev)
        kv_indptr = torch.arange(B + 1, dtype=torch.int32, device=dev) * npg
        last = torch.full((B,), nk - (npg - 1) * P, dtype=torch.int32, device=dev)
        nc, chunk = mixedgemm.dense_attention_prefix_plan(Tq, B, HQ, nk)
        visits = tiles(B, nq, nk)
        lines.append(f"{name}: {B} x ({nq} new, {nk} kv tokens); plan: {nc} chunks of {chunk}; {visits} tiles")
        for kind in kinds:
            data, param = cache_of(kind, B * npg, dev)
            mixedgemm.kv_append(data, param, kv_indptr, indices, last, k, v, kvp, 0)           # every token is "new" to the empty cache
            table = (data, param, kv_indptr, indices, last)
            K, V = (torch.empty((Tk, HKV, 128), dtype=torch.bfloat16, device=dev) for _ in "kv")
            ws = torch.empty((max(mixedgemm.dense_attention_prefix_workspace_bytes(Tq, B, HQ, nk), 16),), dtype=torch.uint8, device=dev)
            pws = torch.empty((max(mixedgemm.paged_prefill_workspace_bytes(Tq, B, HQ, HKV, nk), 16),), dtype=torch.uint8, device=dev)

            def gather():
                return mixedgemm.kv_gather_dense(*table, kvp, 0, Tk, K, V)

            def attention():
                return mixedgemm.dense_attention_prefix(q, K, V, qo, kvp, nk, workspace=ws)

            calls = {"gather + prefix (3 launches)": lambda: (gather(), attention())[1], "kv_gather_dense alone": gather,
                     "dense_attention_prefix alone": attention,
                     "paged_prefill": lambda: mixedgemm.paged_prefill(q, *table, qo, 0, nk, workspace=pws)}
            if not prior and kind == "bf16":
                calls["dense_attention on contiguous k, v"] = lambda: mixedgemm.dense_attention(q, k, v, qo)
            diff = float((calls["gather + prefix (3 launches)"]().float() - calls["paged_prefill"]().float()).abs().max())
            assert diff < 0.05, f"{name} {kind}: the two routes disagree by {diff}"
            lines.append(f"  {kind}: max |o - paged_prefill| {diff:.4f}")
            for n, (med, lo, hi) in contest(calls).items():
                extra, row = "", {}
                if n.startswith("kv_gather"):
                    row = dict(gather_TBps=round(2 * Tk * HKV * (ROW_BYTES[kind] + 256) / med / 1e6, 3))
                    extra = f"  {row['gather_TBps']:.2f} TB/s (read + write)"
                elif n.startswith("dense_attention"):
                    row = dict(tiles=visits, ns_per_tile=round(med * 1e3 / visits, 2))
                    extra = f"  {med * 1e3 / visits:6.2f} ns / tile"
                rows.append(dict(shape=name, kind=kind, call=n, median_us=round(med, 1), min_us=round(lo, 1), max_us=round(hi, 1), **row))
                lines.append(f"    {n:38} {med:9.1f} ({lo:.1f} .. {hi:.1f}) us{extra}")
            del calls, data, param, table, K, V, ws, pws
            torch.cuda.empty_cache()

    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_dense_prefix.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows)}\n")


if __name__ == "__main__":
    main()
