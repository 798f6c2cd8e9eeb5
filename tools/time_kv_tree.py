"""Tree-masked attention over the paged KV cache and keeping a path, on the MI355X.

    python tools/time_kv_tree.py [out.txt]            (default: profiles/time_kv_tree.txt)

Llama-3-8B heads (32 query, 8 kv, head_dim 128), page size 16, shuffled pages, the three cache kinds.
(a) mixedgemm.paged_prefill(tree_mask=) with a chain's words against mixedgemm.paged_prefill on the same cache and queries (the same
    bits): 64 sequences x 8 new tokens over 1 024, and 1 x 64 new tokens over 32 768.
(b) a 4-ary tree of depth 3 (21 nodes) over a 1 024-token prompt, verified in one call -- append + attend_new(tree=) of one layer on
    one sequence -- against the same tree laid out as its 16 root-to-leaf paths: 16 forked sequences of 3 tokens, append +
    attend_new.  The second form appends 48 tokens for 21 and holds 16 page lists; its copy-on-write and forks are not in the time.
(c) keeping a depth-3 path of that tree in 32 layers, for 1 and for 64 sequences: mixedgemm.kv_move_rows (one launch, all layers)
    against the same moves with torch indexing (a gather and a scatter per tensor), and PagedKVCache.accept as a whole (host
    bookkeeping, the launch and the table upload; a host clock around the call and a synchronise).
Every device time is the median (min .. max) over REPEATS replays, taken in alternation, of a hipGraph that holds ITERS back-to-back
calls, by device events, divided by ITERS.  Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd import mixedgemm  # noqa: E402
from micromix_amd.kvcache import PagedKVCache  # noqa: E402

ITERS, WARM, REPEATS = 20, 3, 9
HQ, HKV, P, LAYERS = 32, 8, 16, 32
KINDS = ("int4", "fp8_e4m3", "bf16")
TREE21 = [-1] + [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4
PATH = [0, 2, 10]                                   # root, its second child, that one's second child: slots 2 -> 1 and 10 -> 2 move


def rand(shape, gen, dev, scale=1.0):
    return (torch.randn(shape, generator=gen, device=dev) * scale).to(torch.bfloat16)


def graph_of(fn):
    """a hipGraph of ITERS back-to-back calls of fn, warmed up on a side stream first"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(WARM):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(ITERS):
            fn()
    return g


def alternate(cases):
    graphs = {n: graph_of(fn) for n, fn in cases.items()}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    out = {n: [] for n in cases}
    for _ in range(REPEATS):
        for n, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            out[n].append(a.elapsed_time(b) * 1e3 / ITERS)     # us per call
    return out


def report(lines, rows, title, res, **extra):
    for name, us in res.items():
        med = float(np.median(us))
        rows.append(dict(case=title, call=name, median_us=round(med, 2), min_us=round(min(us), 2), max_us=round(max(us), 2), **extra))
        lines.append(f"{title:58} {name:34} {med:9.2f} ({min(us):.2f} .. {max(us):.2f}) us")


def shuffled(cache, seed=0):
    """hand the pages out in a random order, as a server that has run for a while does"""
    cache._free = [cache._free[i] for i in np.random.default_rng(seed).permutation(len(cache._free))]


def chain_against_causal(kind, B, prior, n, dev, gen):
    cache = PagedKVCache(1, HKV, P, B * (-(-(prior + n) // P) + 1), B, kind=kind, device=dev)
    shuffled(cache)
    cache.extend(prior)
    cache.append(0, rand((B * prior, HKV, 128), gen, dev), rand((B * prior, HKV, 128), gen, dev, 0.5))
    cache.extend(n)
    cache.append(0, rand((B * n, HKV, 128), gen, dev), rand((B * n, HKV, 128), gen, dev, 0.5))
    q = rand((B * n, HQ, 128), gen, dev, 2.0)
    mask, _ = cache.tree_mask([None] * B)
    bound = prior + n
    ws = torch.empty((max(mixedgemm.paged_prefill_workspace_bytes(B * n, B, HQ, HKV, bound), 16),), dtype=torch.uint8, device=dev)
    tbl = (cache.kv_data, cache.kv_param, cache.kv_indptr, cache.kv_indices, cache.last_page_len, cache.append_indptr, 0, bound)
    causal = lambda: mixedgemm.paged_prefill(q, *tbl, workspace=ws)
    tree = lambda: mixedgemm.paged_prefill(q, *tbl, workspace=ws, tree_mask=mask)
    same = torch.equal(causal().view(torch.int16), tree().view(torch.int16))
    return alternate({"paged_prefill": causal, "paged_prefill(tree_mask=chain)": tree}), same


def tree_against_paths(kind, prior, dev, gen):
    k, v = rand((prior, HKV, 128), gen, dev), rand((prior, HKV, 128), gen, dev, 0.5)
    one = PagedKVCache(1, HKV, P, prior // P + 8, 1, kind=kind, device=dev)
    many = PagedKVCache(1, HKV, P, prior // P + 40, 16, kind=kind, device=dev)
    for cache in (one, many):
        shuffled(cache)
        cache.extend([prior] + [0] * (cache.batch - 1))
        cache.append(0, k, v)
    for s in range(1, 16):
        many.fork(0, s)
    one.extend(21)
    many.extend(3)
    mask, _ = one.tree_mask([TREE21])
    q1, k1, v1 = rand((21, HQ, 128), gen, dev, 2.0), rand((21, HKV, 128), gen, dev), rand((21, HKV, 128), gen, dev, 0.5)
    q16, k16, v16 = rand((48, HQ, 128), gen, dev, 2.0), rand((48, HKV, 128), gen, dev), rand((48, HKV, 128), gen, dev, 0.5)
    bound = prior + 64

    def tree():
        one.append(0, k1, v1)
        return one.attend_new(0, q1, max_seq_len=bound, tree=mask)

    def paths():
        many.append(0, k16, v16)
        return many.attend_new(0, q16, max_seq_len=bound)
    return alternate({"1 sequence, 21-node tree": tree, "16 forked sequences x 3 tokens": paths}), (one.pages_in_use, many.pages_in_use)


def keep_a_path(kind, B, prior, dev, gen):
    cache = PagedKVCache(LAYERS, HKV, P, B * (-(-(prior + 21) // P) + 1), B, kind=kind, device=dev)
    shuffled(cache)
    cache.extend(prior)
    cache.extend(21)
    cache.tree_mask([TREE21] * B)
    moves = [(prior + s, prior + d) for d, s in enumerate(PATH) if s != d]
    src = [s for _ in range(B) for s, _ in moves]
    dst = [d for _ in range(B) for _, d in moves]
    table = torch.tensor([len(moves) * b for b in range(B + 1)] + src + dst, dtype=torch.int32).to(dev)
    mptr, src_d, dst_d = table.split([B + 1, len(src), len(dst)])
    pages = lambda pos: torch.tensor([cache._pages[b][p // P] for b in range(B) for p in pos], device=dev)
    slots = lambda pos: torch.tensor([p % P for _ in range(B) for p in pos], device=dev)
    sp, ss, dp, ds = pages([s for s, _ in moves]), slots([s for s, _ in moves]), pages([d for _, d in moves]), slots([d for _, d in moves])

    def ours():
        mixedgemm.kv_move_rows(cache.kv_data, cache.kv_param, cache.kv_indptr, cache.kv_indices, mptr, src_d, dst_d)

    def indexing():
        for t in (cache.kv_data, cache.kv_param):
            if t is not None:
                t[dp, :, :, :, ds] = t[sp, :, :, :, ss]
    res = alternate({"kv_move_rows": ours, "torch indexing": indexing})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cache.accept([PATH] * B)
    torch.cuda.synchronize()
    return res, (time.perf_counter() - t0) * 1e6


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"{REPEATS} replays in alternation of a hipGraph of {ITERS} calls each; us per call: median (min .. max); Hq {HQ}, Hkv {HKV}, P {P}"]
    rows = []
    for kind in KINDS:
        for B, prior, n in ((64, 1024, 8), (1, 32768, 64)):
            res, same = chain_against_causal(kind, B, prior, n, dev, gen)
            report(lines, rows, f"(a) {kind:8} {B:2} x {n:2} new over {prior:5}", res, kind=kind, same_bits=same)
            lines[-1] += f"   same bits: {same}"
    for kind in KINDS:
        res, used = tree_against_paths(kind, 1024, dev, gen)
        report(lines, rows, f"(b) {kind:8} 21-node tree over 1024, append + attend_new", res, kind=kind, pages_tree=used[0], pages_paths=used[1])
        lines[-1] += f"   pages in use: {used[0]} (tree) against {used[1]} (paths)"
    for kind in KINDS:
        for B in (1, 64):
            res, accept_us = keep_a_path(kind, B, 1024, dev, gen)
            report(lines, rows, f"(c) {kind:8} {B:2} sequences, path {PATH}, {LAYERS} layers", res, kind=kind, sequences=B)
            rows.append(dict(case="(c) accept", kind=kind, sequences=B, host_us=round(accept_us, 1)))
            lines.append(f"{'':58} {'PagedKVCache.accept (host clock)':34} {accept_us:9.1f} us, one call")
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_kv_tree.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows)}\n")


if __name__ == "__main__":
    main()
