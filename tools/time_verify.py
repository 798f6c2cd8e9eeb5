"""Greedy verification of drafts on the device, on the MI355X.

    python tools/time_verify.py [out.txt]            (default: profiles/time_verify.txt)

Llama-3-8B's vocabulary (128 256) and heads (8 kv, head_dim 128), page size 16, shuffled pages.
(a) mixedgemm.argmax_rows against torch.argmax(dim=1) on the same bf16 logits, for 1, 21, 64 and 64 x 21 rows.  Each of the ITERS calls
    of a graph reads another buffer of a pool (at least 640 MB or ITERS buffers), so that a call does not find the logits of the call
    before it in the caches; a pool of small buffers still fits the 256 MiB Infinity Cache, and the line says so.
(b) PagedKVCache.verify_launch (mixedgemm.verify_greedy + mixedgemm.kv_move_rows from the device table) for 1 and 64 sequences of the
    21-node tree in 32 layers, the accepted path [0, 2, 10]: the device time of the pair inside a hipGraph, and, by a host clock around
    the calls and a synchronise, the whole step both ways -- verify() (launch + commit) against what a caller did before: copy the T
    target ids to the host, walk the trees in Python, accept(paths).  Both end with the same bookkeeping and table upload.
(c) the argmax as a fraction of 8 TB/s on its own bytes (rows x vocab x 2), from the medians of (a).
Every device time is the median (min .. max) over REPEATS replays, taken in alternation, of a hipGraph that holds ITERS back-to-back
calls, by device events, divided by ITERS; every host time the median (min .. max) over REPEATS steps, taken in alternation.  Nothing
here is a gate.
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
VOCAB, HKV, P, LAYERS = 128256, 8, 16, 32
KINDS = ("int4", "fp8_e4m3", "bf16")
TREE21 = [-1] + [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4
PATH = [0, 2, 10]                                   # root, its second child, that one's second child: slots 2 -> 1 and 10 -> 2 move
PEAK = 8e12                                         # bytes / s


def graph_of(fn):
    """a hipGraph of ITERS back-to-back calls fn(0) .. fn(ITERS - 1), warmed up on a side stream first"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(WARM):
            fn(i)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(ITERS):
            fn(i)
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


def report(lines, rows, title, res, unit="us", **extra):
    for name, us in res.items():
        med = float(np.median(us))
        rows.append(dict(case=title, call=name, median_us=round(med, 2), min_us=round(min(us), 2), max_us=round(max(us), 2), **extra))
        lines.append(f"{title:52} {name:40} {med:10.2f} ({min(us):.2f} .. {max(us):.2f}) {unit}")


def shuffled(cache, seed=0):
    """hand the pages out in a random order, as a server that has run for a while does"""
    cache._free = [cache._free[i] for i in np.random.default_rng(seed).permutation(len(cache._free))]


def argmax_case(rows, dev, gen):
    nbytes = rows * VOCAB * 2
    pool = min(ITERS, max(2, -(-640 * 2 ** 20 // nbytes)))
    logits = [(torch.randn((rows, VOCAB), generator=gen, device=dev) * 3.0).to(torch.bfloat16) for _ in range(pool)]
    ours_out, torch_out = torch.empty((rows,), dtype=torch.int32, device=dev), torch.empty((rows,), dtype=torch.int64, device=dev)
    ws = torch.empty((max(mixedgemm.argmax_rows_workspace_bytes(rows, VOCAB), 16),), dtype=torch.uint8, device=dev)
    same = all(torch.equal(mixedgemm.argmax_rows(x, workspace=ws).long(), torch.argmax(x, dim=1)) for x in logits)
    res = alternate({"mixedgemm.argmax_rows": lambda i: mixedgemm.argmax_rows(logits[i % pool], out=ours_out, workspace=ws),
                     "torch.argmax": lambda i: torch.argmax(logits[i % pool], dim=1, out=torch_out)})
    return res, same, pool, nbytes


def host_walk(target, draft, roots, parents, counts):
    """what a caller did before: the walk of mixedgemm.verify_greedy in Python, over ids already on the host"""
    paths, q0 = [], 0
    for b, n in enumerate(counts):
        cur, want, path = -1, roots[b], []
        while True:
            step = [i for i in range(n) if parents[b][i] == cur and draft[q0 + i] == want]
            if not step:
                break
            cur = step[0]
            path.append(cur)
            want = target[q0 + cur]
        paths.append(path)
        q0 += n
    return paths


def verify_case(kind, B, prior, dev):
    n, steps = len(TREE21), 2 * (REPEATS + 1) + 1
    cache = PagedKVCache(LAYERS, HKV, P, B * (-(-(prior + n + len(PATH) * steps) // P) + 2), B, kind=kind, device=dev)
    shuffled(cache)
    cache.extend(prior)
    draft_h = [100 + i for _ in range(B) for i in range(n)]
    target_h = [0] * (B * n)
    for b in range(B):
        for i, p in enumerate(PATH):
            target_h[b * n + p] = 100 + PATH[i + 1] if i + 1 < len(PATH) else 7
    roots_h = [100] * B
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32).to(dev)
    target, draft, root = i32(target_h), i32(draft_h), i32(roots_h)

    def announce():
        cache.extend(n)
        cache.tree_mask([TREE21] * B)

    # the device time of verify_greedy + kv_move_rows: replays move the rows again, which costs what the first move costs
    announce()
    res = alternate({"verify_launch (verify_greedy + kv_move_rows)": lambda i: cache.verify_launch(target, draft, root)})
    assert cache.commit(cache._verify_result) == ([PATH] * B, [7] * B)

    def ours():
        return cache.verify(target, draft, root)

    def host():
        paths = host_walk(target.cpu().tolist(), draft_h, roots_h, [TREE21] * B, [n] * B)
        cache.accept(paths)
        return paths, None

    clock = {"verify() = verify_launch + commit": [], "ids to host + Python walk + accept": []}
    for rep in range(REPEATS + 1):
        for name, fn in zip(clock, (ours, host)):
            announce()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            paths, _ = fn()
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) * 1e6
            assert paths == [PATH] * B
            if rep:                                             # the first step of each warms it up
                clock[name].append(us)
    return res, clock


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"{REPEATS} replays in alternation of a hipGraph of {ITERS} calls each; us per call: median (min .. max); vocab {VOCAB}, "
             f"MM_ARGMAX_CHUNK {mixedgemm._lib.MM_ARGMAX_CHUNK}"]
    rows, share = [], []
    for nrows in (1, 21, 64, 64 * 21):
        res, same, pool, nbytes = argmax_case(nrows, dev, gen)
        report(lines, rows, f"(a) argmax of {nrows:4} x {VOCAB} bf16 ({nbytes / 2 ** 20:.1f} MB)", res, logit_rows=nrows, same_answers=same, pool=pool)
        lines[-1] += f"   same answers: {same}; pool of {pool} buffers, {pool * nbytes / 2 ** 20:.0f} MB"
        for name, us in res.items():
            share.append((nrows, name, nbytes, float(np.median(us)), pool * nbytes))
        torch.cuda.empty_cache()
    for kind in KINDS:
        for B in (1, 64):
            res, clock = verify_case(kind, B, 1024, dev)
            title = f"(b) {kind:8} {B:2} sequences x 21-node tree, {LAYERS} layers"
            report(lines, rows, title, res, kind=kind, sequences=B)
            report(lines, rows, title, clock, unit="us, host clock, one step", kind=kind, sequences=B)
            torch.cuda.empty_cache()
    for nrows, name, nbytes, med, footprint in share:
        frac = nbytes / (med * 1e-6) / PEAK
        where = "larger than the 256 MiB Infinity Cache" if footprint > 256 * 2 ** 20 else "fits the 256 MiB Infinity Cache"
        rows.append(dict(case="(c)", rows=nrows, call=name, bytes=nbytes, tb_per_s=round(nbytes / (med * 1e-6) / 1e12, 3), share_of_8tbs=round(frac, 3)))
        lines.append(f"(c) {nrows:4} rows {name:24} {nbytes / (med * 1e-6) / 1e12:6.3f} TB/s = {100 * frac:5.1f} % of 8 TB/s (the pool {where})")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_verify.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows)}\n")


if __name__ == "__main__":
    main()
