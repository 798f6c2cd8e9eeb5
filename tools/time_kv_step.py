"""Device steps of the paged KV cache (mixedgemm.kv_step, PagedKVCache.step_launch / sync), on the MI355X.

    python tools/time_kv_step.py [out.txt]            (default: profiles/time_kv_step.txt)

Llama-3-8B's heads (8 kv, head_dim 128), 32 layers, page size 16, an int4 cache with shuffled pages, 1 and 64 sequences of 1 024 tokens;
the drafts of tools/time_verify.py: the 21-node tree with the accepted path [0, 2, 10], and a chain of 5 of which 2 are accepted.
(a) the device time of one step_launch (the two launches of mm_kv_step) inside a hipGraph of ITERS back-to-back steps, with the keep
    counts of the draft and with keep = None and one token a sequence (plain decode): median (min .. max) over REPEATS replays by device
    events, divided by ITERS.  The sequences grow from replay to replay, as they do in use.
(b) one speculative step by a host clock around blocks of 8 steps and a synchronise, divided by 8: verify_launch + step_launch with one
    sync() per block, against what the host does without device steps, verify() + extend() per step, each step timed by itself (for
    the tree also with the tree_mask() call that a host extend makes necessary again; a device step keeps the tree).  Median
    (min .. max) over REPEATS blocks taken in alternation; both ways run in this process on caches of their own with the same inputs.
    The host path therefore synchronises after every extend() and the device path once per block; verify() synchronises anyway
    through its copy to the host.  Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd.kvcache import PagedKVCache  # noqa: E402

ITERS, WARM, REPEATS, BLOCK = 20, 3, 9, 8
HKV, P, LAYERS, PRIOR, MSL = 8, 16, 32, 1024, 4096
TREE21 = [-1] + [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4
DRAFTS = {"21-node tree, 3 kept": (TREE21, [0, 2, 10]), "chain of 5, 2 kept": (None, [0, 1])}


def i32(xs, dev):
    return torch.tensor(xs, dtype=torch.int32).to(dev)


def new_cache(B, n, steps, dev):
    pages = B * (-(-(PRIOR + n * 2 + 3 * steps) // P) + 2)
    cache = PagedKVCache(LAYERS, HKV, P, pages, B, kind="int4", device=dev)
    cache._free = [cache._free[i] for i in np.random.default_rng(0).permutation(len(cache._free))]
    cache.extend(PRIOR)
    return cache


def draft_inputs(B, n, path, dev):
    """(target_tok, draft_tok, root_tok) under which every sequence's walk takes `path` and the bonus token is 7"""
    target = [0] * (B * n)
    for b in range(B):
        for i, p in enumerate(path):
            target[b * n + p] = 100 + path[i + 1] if i + 1 < len(path) else 7
    return i32(target, dev), i32([100 + i for _ in range(B) for i in range(n)], dev), i32([100] * B, dev)


def device_time(B, n, keep, dev):
    """us per step_launch inside a graph of ITERS of them"""
    cache = new_cache(B, n, WARM + ITERS * (REPEATS + 2), dev)
    cache.extend(n)
    result = None
    if keep is not None:
        result = torch.full((B, 66), -1, dtype=torch.int32, device=dev)
        result[:, 0] = keep
    for _ in range(WARM):
        cache.step_launch(result, n, max_seq_len=MSL)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(ITERS):
            cache.step_launch(result, n, max_seq_len=MSL)
    g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / ITERS)
    cache.sync()                                                 # raises if a step could not be taken
    return us


def host_clock(B, parents, path, dev):
    n, k = len(parents) if parents else 5, len(path)
    blocks = REPEATS + 1
    ours, host = (new_cache(B, n, BLOCK * blocks, dev) for _ in range(2))
    target, draft, root = draft_inputs(B, n, path, dev)
    for c in (ours, host):
        c.extend(n)
        c.tree_mask([parents] * B)
    names = ["verify_launch + step_launch, sync() every 8", "verify() + extend()"] + (["verify() + extend() + tree_mask()"] if parents else [])
    clock = {name: [] for name in names}

    def device_block():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(BLOCK):
            ours.step_launch(ours.verify_launch(target, draft, root), n, max_seq_len=MSL)
        ours.sync()
        torch.cuda.synchronize()
        return [(time.perf_counter() - t0) * 1e6 / BLOCK]

    def host_block():
        """every step is timed by itself, so that the tree_mask() call a host extend makes necessary for a tree can be left out or in"""
        plain = with_mask = 0.0
        for _ in range(BLOCK):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            paths, _ = host.verify(target, draft, root)
            host.extend(n)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            host.tree_mask([parents] * B)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert paths == [path] * B
            plain += t1 - t0
            with_mask += t2 - t0
        return [plain * 1e6 / BLOCK, with_mask * 1e6 / BLOCK]

    for rep in range(blocks):
        got = device_block() + host_block()
        if rep:                                                  # the first block of each warms it up
            for name, us in zip(names, got):
                clock[name].append(us)
    want = [PRIOR + k * BLOCK * blocks + n] * B
    assert ours.seq_lens == want and host.seq_lens == want, (ours.seq_lens[:2], host.seq_lens[:2], want[0])
    return clock


def main():
    dev = torch.device("cuda:0")
    lines = [f"int4 cache, {LAYERS} layers, {HKV} kv heads, page size {P}, {PRIOR} tokens a sequence; us: median (min .. max) over {REPEATS}"]
    rows = []

    def report(title, name, us, unit):
        med = float(np.median(us))
        rows.append(dict(case=title, call=name, median_us=round(med, 2), min_us=round(min(us), 2), max_us=round(max(us), 2)))
        lines.append(f"{title:44} {name:46} {med:9.2f} ({min(us):.2f} .. {max(us):.2f}) {unit}")

    for B in (1, 64):
        for name, (parents, path) in DRAFTS.items():
            n = len(parents) if parents else 5
            report(f"(a) {B:2} sequences, {name}", "step_launch in a hipGraph", device_time(B, n, len(path), dev), "us per step, device")
        report(f"(a) {B:2} sequences, decode, keep = None", "step_launch in a hipGraph", device_time(B, 1, None, dev), "us per step, device")
        torch.cuda.empty_cache()
    for B in (1, 64):
        for name, (parents, path) in DRAFTS.items():
            for call, us in host_clock(B, parents, path, dev).items():
                report(f"(b) {B:2} sequences, {name}", call, us, "us per step, host clock")
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_kv_step.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows)}\n")


if __name__ == "__main__":
    main()
