"""Shared-prefix decode on the MI355X: attend(shared=True) against attend() on the same forked cache.

    python tools/time_kv_shared.py [out.txt]            (default: profiles/r17_time_kv_shared.txt)

Llama-3-8B heads (Hq 32, Hkv 8, head_dim 128, page size 16), one layer, the three kinds.  A prompt is appended once, forked to n
samples, and every sample decodes 64 tokens of its own (the first step copies the partly filled last page where there is one), so the
samples share the prompt's whole pages and hold 64 tokens each on pages of their own:
    8 samples of a 4096-token prompt, 64 samples of a 4096-token prompt, 64 samples of a 1024-token prompt,
    and 8 sequences of 4160 tokens that share nothing: what the shared path costs when taken for no reason.
attend() is the path the cache had before (mm_paged_decode: every sample walks the prompt's pages itself); attend(shared=True) is
mm_paged_decode_shared with the groups share_groups() found.  Both run on the same cache object, with their default bounds.
Time = device events around ITERS back-to-back calls / ITERS; the two are timed REPEATS times in alternation after WARM calls each; a
line gives the median and the min .. max over the repeats.  One layer's K and V of these caches fit the 256 MiB Infinity Cache, so
this is the kernels' time on cached data, the regime DESIGN 7b describes (bound by the tile chain, not by bytes).  The largest
difference between the two outputs is printed beside the times.  Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd.kvcache import PagedKVCache  # noqa: E402

ITERS, WARM, REPEATS = 200, 10, 7
HQ, HKV, P, STEPS = 32, 8, 16, 64
KINDS = ("int4", "fp8_e4m3", "bf16")
SHAPES = (("8 samples of a 4096-token prompt", 8, 4096, True), ("64 samples of a 4096-token prompt", 64, 4096, True),
          ("64 samples of a 1024-token prompt", 64, 1024, True), ("8 sequences of 4160 tokens, nothing shared", 8, 4096, False))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / ITERS     # us


def alternate(cases):
    for fn in cases.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    out = {n: [] for n in cases}
    for _ in range(REPEATS):
        for n, fn in cases.items():
            out[n].append(timed(fn))
    return out


def rand(shape, gen, dev, scale=1.0):
    return (torch.randn(shape, generator=gen, device=dev) * scale).to(torch.bfloat16)


def build(kind, samples, prompt, fork, dev, gen):
    pages = (-(-prompt // P) + 1 + samples * (-(-STEPS // P) + 1)) if fork else samples * (-(-(prompt + STEPS) // P) + 1)
    cache = PagedKVCache(1, HKV, P, pages, samples, kind=kind, device=dev)
    first = [prompt] + [0] * (samples - 1) if fork else [prompt] * samples
    cache.extend(first)
    cache.append(0, rand((sum(first), HKV, 128), gen, dev), rand((sum(first), HKV, 128), gen, dev, 0.5))
    if fork:
        for s in range(1, samples):
            cache.fork(0, s)
    for _ in range(STEPS):
        cache.extend(1)
        cache.append(0, rand((samples, HKV, 128), gen, dev), rand((samples, HKV, 128), gen, dev, 0.5))
    return cache


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"{REPEATS} repeats in alternation of {ITERS} calls each after {WARM} warm-up calls; us per call: median (min .. max); "
             f"Hq {HQ}, Hkv {HKV}, P {P}, one layer, {STEPS} decoded tokens per sample"]
    out = []
    for kind in KINDS:
        for name, samples, prompt, fork in SHAPES:
            cache = build(kind, samples, prompt, fork, dev, gen)
            groups, shared = cache.share_groups()
            q = rand((samples, HQ, 128), gen, dev, 2.0)
            o_plain, o_shared = cache.attend(0, q), cache.attend(0, q, shared=True)
            torch.cuda.synchronize()
            diff = float((o_plain.float() - o_shared.float()).abs().max())
            res = alternate({"attend()": lambda: cache.attend(0, q), "attend(shared=True)": lambda: cache.attend(0, q, shared=True)})
            med = {n: float(np.median(us)) for n, us in res.items()}
            lines.append(f"-- {kind}: {name}: {len(groups)} group(s), shared count {max(shared)}, longest tail {cache._max_suffix}; "
                         f"max |attend() - attend(shared=True)| = {diff:.3e}")
            for n, us in res.items():
                lines.append(f"   {n:20} {med[n]:9.2f} ({min(us):.2f} .. {max(us):.2f})")
            lines.append(f"   attend() / attend(shared=True) = {med['attend()'] / med['attend(shared=True)']:.2f}")
            out.append(dict(kind=kind, shape=name, samples=samples, prompt=prompt, groups=len(groups), shared=max(shared),
                            plain_us=[round(u, 2) for u in res["attend()"]], shared_us=[round(u, 2) for u in res["attend(shared=True)"]],
                            plain_over_shared=round(med["attend()"] / med["attend(shared=True)"], 3), max_abs_diff=diff))
            del cache
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    print(json.dumps(out))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r17_time_kv_shared.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(out)}\n")


if __name__ == "__main__":
    main()
