"""Page sharing in the paged KV cache on the MI355X: the copy-on-write kernel against torch's index ops, and the pages a fork saves.

    python tools/time_kv_fork.py [out.txt]            (default: profiles/r16_time_kv_fork.txt)

Llama-3-8B geometry (32 layers, 8 kv heads, head_dim 128, page size 16), the three kinds.
(a) mixedgemm.kv_copy_pages for 1, 8 and 64 pairs with rows 1, 8 and 16, against
    kv_data.index_copy_(0, dst, kv_data.index_select(0, src)) (and the same for kv_param), which always moves whole pages.
    Time = device events around ITERS back-to-back calls / ITERS, so a small call shows the rate at which the host can issue
    it, not the kernel's own time.  The cases of one (kind, pairs) group are timed REPEATS times in
    alternation; a line gives the median and the min .. max over the repeats, and the bytes the call reads plus writes (codes and
    parameters of the rows it moves) over the median time as a fraction of 8 TB/s.  The pool holds POOL pages and every call of a
    window takes the next pairs in it, so a page comes round again only after the whole pool (larger than the 256 MiB Infinity Cache
    for every kind) has gone by.
(b) pages_in_use of 8 samples forked from one 4096-token prompt after 64 decode steps, against 8 independent sequences.
Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd import mixedgemm  # noqa: E402
from micromix_amd.kvcache import PagedKVCache  # noqa: E402

ITERS, WARM, REPEATS = 50, 10, 7
L, HKV, P, POOL = 32, 8, 16, 1024
KINDS = ("int4", "fp8", "bf16")
ROW_BYTES = {"int4": 64 + 4, "fp8": 128 + 4, "bf16": 256}        # one (token, kv head) row of K or of V, parameters included
PEAK = 8e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(ITERS):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / ITERS     # us


def alternate(cases):
    for fn in cases.values():
        for i in range(WARM):
            fn(i)
    torch.cuda.synchronize()
    out = {n: [] for n in cases}
    for _ in range(REPEATS):
        for n, fn in cases.items():
            out[n].append(timed(fn))
    return out


def pool(kind, dev):
    shape = (POOL, L, 2, HKV, P)
    if kind == "bf16":
        return torch.randn(shape + (128,), device=dev).to(torch.bfloat16), None
    data = torch.randint(0, 256, shape + (64 if kind == "int4" else 128,), dtype=torch.uint8, device=dev)
    return data, torch.rand(shape + (2,), device=dev).to(torch.float16)


def copy_group(kind, pairs, data, param, dev, rng):
    """the calls of a window walk through the pool: set i holds `pairs` sources and as many other pages as destinations"""
    sets = POOL // (2 * pairs)
    perm = rng.permutation(POOL)[: sets * 2 * pairs].reshape(sets, 2, pairs)
    src32, dst32 = (torch.from_numpy(perm[:, j].astype(np.int32)).to(dev) for j in (0, 1))
    src64, dst64 = src32.long(), dst32.long()
    cases = {}
    for r in (1, 8, 16):
        rows = torch.full((pairs,), r, dtype=torch.int32, device=dev)
        cases[f"kv_copy_pages rows {r}"] = (lambda rw: lambda i: mixedgemm.kv_copy_pages(data, param, src32[i % sets], dst32[i % sets], rw))(rows)

    def torch_copy(i):
        data.index_copy_(0, dst64[i % sets], data.index_select(0, src64[i % sets]))
        if param is not None:
            param.index_copy_(0, dst64[i % sets], param.index_select(0, src64[i % sets]))
    cases["torch index_select + index_copy_"] = torch_copy
    return alternate(cases), sets


def pages_saved(dev):
    prompt, samples, steps = 4096, 8, 64
    need = samples * -(-(prompt + steps) // P)
    forked = PagedKVCache(1, 1, P, need, samples, kind="int4", device=dev)       # the bookkeeping does not depend on layers, heads or kind
    alone = PagedKVCache(1, 1, P, need, samples, kind="int4", device=dev)
    forked.extend([prompt] + [0] * (samples - 1))
    for s in range(1, samples):
        forked.fork(0, s)
    alone.extend(prompt)
    for _ in range(steps):
        forked.extend(1)
        alone.extend(1)
    torch.cuda.synchronize()
    return forked.pages_in_use, alone.pages_in_use


def main():
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lines = [f"{REPEATS} repeats in alternation of {ITERS} calls each; us: median (min .. max); pool of {POOL} pages, L {L}, Hkv {HKV}, P {P}"]
    out = []
    for kind in KINDS:
        data, param = pool(kind, dev)
        page_mb = L * 2 * HKV * P * ROW_BYTES[kind] / 2 ** 20
        lines.append(f"-- {kind}: a page is {page_mb:.3f} MiB, the pool {page_mb * POOL / 1024:.2f} GiB")
        for pairs in (1, 8, 64):
            res, sets = copy_group(kind, pairs, data, param, dev, rng)
            base = float(np.median(res["torch index_select + index_copy_"]))
            for name, us in res.items():
                r = int(name.split()[-1]) if name.startswith("kv_copy") else P
                moved = 2 * pairs * L * 2 * HKV * r * ROW_BYTES[kind]
                med = float(np.median(us))
                frac = moved / (med * 1e-6) / PEAK
                out.append(dict(kind=kind, pairs=pairs, case=name, median_us=round(med, 2), min_us=round(min(us), 2), max_us=round(max(us), 2),
                                bytes_read_plus_written=moved, fraction_of_8TBps=round(frac, 4), torch_over_this=round(base / med, 2)))
                lines.append(f"{kind:5} {pairs:3} pairs  {name:34} {med:9.2f} ({min(us):.2f} .. {max(us):.2f})   {moved / 2 ** 20:8.2f} MiB moved"
                             f"   {frac:6.3f} of 8 TB/s   torch / this = {base / med:5.2f}")
        del data, param
        torch.cuda.empty_cache()
    f, a = pages_saved(dev)
    lines.append(f"-- 8 samples of a 4096-token prompt after 64 decode steps: {f} pages in use forked, {a} pages as 8 independent sequences")
    for kind in KINDS:
        mib = L * 2 * HKV * P * ROW_BYTES[kind] / 2 ** 20
        lines.append(f"   {kind:5} {f * mib / 1024:7.3f} GiB forked, {a * mib / 1024:7.3f} GiB independent")
    out.append(dict(case="pages_in_use", forked=f, independent=a))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(out))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r16_time_kv_fork.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(out)}\n")


if __name__ == "__main__":
    main()
