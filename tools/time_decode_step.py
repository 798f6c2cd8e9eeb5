"""The one-launch decode step on the MI355X: rope_append_decode against rope_kv_append -> paged_decode, each as one hipGraph.

    python tools/time_decode_step.py [out.txt]            (default: profiles/time_decode_step.txt)

Llama-3-8B heads (Hq 32, Hkv 8, head_dim 128), page size 16, shuffled pages, one layer, the three kinds, at batch x cached tokens
1 x 4 096, 1 x 32 768, 8 x 4 096 and 64 x 1 024; the step's token is the last of each sequence.  q, k, v are views of one packed projection.
Each contender is captured as a hipGraph of STEPS steps (a step writes the same row again, so repeating it changes nothing); both
graphs are replayed in alternation in one process, REPEATS times after WARM warm-up replays, with device events around each replay.
A line gives us per step: the median and the min .. max over the replays.  The outputs and the caches of the two are compared first.
The chain is the code the fused call replaces, unchanged by it.  Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd import mixedgemm  # noqa: E402

STEPS, WARM, REPEATS = 20, 3, 9
HQ, HKV, P = 32, 8, 16
KINDS = ("int4", "fp8_e4m3", "bf16")
SHAPES = ((1, 4096), (1, 32768), (8, 4096), (64, 1024))


def rand(shape, gen, dev, scale=1.0):
    return (torch.randn(shape, generator=gen, device=dev) * scale).to(torch.bfloat16)


def make_cache(kind, B, n, dev, gen):
    """(kv_data, kv_param, page table) of B sequences of n tokens on shuffled pages, all n rows written"""
    per = -(-n // P)
    pages = B * per + 1
    if kind == "bf16":
        data, param = torch.zeros((pages, 1, 2, HKV, P, 128), dtype=torch.bfloat16, device=dev), None
    else:
        data = torch.zeros((pages, 1, 2, HKV, P, 64 if kind == "int4" else 128), dtype=torch.uint8, device=dev)
        param = torch.zeros((pages, 1, 2, HKV, P, 2), dtype=torch.float16, device=dev)
    tbl = [torch.arange(0, B * per + 1, per, dtype=torch.int32, device=dev),
           (1 + torch.randperm(B * per, generator=gen, device=dev)).to(torch.int32),
           torch.full((B,), n - (per - 1) * P, dtype=torch.int32, device=dev)]
    for b in range(B):                                   # one sequence at a time: the append's inputs stay small
        one = [torch.tensor([0, per], dtype=torch.int32, device=dev), tbl[1][b * per: (b + 1) * per].contiguous(), tbl[2][b: b + 1]]
        mixedgemm.kv_append(data, param, *one, rand((n, HKV, 128), gen, dev), rand((n, HKV, 128), gen, dev, 0.5),
                            torch.tensor([0, n], dtype=torch.int32, device=dev), 0)
    return data, param, tbl


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(STEPS):
            out = fn()
    return g, out


def replay_us(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / STEPS


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"us per decode step of one layer: median (min .. max) of {REPEATS} replays, in alternation, of a hipGraph of {STEPS} steps, "
             f"after {WARM} warm-up replays; Hq {HQ}, Hkv {HKV}, P {P}, shuffled pages"]
    out = []
    for kind in KINDS:
        for B, n in SHAPES:
            data, param, tbl = make_cache(kind, B, n, dev, gen)
            twin = (data.clone(), None if param is None else param.clone())
            packed = rand((B, (HQ + 2 * HKV) * 128), gen, dev)
            q, k, v = packed[:, : HQ * 128], packed[:, HQ * 128: (HQ + HKV) * 128], packed[:, (HQ + HKV) * 128:]
            ang = torch.rand((B, 128), generator=gen, device=dev) * 6.28
            cos, sin = ang.cos().to(torch.bfloat16), ang.sin().to(torch.bfloat16)
            app = torch.arange(B + 1, dtype=torch.int32, device=dev)
            ws = torch.empty((max(mixedgemm.rope_append_decode_workspace_bytes(B, HQ, HKV, n), 16),), dtype=torch.uint8, device=dev)
            ws2 = torch.empty_like(ws)

            def chain():
                q_rot = mixedgemm.rope_kv_append(data, param, *tbl, q, k, v, cos, sin, app, 0)
                return mixedgemm.paged_decode(q_rot, data, param, *tbl, 0, n, workspace=ws)

            def fused():
                return mixedgemm.rope_append_decode(*twin, *tbl, q, k, v, cos, sin, 0, n, workspace=ws2)

            (g_chain, o_chain), (g_fused, o_fused) = graph_of(chain), graph_of(fused)
            for _ in range(WARM):
                g_chain.replay()
                g_fused.replay()
            torch.cuda.synchronize()
            same = bool(torch.equal(o_chain.view(torch.int16), o_fused.view(torch.int16)) and
                        torch.equal(data.view(torch.uint8), twin[0].view(torch.uint8)))
            us = {"chain": [], "fused": []}
            for _ in range(REPEATS):
                us["chain"].append(replay_us(g_chain))
                us["fused"].append(replay_us(g_fused))
            med = {m: float(np.median(u)) for m, u in us.items()}
            lines.append(f"-- {kind:8} {B:2} x {n:5}: outputs and caches {'equal' if same else 'DIFFER'}")
            lines.append(f"   append_rope -> attend  {med['chain']:8.2f} ({min(us['chain']):.2f} .. {max(us['chain']):.2f})")
            lines.append(f"   decode_step            {med['fused']:8.2f} ({min(us['fused']):.2f} .. {max(us['fused']):.2f})"
                         f"   chain - fused = {med['chain'] - med['fused']:+.2f} us")
            out.append(dict(kind=kind, batch=B, tokens=n, equal=same, chain_us=[round(u, 2) for u in us["chain"]],
                            fused_us=[round(u, 2) for u in us["fused"]]))
            del g_chain, g_fused, data, param, twin
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_decode_step.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(out)}\n")


if __name__ == "__main__":
    main()
