"""Paged-KV decode attention on the MI355X: mixedgemm.paged_decode (int4 and bf16 caches) against torch SDPA over contiguous bf16 K/V.

    python tools/time_kv_decode.py [out.txt]

Llama-3-8B attention heads (Hq 32, Hkv 8, head_dim 128), page size 16, shuffled pages; B x context in {1 x 4k, 1 x 32k, 8 x 4k,
64 x 1k}.  Kernel time = device events around `ITERS` back-to-back calls (the merge launch included) / ITERS; the cache bytes read
are len x Hkv x 2 x (64 + 4) (int4) or len x Hkv x 2 x 256 (bf16), as TB/s and as a fraction of 8 TB/s (HBM peak) and 6.3 TB/s
(the copy rate).  SDPA: torch.nn.functional.scaled_dot_product_attention on [B, Hq, 1, 128] x [B, Hq, T, 128] bf16 after the
reference's repeat_kv (what model/qLlamaLayer.py runs without --kv_cache), timed the same way without the repeat.
Last: one Llama-3-8B attention step at M = 1 (FusedQLinear.forward_norm -> RoPE -> append -> attend -> o_proj) as one hipGraph.
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

ITERS, WARM = 50, 10
HQ, HKV, P = 32, 8, 16


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


def case(kind, B, T, dev, rng):
    npg = -(-T // P)
    max_pages = B * npg
    pages = torch.from_numpy(rng.permutation(max_pages).astype(np.int32)).to(dev)
    indptr = torch.arange(0, B + 1, dtype=torch.int32, device=dev) * npg
    last = torch.full((B,), T - (npg - 1) * P, dtype=torch.int32, device=dev)
    if kind == "int4":
        data = torch.randint(0, 256, (max_pages, 1, 2, HKV, P, 64), dtype=torch.uint8, device=dev)
        param = (torch.rand((max_pages, 1, 2, HKV, P, 2), device=dev) * 0.2 + 0.05).to(torch.float16)
        nbytes = B * T * HKV * 2 * (64 + 4)
    else:
        data = torch.randn((max_pages, 1, 2, HKV, P, 128), device=dev).to(torch.bfloat16)
        param = None
        nbytes = B * T * HKV * 2 * 256
    q = torch.randn((B, HQ, 128), device=dev).to(torch.bfloat16)
    ws_bytes = mixedgemm.paged_decode_workspace_bytes(B, HQ, HKV, T)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    us = timed(lambda: mixedgemm.paged_decode(q, data, param, indptr, pages, last, 0, T, workspace=ws))
    return us, nbytes, ws_bytes


def sdpa_case(B, T, dev):
    q = torch.randn((B, HQ, 1, 128), device=dev).to(torch.bfloat16)
    k = torch.randn((B, HKV, T, 128), device=dev).to(torch.bfloat16).repeat_interleave(HQ // HKV, 1)
    v = torch.randn((B, HKV, T, 128), device=dev).to(torch.bfloat16).repeat_interleave(HQ // HKV, 1)
    f = torch.nn.functional.scaled_dot_product_attention
    return timed(lambda: f(q, k, v)), B * T * HKV * 2 * 256


def attention_step(dev, kind, T0=4096):
    from micromix_amd.qlinear import FusedQLinear, QLinearLayer
    H = 4096
    g = torch.Generator().manual_seed(0)
    idx = torch.randperm(H, generator=g).to(torch.int16).to(dev)
    lins = []
    for n, k in ((HQ * 128, H), (HKV * 128, H), (HKV * 128, H), (H, HQ * 128)):
        m = torch.nn.Linear(k, n, bias=False, dtype=torch.bfloat16).to(dev)
        m.weight.data = (torch.randn((n, k), generator=g) * 0.02).to(torch.bfloat16).to(dev)
        lins.append(m)
    fused = FusedQLinear([QLinearLayer(m, p8_num=1024, p6_num=1024, reorder_index=idx) for m in lins[:3]])
    oproj = QLinearLayer(lins[3], p8_num=1024, p6_num=1024, reorder_index=torch.arange(H, dtype=torch.int16, device=dev))
    norm_w = torch.ones((H,), dtype=torch.bfloat16, device=dev)
    inv = 1.0 / (500000.0 ** (torch.arange(0, 128, 2, device=dev).float() / 128))
    cache = PagedKVCache(1, HKV, P, T0 // P + 64, 1, kind=kind, device=dev)
    cache.extend(T0)
    cache.append(0, torch.randn((T0, HKV, 128), device=dev).to(torch.bfloat16), torch.randn((T0, HKV, 128), device=dev).to(torch.bfloat16))
    cache.extend(1)
    x = torch.randn((1, H), device=dev).to(torch.bfloat16)
    pos = torch.full((1,), float(T0), device=dev)

    def rope(t, nh):
        t = t.view(1, nh, 128).float()
        ang = pos * inv
        cos, sin = torch.cat([ang.cos(), ang.cos()]), torch.cat([ang.sin(), ang.sin()])
        return (t * cos + torch.cat([-t[..., 64:], t[..., :64]], -1) * sin).to(torch.bfloat16)

    bound = T0 + 256

    def step():
        q, k, v = fused.forward_norm(x, norm_w, 1e-5)
        q, k = rope(q, HQ), rope(k, HKV)
        cache.append(0, k.contiguous(), v.reshape(1, HKV, 128).contiguous())
        o = cache.attend(0, q.contiguous(), max_seq_len=bound)
        return oproj(o.reshape(1, 1, HQ * 128))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return timed(graph.replay), timed(step, 20)


def main():
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lines, rows = [], []
    lines.append(f"{'cache':6} {'B x T':>10} {'us':>8} {'MB read':>8} {'TB/s':>6} {'/8':>5} {'/6.3':>5} {'workspace':>9}")
    for B, T in ((1, 4096), (1, 32768), (8, 4096), (64, 1024)):
        for kind in ("int4", "bf16"):
            us, nb, ws = case(kind, B, T, dev, rng)
            tbs = nb / us / 1e6
            rows.append(dict(kind=kind, B=B, T=T, us=round(us, 2), bytes=nb, tbps=round(tbs, 3), workspace=ws))
            lines.append(f"{kind:6} {f'{B} x {T}':>10} {us:8.2f} {nb / 1e6:8.2f} {tbs:6.2f} {tbs / 8:5.2f} {tbs / 6.3:5.2f} {ws:9d}")
        us, nb = sdpa_case(B, T, dev)
        rows.append(dict(kind="sdpa_bf16", B=B, T=T, us=round(us, 2), bytes=nb, tbps=round(nb / us / 1e6, 3)))
        lines.append(f"{'sdpa':6} {f'{B} x {T}':>10} {us:8.2f} {nb / 1e6:8.2f} {nb / us / 1e6:6.2f}   (torch SDPA, contiguous bf16 K/V after repeat_kv)")
    for kind in ("int4", "bf16"):
        g_us, e_us = attention_step(dev, kind)
        rows.append(dict(kind=f"attention_step_{kind}", T=4096, graph_us=round(g_us, 2), eager_us=round(e_us, 2)))
        lines.append(f"Llama-3-8B attention step at M = 1, 4096 cached tokens, {kind} cache: {g_us:.2f} us as one hipGraph ({e_us:.2f} us eager)")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows)}\n")


if __name__ == "__main__":
    main()
