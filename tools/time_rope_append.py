"""The fused RoPE + KV append on the MI355X: mixedgemm.rope_kv_append / PagedKVCache.append_rope against the glue it replaces.

    python tools/time_rope_append.py [out.txt]

Llama-3-8B attention heads (Hq 32, Hkv 8, head_dim 128), page size 16.
1. The op alone at T = 1 and T = 4096, int4 and bf16 caches, from views of the packed q | k | v projection: one launch against
   torch bf16 RoPE (HF apply_rotary_pos_emb) + `.contiguous()` + kv_append.  Time = device events around ITERS back-to-back calls / ITERS.
   At T = 4096 the op's own bytes (q, k, v, cos, sin read; q and the cache rows written) as TB/s and as a fraction of 8 TB/s.
2. One Llama-3-8B attention step at M = 1 over 4096 cached tokens as one hipGraph (FusedQLinear.forward_norm -> RoPE -> append -> attend ->
   o_proj), three ways in the same run: the float RoPE of tools/time_kv_decode.py, a bf16 torch RoPE, and append_rope.
"""
from __future__ import annotations

import json
import os
import sys

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


def tables(pos, dev):
    """HF LlamaRotaryEmbedding (theta 5e5): bf16 cos, sin [T, 128]"""
    inv = 1.0 / (500000.0 ** (torch.arange(0, 128, 2, device=dev).float() / 128))
    emb = torch.cat([pos[:, None].float() * inv, pos[:, None].float() * inv], -1)
    return emb.cos().to(torch.bfloat16), emb.sin().to(torch.bfloat16)


def rope_bf16(x, cos, sin):
    cos, sin = cos.unsqueeze(1), sin.unsqueeze(1)
    return (x * cos) + (torch.cat((-x[..., 64:], x[..., :64]), dim=-1) * sin)


def op_alone(kind, T, dev):
    cache = PagedKVCache(1, HKV, P, T // P + 2, 1, kind=kind, device=dev)
    cache.extend(T)
    buf = torch.randn((T, (HQ + 2 * HKV) * 128), device=dev).to(torch.bfloat16)
    q, k, v = buf.split([HQ * 128, HKV * 128, HKV * 128], dim=1)
    cos, sin = tables(torch.arange(T, device=dev), dev)

    def unfused():
        qr = rope_bf16(q.view(T, HQ, 128), cos, sin).contiguous()
        cache.append(0, rope_bf16(k.view(T, HKV, 128), cos, sin).contiguous(), v.reshape(T, HKV, 128).contiguous())
        return qr

    fused_us = timed(lambda: cache.append_rope(0, q, k, v, cos, sin))
    unfused_us = timed(unfused)
    rows = T * HKV * 2 * ((64 + 4) if kind == "int4" else 256)
    nbytes = T * (HQ + 2 * HKV) * 256 + T * 2 * 256 + T * HQ * 256 + rows
    return fused_us, unfused_us, nbytes


def attention_steps(dev, kind, T0=4096):
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
    x = torch.randn((1, H), device=dev).to(torch.bfloat16)
    pos = torch.full((1,), float(T0), device=dev)
    cos_t, sin_t = tables(pos, dev)          # what the model computes once per forward for all layers
    bound = T0 + 256

    def fresh_cache():
        cache = PagedKVCache(1, HKV, P, T0 // P + 64, 1, kind=kind, device=dev)
        cache.extend(T0)
        cache.append(0, torch.randn((T0, HKV, 128), device=dev).to(torch.bfloat16), torch.randn((T0, HKV, 128), device=dev).to(torch.bfloat16))
        cache.extend(1)
        return cache

    def rope_float(t, nh):                   # the chain of tools/time_kv_decode.py
        t = t.view(1, nh, 128).float()
        ang = pos * inv
        cos, sin = torch.cat([ang.cos(), ang.cos()]), torch.cat([ang.sin(), ang.sin()])
        return (t * cos + torch.cat([-t[..., 64:], t[..., :64]], -1) * sin).to(torch.bfloat16)

    def step_float(cache):
        q, k, v = fused.forward_norm(x, norm_w, 1e-5)
        q, k = rope_float(q, HQ), rope_float(k, HKV)
        cache.append(0, k.contiguous(), v.reshape(1, HKV, 128).contiguous())
        return oproj(cache.attend(0, q.contiguous(), max_seq_len=bound).reshape(1, 1, HQ * 128))

    def step_bf16(cache):
        q, k, v = fused.forward_norm(x, norm_w, 1e-5)
        q, k = rope_bf16(q.view(1, HQ, 128), cos_t, sin_t), rope_bf16(k.view(1, HKV, 128), cos_t, sin_t)
        cache.append(0, k.contiguous(), v.reshape(1, HKV, 128).contiguous())
        return oproj(cache.attend(0, q.contiguous(), max_seq_len=bound).reshape(1, 1, HQ * 128))

    def step_fused(cache):
        q, k, v = fused.forward_norm(x, norm_w, 1e-5)
        return oproj(cache.attend(0, cache.append_rope(0, q, k, v, cos_t, sin_t), max_seq_len=bound).reshape(1, 1, HQ * 128))

    out = {}
    for name, step in (("float_rope", step_float), ("bf16_rope", step_bf16), ("append_rope", step_fused)):
        cache = fresh_cache()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                step(cache)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step(cache)
        out[name] = (timed(graph.replay), timed(lambda: step(cache), 20))
    return out


def main():
    dev = torch.device("cuda:0")
    lines, rows = [], []
    lines.append(f"{'cache':6} {'T':>5} {'fused us':>9} {'torch rope + append us':>23} {'MB moved':>9} {'TB/s':>6} {'/8':>5}")
    for T in (1, 4096):
        for kind in ("int4", "bf16"):
            f_us, u_us, nb = op_alone(kind, T, dev)
            tbs = nb / f_us / 1e6
            rows.append(dict(kind=kind, T=T, fused_us=round(f_us, 2), unfused_us=round(u_us, 2), bytes=nb, tbps=round(tbs, 3)))
            lines.append(f"{kind:6} {T:5d} {f_us:9.2f} {u_us:23.2f} {nb / 1e6:9.3f} {tbs:6.2f} {tbs / 8:5.2f}")
    for kind in ("int4", "bf16"):
        res = attention_steps(dev, kind)
        for name, (g_us, e_us) in res.items():
            rows.append(dict(kind=f"attention_step_{kind}", chain=name, T=4096, graph_us=round(g_us, 2), eager_us=round(e_us, 2)))
            lines.append(f"Llama-3-8B attention step at M = 1, 4096 cached tokens, {kind} cache, {name:11}: {g_us:7.2f} us as one hipGraph "
                         f"({e_us:.2f} us eager)")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows)}\n")


if __name__ == "__main__":
    main()
