"""The prefill-shaped RoPE + KV append (include/micromix_rope.h: mm_rope_prefill) on the MI355X, against what each of its three uses
had before.

    python tools/time_rope_prefill.py [out.txt]            (default: profiles/time_rope_prefill.txt)

Llama-3-8B heads (Hq 32, Hkv 8, head_dim 128), page size 16, one prompt of T = 2 048 and T = 4 096 tokens, q | k | v as views of one
packed projection.
(a) rope_kv_append_dense (cache and both outputs) against rope_kv_append on the same inputs, int4 / fp8 / bf16 caches; TB/s and the
    fraction of 8 TB/s on each op's own bytes: q, k, v, cos, sin read, q and the cache rows written, and for the new one k_seen (and
    v_seen, int4 and fp8) written.  The two caches are compared byte for byte first.
(b) rope_qk against HF's bf16 apply_rotary_pos_emb on [1, H, T, 128] tensors, with the transposes that layout needs from and to
    the token-major one.
(c) one layer's prompt ingestion: append_rope + attend_new against prefill_fresh, the three kinds.
us per call inside a hipGraph of ITERS calls between device events, after a warm-up; the contenders' graphs are replayed in turn,
REPEATS times: median (min .. max).  Nothing here is a gate.
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

ITERS, WARM, REPEATS = 10, 2, 9
HQ, HKV, P = 32, 8, 16
KINDS = ("int4", "fp8_e4m3", "bf16")
ROW_BYTES = {"int4": 64 + 4, "fp8_e4m3": 128 + 4, "bf16": 256}


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
    """{name: (median, min, max) us} of the calls, their graphs replayed in turn"""
    graphs = {n: graph_of(c) for n, c in calls.items()}
    us = {n: [] for n in calls}
    for _ in range(REPEATS):
        for n, g in graphs.items():
            us[n].append(replay_us(g))
    return {n: (float(np.median(t)), min(t), max(t)) for n, t in us.items()}


def tables(T, dev):
    """HF LlamaRotaryEmbedding (theta 5e5): bf16 cos, sin [T, 128]"""
    inv = 1.0 / (500000.0 ** (torch.arange(0, 128, 2, device=dev).float() / 128))
    emb = torch.cat([torch.arange(T, device=dev)[:, None].float() * inv] * 2, -1)
    return emb.cos().to(torch.bfloat16), emb.sin().to(torch.bfloat16)


def hf_rope(x, cos, sin):
    """apply_rotary_pos_emb on [1, H, T, 128], cos / sin [1, 1, T, 128]"""
    return (x * cos) + (torch.cat((-x[..., 64:], x[..., :64]), dim=-1) * sin)


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(1)
    lines = [f"us per call: median (min .. max) over {REPEATS} alternated replays of a hipGraph of {ITERS} calls; Hq {HQ}, Hkv {HKV}, P {P}"]
    rows = []

    def report(part, T, kind, res, nbytes=None):
        for n, (med, lo, hi) in res.items():
            nb = (nbytes or {}).get(n)
            rows.append(dict(part=part, T=T, kind=kind, call=n, median_us=round(med, 1), min_us=round(lo, 1), max_us=round(hi, 1),
                             **({"bytes": nb, "tbps": round(nb / med / 1e6, 2)} if nb else {})))
            rate = f"  {nb / 1e6:7.1f} MB  {nb / med / 1e6:5.2f} TB/s  {nb / med / 8e6:4.2f} of 8" if nb else ""
            lines.append(f"    T {T:5d} {kind:9} {n:30} {med:8.1f} ({lo:.1f} .. {hi:.1f}) us{rate}")

    for T in (2048, 4096):
        buf = torch.randn((T, (HQ + 2 * HKV) * 128), generator=gen).to(torch.bfloat16).to(dev)
        q, k, v = buf[:, : HQ * 128], buf[:, HQ * 128: (HQ + HKV) * 128], buf[:, (HQ + HKV) * 128:]
        cos, sin = tables(T, dev)
        common = T * (HQ + 2 * HKV) * 256 + T * 2 * 256 + T * HQ * 256

        lines.append("(a) rope_kv_append_dense (cache, k_seen, v_seen) against rope_kv_append")
        for kind in KINDS:
            old, new = (PagedKVCache(1, HKV, P, T // P + 2, 1, kind=kind, device=dev) for _ in range(2))
            old.extend(T), new.extend(T)
            old.append_rope(0, q, k, v, cos, sin), new.append_rope(0, q, k, v, cos, sin, dense=True)
            assert torch.equal(old.kv_data.view(torch.uint8), new.kv_data.view(torch.uint8)), f"{kind}: the two kernels fill the cache differently"
            cache = common + T * HKV * 2 * ROW_BYTES[kind]
            nbytes = {"rope_kv_append": cache, "rope_kv_append_dense": cache + T * HKV * 256 * (1 if kind == "bf16" else 2)}
            report("a", T, kind, contest({"rope_kv_append": lambda: old.append_rope(0, q, k, v, cos, sin),
                                          "rope_kv_append_dense": lambda: new.append_rope(0, q, k, v, cos, sin, dense=True)}), nbytes)

        lines.append("(b) rope_qk against HF's bf16 apply_rotary_pos_emb on [1, H, T, 128], transposes included")
        c4, s4 = cos[None, None], sin[None, None]

        def hf():
            qh, kh = q.view(1, T, HQ, 128).transpose(1, 2), k.view(1, T, HKV, 128).transpose(1, 2)
            return hf_rope(qh, c4, s4).transpose(1, 2).contiguous(), hf_rope(kh, c4, s4).transpose(1, 2).contiguous()

        assert all(torch.equal(x.view(torch.int16).reshape(-1), y.view(torch.int16).reshape(-1)) for x, y in zip(hf(), mixedgemm.rope_qk(q, k, cos, sin)))
        report("b", T, "-", contest({"torch apply_rotary_pos_emb": hf, "rope_qk": lambda: mixedgemm.rope_qk(q, k, cos, sin)}),
               {"rope_qk": 2 * T * (HQ + HKV) * 256 + T * 2 * 256})

        lines.append("(c) one layer's prompt: append_rope + attend_new against prefill_fresh")
        for kind in KINDS:
            cache = PagedKVCache(1, HKV, P, T // P + 2, 1, kind=kind, device=dev)
            cache.extend(T)
            report("c", T, kind, contest({"append_rope + attend_new": lambda: cache.attend_new(0, cache.append_rope(0, q, k, v, cos, sin), max_seq_len=T),
                                          "prefill_fresh": lambda: cache.prefill_fresh(0, q, k, v, cos, sin)}))
        torch.cuda.empty_cache()

    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_rope_prefill.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows)}\n")


if __name__ == "__main__":
    main()
