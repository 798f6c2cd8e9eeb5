"""Dense causal GQA attention over contiguous bf16 q, k, v (mixedgemm.dense_attention) on the MI355X, against the two routes the same
call had before: mixedgemm.paged_prefill over a bf16 cache holding the same tokens, and torch SDPA after repeat_kv.

    python tools/time_dense_attention.py [out.txt]            (default: profiles/time_dense_attention.txt)

Shapes (head_dim 128): (a) 1 x 4 096 and (b) 1 x 2 048 with Llama-3-8B heads (Hq 32, Hkv 8), (c) 8 ragged prompts of 300-700 tokens, the
same heads, (d) 1 x 4 096 with Hq 40 (Qwen2.5-14B).  dense_attention reads q, k, v in place as views of one packed projection; the cache
of paged_prefill (page size 16, shuffled pages) is filled beforehand and not charged; SDPA gets K / V already repeated, is_causal when
the batch is one sequence and a block-diagonal causal boolean mask over the flattened tokens when it is ragged.
us per call inside a hipGraph of ITERS calls between device events, after a warm-up; the three contenders' graphs are replayed in turn,
REPEATS times: median (min .. max).  TF/s on the causal FLOPs 4 * 128 * Hq * sum(i + 1).  The outputs of the three are compared first.
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

ITERS, WARM, REPEATS, P = 10, 2, 9, 16


def shapes():
    rng = np.random.default_rng(0)
    return [("a 1 x 4096", 32, 8, [4096]), ("b 1 x 2048", 32, 8, [2048]), ("c 8 ragged 300-700", 32, 8, rng.integers(300, 701, 8).tolist()),
            ("d 1 x 4096, Hq 40", 40, 8, [4096])]


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


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(1)
    rng = np.random.default_rng(1)
    lines = [f"us per call: median (min .. max) over {REPEATS} alternated replays of a hipGraph of {ITERS} calls; TF/s on the causal FLOPs"]
    rows_out = []
    for name, Hq, Hkv, lens in shapes():
        T, B, g = sum(lens), len(lens), Hq // Hkv
        flops = sum(4 * 128 * Hq * n * (n + 1) // 2 for n in lens)
        packed = torch.randn((T, (Hq + 2 * Hkv) * 128), generator=gen).to(torch.bfloat16).to(dev)
        q, k, v = packed[:, :Hq * 128], packed[:, Hq * 128:(Hq + Hkv) * 128], packed[:, (Hq + Hkv) * 128:]
        indptr = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)

        # paged_prefill: a bf16 cache that holds the same tokens
        npg = [-(-n // P) for n in lens]
        pages = torch.from_numpy(rng.permutation(sum(npg)).astype(np.int32)).to(dev)
        kv_indptr = torch.tensor(np.concatenate([[0], np.cumsum(npg)]), dtype=torch.int32, device=dev)
        last = torch.tensor([n - (c - 1) * P for n, c in zip(lens, npg)], dtype=torch.int32, device=dev)
        data = torch.zeros((sum(npg), 1, 2, Hkv, P, 128), dtype=torch.bfloat16, device=dev)
        mixedgemm.kv_append(data, None, kv_indptr, pages, last, k.reshape(T, Hkv, 128).contiguous(), v.reshape(T, Hkv, 128).contiguous(), indptr, 0)
        qc = q.reshape(T, Hq, 128).contiguous()
        ws = torch.empty((max(mixedgemm.paged_prefill_workspace_bytes(T, B, Hq, Hkv, max(lens)), 16),), dtype=torch.uint8, device=dev)

        # torch SDPA: K / V repeated beforehand, [1, Hq, T, 128]
        sq = qc.transpose(0, 1)[None]
        sk, sv = (t.reshape(T, Hkv, 128).repeat_interleave(g, 1).transpose(0, 1)[None].contiguous() for t in (k, v))
        mask = None
        if B > 1:
            seq = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(lens, device=dev))
            pos = torch.arange(T, device=dev)
            mask = (seq[:, None] == seq[None, :]) & (pos[None, :] <= pos[:, None])
        sdpa = torch.nn.functional.scaled_dot_product_attention

        calls = {"dense_attention": lambda: mixedgemm.dense_attention(q, k, v, indptr),
                 "paged_prefill bf16": lambda: mixedgemm.paged_prefill(qc, data, None, kv_indptr, pages, last, indptr, 0, max(lens), workspace=ws),
                 "torch SDPA": lambda: sdpa(sq, sk, sv, attn_mask=mask, is_causal=mask is None)}
        outs = {n: c().reshape(-1, T, 128).float() if n == "torch SDPA" else c().transpose(0, 1).float() for n, c in calls.items()}
        diffs = {n: float((outs[n] - outs["dense_attention"]).abs().max()) for n in calls if n != "dense_attention"}
        assert max(diffs.values()) < 0.05, f"the contenders disagree: {diffs}"
        graphs = {n: graph_of(c) for n, c in calls.items()}
        us = {n: [] for n in calls}
        for _ in range(REPEATS):
            for n, gr in graphs.items():
                us[n].append(replay_us(gr))
        lines.append(f"{name}: T {T}, Hq {Hq}, Hkv {Hkv}, {flops / 1e9:.1f} GFLOP; max |o - dense_attention|: "
                     + ", ".join(f"{n} {d:.4f}" for n, d in diffs.items()))
        for n, t in us.items():
            med = float(np.median(t))
            rows_out.append(dict(shape=name, call=n, median_us=round(med, 1), min_us=round(min(t), 1), max_us=round(max(t), 1),
                                 tflops=round(flops / med / 1e6, 1)))
            lines.append(f"    {n:20} {med:9.1f} ({min(t):.1f} .. {max(t):.1f}) us  {flops / med / 1e6:7.1f} TF/s")
        del graphs, outs, mask
        torch.cuda.empty_cache()

    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows_out))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_dense_attention.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows_out)}\n")


if __name__ == "__main__":
    main()
