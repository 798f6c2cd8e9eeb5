"""The cache-less route for 64-wide heads (mixedgemm.dense_attention / dense_attention_window / rope_qk given [T, H, 64] tensors) on the
MI355X, against what the same call had before: the 128-wide kernel on zero-padded copies, and torch.

    python tools/time_dense_attention_hd64.py [out.txt]            (default: profiles/time_dense_attention_hd64.txt)

Shapes: Llama-3.2-1B heads (Hq 32, Hkv 8, head_dim 64) at 1 x 2 048, 1 x 4 096, 8 ragged prompts of 300-700 tokens, and 1 x 8 192 with a
window of 4 096.  Contenders:
  (a)  the new call, q, k, v read in place as [T, H, 64] views of one packed projection;
  (b)  q, k, v zero-padded to 128 columns, dense_attention(_window) at 128 with sm_scale = 1/8, the result sliced: the padded operands made
       beforehand (copies not charged) and the three pads plus the slice inside the timed call (copies charged);
  (c)  torch SDPA after repeat_kv, not charged; is_causal when square, a boolean mask when ragged or windowed.
And rope_qk at T = 4 096 against HF's apply_rotary_pos_emb chain in torch bf16.
us per call inside a hipGraph of ITERS calls between device events, after a warm-up; the contenders' graphs are replayed in turn, REPEATS
times: median (min .. max).  TF/s on the causal FLOPs 4 * 64 * Hq * sum(i + 1) (the band's when windowed).  The outputs are compared
first.  Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd import mixedgemm  # noqa: E402

ITERS, WARM, REPEATS, HQ, HKV = 10, 2, 9, 32, 8


def shapes():
    rng = np.random.default_rng(0)
    return [("1 x 2048", [2048], 0), ("1 x 4096", [4096], 0), ("8 ragged 300-700", rng.integers(300, 701, 8).tolist(), 0),
            ("1 x 8192, W 4096", [8192], 4096)]


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


def contest(calls, lines, rows_out, shape, flops=None):
    """the graphs of `calls` replayed in turn; one line and one record per contender"""
    graphs = {n: graph_of(c) for n, c in calls.items()}
    us = {n: [] for n in calls}
    for _ in range(REPEATS):
        for n, gr in graphs.items():
            us[n].append(replay_us(gr))
    first = float(np.median(next(iter(us.values()))))
    for n, t in us.items():
        med = float(np.median(t))
        rate = f"  {flops / med / 1e6:7.1f} TF/s" if flops else ""
        rows_out.append(dict(shape=shape, call=n, median_us=round(med, 1), min_us=round(min(t), 1), max_us=round(max(t), 1),
                             ratio_to_first=round(med / first, 2), **({"tflops": round(flops / med / 1e6, 1)} if flops else {})))
        lines.append(f"    {n:44} {med:9.1f} ({min(t):.1f} .. {max(t):.1f}) us{rate}  x{med / first:.2f}")


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(1)
    lines = [f"us per call: median (min .. max) over {REPEATS} alternated replays of a hipGraph of {ITERS} calls; TF/s on the causal FLOPs; "
             "x: time / time of (a)"]
    rows_out = []
    pad = torch.nn.functional.pad
    sdpa = torch.nn.functional.scaled_dot_product_attention
    for name, lens, W in shapes():
        T, B, g = sum(lens), len(lens), HQ // HKV
        flops = sum(4 * 64 * HQ * (n * (n + 1) // 2 - (max(n - W, 0) * (max(n - W, 0) + 1) // 2 if W else 0)) for n in lens)
        packed = torch.randn((T, (HQ + 2 * HKV) * 64), generator=gen).to(torch.bfloat16).to(dev)
        q, k, v = (t.unflatten(1, (-1, 64)) for t in (packed[:, :HQ * 64], packed[:, HQ * 64:(HQ + HKV) * 64], packed[:, (HQ + HKV) * 64:]))
        indptr = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)

        def at128(q_, k_, v_):
            if W:
                return mixedgemm.dense_attention_window(q_, k_, v_, W, indptr, 0.125)
            return mixedgemm.dense_attention(q_, k_, v_, indptr, 0.125)

        qp, kp, vp = (pad(t, (0, 64)) for t in (q, k, v))
        sq = q.transpose(0, 1)[None]
        sk, sv = (t.repeat_interleave(g, 1).transpose(0, 1)[None].contiguous() for t in (k, v))
        mask = None
        if B > 1 or W:
            seq = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(lens, device=dev))
            pos = torch.arange(T, device=dev)
            mask = (seq[:, None] == seq[None, :]) & (pos[None, :] <= pos[:, None]) & ((pos[None, :] > pos[:, None] - W) if W else True)
        calls = {"(a) hd64 kernel": (lambda: mixedgemm.dense_attention_window(q, k, v, W, indptr)) if W else (lambda: mixedgemm.dense_attention(q, k, v, indptr)),
                 "(b) 128 kernel on padded copies, uncharged": lambda: at128(qp, kp, vp),
                 "(b) 128 kernel, 3 pads + slice charged": lambda: at128(pad(q, (0, 64)), pad(k, (0, 64)), pad(v, (0, 64)))[..., :64].contiguous(),
                 "(c) torch SDPA after repeat_kv": lambda: sdpa(sq, sk, sv, attn_mask=mask, is_causal=mask is None)}
        outs = {n: c() for n, c in calls.items()}
        ref = outs["(a) hd64 kernel"].float()
        diffs = {n: float(((o[0].transpose(0, 1) if n.startswith("(c)") else o[..., :64]).float() - ref).abs().max()) for n, o in outs.items()
                 if not n.startswith("(a)")}
        assert max(diffs.values()) < 0.05, f"the contenders disagree: {diffs}"
        lines.append(f"{name}: T {T}, Hq {HQ}, Hkv {HKV}, head_dim 64, {flops / 1e9:.1f} GFLOP; max |o - (a)|: "
                     + ", ".join(f"{n[:3]} {d:.4f}" for n, d in diffs.items()))
        contest(calls, lines, rows_out, name, flops)
        del outs, mask, calls
        torch.cuda.empty_cache()

    # RoPE at T = 4096: the HIP call against HF's chain in torch bf16 (x * cos + rotate_half(x) * sin for q and for k)
    T = 4096
    packed = torch.randn((T, (HQ + 2 * HKV) * 64), generator=gen).to(torch.bfloat16).to(dev)
    q, k = packed[:, :HQ * 64].unflatten(1, (-1, 64)), packed[:, HQ * 64:(HQ + HKV) * 64].unflatten(1, (-1, 64))
    cos, sin = (torch.randn((T, 64), generator=gen).to(torch.bfloat16).to(dev) for _ in range(2))

    def hf_chain():
        c, s = cos[:, None, :], sin[:, None, :]
        return tuple(x * c + torch.cat((-x[..., 32:], x[..., :32]), dim=-1) * s for x in (q, k))

    same = all(torch.equal(a, b) for a, b in zip(mixedgemm.rope_qk(q, k, cos, sin), hf_chain()))
    lines.append(f"rope_qk: T {T}, Hq {HQ}, Hkv {HKV}, head_dim 64; bit-equal to the torch chain: {same}")
    contest({"rope_qk (mm_rope_qk_hd64)": lambda: mixedgemm.rope_qk(q, k, cos, sin), "HF apply_rotary_pos_emb, torch bf16": hf_chain},
            lines, rows_out, "rope_qk 4096")

    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows_out))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_dense_attention_hd64.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows_out)}\n")


if __name__ == "__main__":
    main()
