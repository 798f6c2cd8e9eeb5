"""Qwen3's QK-norm inside the RoPE kernels on the MI355X: each normed op against the op without the norm and against the chain it replaces.

    python tools/time_qknorm.py [out.txt]            (default: profiles/time_qknorm.txt)

Qwen3-8B heads (Hq 32, Hkv 8, head_dim 128), page size 16, shuffled pages, one layer, the three kinds.  append_rope at T = 1, 64 and
4 096 tokens of one sequence, append_rope(dense=True) at T = 4 096, decode_step at batch x cached tokens 1 x 4 096, 1 x 32 768,
8 x 4 096 and 64 x 1 024 (tools/time_decode_step.py's shapes and method: its helpers are used).  Three contenders, each captured as a
hipGraph of STEPS steps and replayed in alternation, REPEATS times after WARM warm-up replays, device events around each replay:
  plain   the op without the norm: the kernels it runs are instruction for instruction the parent commit's
  normed  the op with qk_norm=
  hf      the chain the normed op replaces: HF's Qwen3RMSNorm in torch on the q and k views (float, pow, mean, add, rsqrt, mul, to, mul,
          the last writing into a second packed projection), then the plain op
A line gives us per step: the median and the min .. max over the replays.  normed and hf are compared first (q, or o): they may differ
where HF's order of the sum moves a bf16 output, and the line counts the elements.  Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from micromix_amd import mixedgemm  # noqa: E402
from time_decode_step import HKV, KINDS, REPEATS, SHAPES, STEPS, WARM, graph_of, make_cache, rand, replay_us  # noqa: E402

HQ, EPS = 32, 1e-6
APPENDS = (("append_rope", 1), ("append_rope", 64), ("append_rope", 4096), ("append_rope dense", 4096))


def hf_norm(x, w, out):
    """HF's Qwen3RMSNorm.forward on x [T, H, 128], the last product written into `out`"""
    h = x.float()
    h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS)
    return torch.mul(w, h.to(torch.bfloat16), out=out)


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"us per call: median (min .. max) of {REPEATS} replays, in alternation, of a hipGraph of {STEPS} calls, after {WARM} warm-up "
             f"replays; Hq {HQ}, Hkv {HKV}, P 16, shuffled pages"]
    out = []
    norm = (1 + 0.25 * rand((128,), gen, dev), 1 + 0.25 * rand((128,), gen, dev), EPS)
    for kind in KINDS:
        for what, shape in (*APPENDS, *(("decode_step", s) for s in SHAPES)):
            step = what == "decode_step"
            B, n = shape if step else (1, shape)
            T = B if step else n
            caches = []
            data, param, tbl = make_cache(kind, B, n, dev, gen)
            for _ in range(3):
                caches.append((data.clone(), None if param is None else param.clone()))
            del data, param
            packed = rand((T, (HQ + 2 * HKV) * 128), gen, dev, 2.0)
            packed2 = packed.clone()
            split = lambda p: (p[:, : HQ * 128], p[:, HQ * 128: (HQ + HKV) * 128], p[:, (HQ + HKV) * 128:])
            (q, k, v), (q2, k2, v2) = split(packed), split(packed2)
            ang = torch.rand((T, 128), generator=gen, device=dev) * 6.28
            cos, sin = ang.cos().to(torch.bfloat16), ang.sin().to(torch.bfloat16)
            app = torch.arange(B + 1, dtype=torch.int32, device=dev) if step else torch.tensor([0, T], dtype=torch.int32, device=dev)
            ws = [torch.empty((max(mixedgemm.rope_append_decode_workspace_bytes(B, HQ, HKV, n), 16),), dtype=torch.uint8, device=dev) for _ in range(3)]

            def op(i, q, k, v, **kw):
                if step:
                    return mixedgemm.rope_append_decode(*caches[i], *tbl, q, k, v, cos, sin, 0, n, workspace=ws[i], **kw)
                if what.endswith("dense"):
                    return mixedgemm.rope_kv_append_dense(*caches[i], *tbl, q, k, v, cos, sin, app, 0, **kw)[0]
                return mixedgemm.rope_kv_append(*caches[i], *tbl, q, k, v, cos, sin, app, 0, **kw)

            def hf():
                hf_norm(q.view(T, HQ, 128), norm[0], q2.view(T, HQ, 128))
                hf_norm(k.view(T, HKV, 128), norm[1], k2.view(T, HKV, 128))
                return op(2, q2, k2, v2)

            graphs = {"plain": graph_of(lambda: op(0, q, k, v)), "normed": graph_of(lambda: op(1, q, k, v, qk_norm=norm)), "hf": graph_of(hf)}
            for _ in range(WARM):
                for g, _ in graphs.values():
                    g.replay()
            torch.cuda.synchronize()
            differ = int((graphs["normed"][1].view(torch.int16) != graphs["hf"][1].view(torch.int16)).sum())
            us = {m: [] for m in graphs}
            for _ in range(REPEATS):
                for m, (g, _) in graphs.items():
                    us[m].append(replay_us(g))
            med = {m: float(np.median(u)) for m, u in us.items()}
            lines.append(f"-- {kind:8} {what:17} {B:2} x {n:5}: normed against hf, {differ} of {graphs['hf'][1].numel()} output elements differ")
            for m in graphs:
                lines.append(f"   {m:7}{med[m]:9.2f} ({min(us[m]):.2f} .. {max(us[m]):.2f})" +
                             (f"   normed - plain = {med['normed'] - med['plain']:+.2f} us, hf / normed = {med['hf'] / med['normed']:.2f}" if m == "hf" else ""))
            out.append(dict(kind=kind, op=what, batch=B, tokens=n, differ=differ, **{m + "_us": [round(u, 2) for u in us[m]] for m in us}))
            del graphs, caches
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_qknorm.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(out)}\n")


if __name__ == "__main__":
    main()
