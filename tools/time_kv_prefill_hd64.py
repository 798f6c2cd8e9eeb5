"""Times causal multi-token attention over the paged cache for 64-wide heads (include/micromix_kv_prefill_hd64.h) on Llama-3.2-1B
heads (Hq 32, Hkv 8), P = 16, shuffled pages, bf16 and fp8.

    python tools/time_kv_prefill_hd64.py --build-ablation     # no GPU: links tools/_build/libmicromix_prefill_rows128.so
    python tools/time_kv_prefill_hd64.py [out.txt]            # on the GPU; the forced-128-rows line appears when that library exists

Protocol of tools/time_kv_hd64.py: us per call inside a hipGraph of 10 calls, device events, warmed up, the contenders' graphs replayed
in turn in one process, median (min .. max) of 9, the merge launch charged.  DESIGN 7c's five shapes (sequences x new tokens over held
tokens): 1 x 4 096 over 0; 1 x 512 over 32 256; 8 ragged prompts of 300 .. 700 over 0; 64 x 5 over 1 019; 64 x 1 over 1 023.  Contenders:
(a) paged_prefill on the 64-wide cache, bf16 and fp8; (a128) the bf16 call on the ablation library, whose plan always takes the 128-row
kernel; (b) paged_prefill on a 128-wide bf16 cache holding the same rows zero-padded, sm_scale 1/8, without and with the copies that
pad q and the layer's cache charged; (c) torch SDPA after repeat_kv under the explicit bottom-right mask (one sequence at a time is
not timed: equal-length shapes only); (d) dense_attention [T, H, 64] on the square shape; (e) paged_decode on the last shape."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ABLATION = os.path.join(ROOT, "tools", "_build", "libmicromix_prefill_rows128.so")


def build_ablation():
    from micromix_amd import build
    build.build(verbose=False)                                   # the product objects the ablation library shares
    os.makedirs(os.path.dirname(ABLATION), exist_ok=True)
    src, obj = "kv_prefill_hd64.hip", os.path.join(os.path.dirname(ABLATION), "kv_prefill_hd64_rows128.o")
    subprocess.check_call([build.hipcc(), *build.FLAGS, *build.SOURCE_FLAGS[src], "-DMM_KV_PREFILL_HD64_FORCE_ROWS=128", "-c",
                           os.path.join(build.CSRC, src), "-o", obj])
    objs = [obj if s == src else os.path.join(build.OBJDIR, s.replace(".hip", ".o")) for s in build.SOURCES]
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-fno-gpu-rdc", *objs, "-o", ABLATION])
    print(ABLATION)


def main(out_path):
    import numpy as np
    import torch
    from micromix_amd import _lib, mixedgemm
    from micromix_amd.kvcache import PagedKVCache

    dev, Hq, Hkv, P, CALLS, REPS = torch.device("cuda:0"), 32, 8, 16, 10, 9
    g, lines = Hq // Hkv, []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def graph_of(fn):
        fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(CALLS):
                fn()
        return gr

    def race(contenders):
        """{name: fn} -> {name: (median, min, max)} in us per call: the graphs replayed in turn, REPS times after three warm rounds"""
        graphs = {n: graph_of(f) for n, f in contenders.items()}
        times = {n: [] for n in graphs}
        for rep in range(REPS + 3):
            for n, gr in graphs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                gr.replay()
                b.record()
                b.synchronize()
                if rep >= 3:
                    times[n].append(a.elapsed_time(b) * 1e3 / CALLS)
        return {n: (float(np.median(t)), min(t), max(t)) for n, t in times.items()}

    rows128 = _lib._bind(ctypes.CDLL(ABLATION), _lib._KV_PREFILL_HD64_PROTOS) if os.path.exists(ABLATION) else None
    say(f"paged prefill, head_dim 64: Hq {Hq}, Hkv {Hkv}, P {P}, shuffled pages; us per call in a hipGraph of {CALLS}, median (min .. max) of {REPS}")
    say(f"ablation library (-DMM_KV_PREFILL_HD64_FORCE_ROWS=128): {'present' if rows128 else 'absent: row (a128) not run'}")
    rng = np.random.default_rng(0)
    ragged = [int(n) for n in rng.integers(300, 701, 8)]
    shapes = [("1 x 4096 square", [0], [4096]), ("512 over 32768", [32256], [512]), ("8 ragged prompts 300..700", [0] * 8, ragged),
              ("64 x 5 over 1024", [1019] * 64, [5] * 64), ("64 x 1 over 1024", [1023] * 64, [1] * 64)]
    for name, prior, new in shapes:
        B, T, lens = len(new), sum(new), [p + n for p, n in zip(prior, new)]
        need = [-(-n // P) for n in lens]
        pages, bound = sum(need), max(lens)
        tbl = [torch.tensor(np.concatenate([[0], np.cumsum(need)]), dtype=torch.int32, device=dev),
               torch.from_numpy(rng.permutation(pages).astype(np.int32)).to(dev),
               torch.tensor([n - (c - 1) * P for n, c in zip(lens, need)], dtype=torch.int32, device=dev)]
        qo = torch.tensor(np.concatenate([[0], np.cumsum(new)]), dtype=torch.int32, device=dev)
        vals = torch.randn((pages, 1, 2, Hkv, P, 64), device=dev).to(torch.bfloat16)
        fp8 = PagedKVCache(1, Hkv, P, pages, B, kind="fp8_e4m3", device=dev, head_dim=64)
        e = torch.ceil(torch.log2(vals.float().abs().amax(-1, keepdim=True) / 448.0)).clamp(-14, 15)
        fp8.kv_data.copy_((vals.float() * torch.exp2(-e)).to(torch.float8_e4m3fn))
        fp8.kv_param[..., 0:1] = torch.exp2(e).to(torch.float16)
        q = torch.randn((T, Hq, 64), device=dev).to(torch.bfloat16)
        wide, qw = torch.zeros((pages, 1, 2, Hkv, P, 128), dtype=torch.bfloat16, device=dev), torch.zeros((T, Hq, 128), dtype=torch.bfloat16, device=dev)
        wide[..., :64], qw[..., :64] = vals, q
        ws = torch.empty((max(mixedgemm.paged_prefill_hd64_workspace_bytes(T, B, Hq, Hkv, bound), mixedgemm.paged_prefill_workspace_bytes(T, B, Hq, Hkv, bound),
                              rows128.mm_paged_prefill_hd64_workspace_bytes(T, B, Hq, Hkv, bound) if rows128 else 0, 16),), dtype=torch.uint8, device=dev)
        o = torch.empty((T, Hq, 64), dtype=torch.bfloat16, device=dev)

        def forced():
            st = rows128.mm_paged_prefill_hd64(q.data_ptr(), qo.data_ptr(), T, vals.data_ptr(), None, _lib.MM_KV_BF16, pages, 1, 0, Hkv, P,
                                               *(t.data_ptr() for t in tbl), B, Hq, bound, 0.0, ws.data_ptr(), ws.numel(), o.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream)
            assert st == 0, st

        def padded_with_copies():
            wide[..., :64].copy_(vals)
            qw[..., :64].copy_(q)
            return mixedgemm.paged_prefill(qw, wide, None, *tbl, qo, 0, bound, sm_scale=0.125, workspace=ws)[..., :64].contiguous()

        runs = {"(a) bf16": lambda: mixedgemm.paged_prefill(q, vals, None, *tbl, qo, 0, bound, workspace=ws),
                "(a) fp8": lambda: mixedgemm.paged_prefill(q, fp8.kv_data, fp8.kv_param, *tbl, qo, 0, bound, workspace=ws)}
        if rows128:
            runs["(a128) bf16, 128 rows forced"] = forced
        runs["(b) 128-wide padded"] = lambda: mixedgemm.paged_prefill(qw, wide, None, *tbl, qo, 0, bound, sm_scale=0.125, workspace=ws)
        runs["(b+) ... with the copies"] = padded_with_copies
        if len(set(lens)) == 1 and len(set(new)) == 1:           # (c): contiguous K, V [B, Hkv, len, 64] and the explicit bottom-right mask
            order = tbl[1].long().view(B, -1)
            kc, vc = (vals[order, 0, w].permute(0, 2, 1, 3, 4).reshape(B, Hkv, -1, 64)[:, :, : lens[0]].contiguous() for w in (0, 1))
            mask = torch.arange(lens[0], device=dev)[None, :] <= (prior[0] + torch.arange(new[0], device=dev))[:, None]
            qs = q.view(B, new[0], Hq, 64).transpose(1, 2)
            runs["(c) torch SDPA, explicit mask"] = lambda: torch.nn.functional.scaled_dot_product_attention(
                qs, kc.repeat_interleave(g, 1), vc.repeat_interleave(g, 1), attn_mask=mask, scale=0.125)
            if prior[0] == 0 and B == 1:
                kd, vd = kc[0].transpose(0, 1).contiguous(), vc[0].transpose(0, 1).contiguous()
                runs["(d) dense_attention [T, H, 64]"] = lambda: mixedgemm.dense_attention(q, kd, vd)
        if set(new) == {1}:
            wsd = torch.empty((max(mixedgemm.paged_decode_hd64_workspace_bytes(B, Hq, Hkv, bound), 16),), dtype=torch.uint8, device=dev)
            runs["(e) paged_decode"] = lambda: mixedgemm.paged_decode(q, vals, None, *tbl, 0, bound, workspace=wsd)
        say()
        say(f"{name}: T {T}, plan {tuple(mixedgemm.paged_prefill_hd64_plan(T, B, Hq, Hkv, bound))} (rows, tile tokens, tiles, chunks, chunk length)")
        for n, t in race(runs).items():
            say(f"  {n:32s} {t[0]:9.1f} ({t[1]:.1f} .. {t[2]:.1f}) us")
        del vals, wide, fp8, runs
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if "--build-ablation" in sys.argv:
        build_ablation()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else None)
