"""Times the paged KV cache for 64-wide heads (include/micromix_kv_hd64.h) on Llama-3.2-1B heads (Hq 32, Hkv 8), P = 16, shuffled pages.

    python tools/time_kv_hd64.py --build-ablation     # no GPU: links tools/_build/libmicromix_nodepth.so (-DMM_KV_HD64_NO_DEPTH)
    python tools/time_kv_hd64.py [out.txt]            # on the GPU; the ablation rows appear when that library exists

Protocol of tools/time_kv_decode.py and DESIGN 7z: us per call inside a hipGraph of 10 calls, device events, warmed up, the contenders'
graphs replayed in turn in one process, median (min .. max) of 9.  Decode, B x T in 1 x 4 096, 1 x 32 768, 8 x 4 096, 64 x 1 024, merge
charged: (a) paged_decode on the 64-wide cache, bf16 and fp8, with TB/s on its own cache bytes; (a-) the same entry of the ablation
library, which issues tile n + 1's loads after tile n's p.V; (b) paged_decode on a 128-wide bf16 cache holding the same K and V
zero-padded, sm_scale = 1/8; (c) torch SDPA after repeat_kv on contiguous K, V.  Then append_rope at 64 x 1 token and at 1 x 4 096 against
torch RoPE + index copies, and one layer's prefill_fresh at 1 x 4 096."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ABLATION = os.path.join(ROOT, "tools", "_build", "libmicromix_nodepth.so")


def build_ablation():
    from micromix_amd import build
    build.build(verbose=False)                                   # the product objects the ablation library shares
    os.makedirs(os.path.dirname(ABLATION), exist_ok=True)
    obj = os.path.join(os.path.dirname(ABLATION), "kv_hd64_nodepth.o")
    subprocess.check_call([build.hipcc(), *build.FLAGS, "-DMM_KV_HD64_NO_DEPTH", "-c", os.path.join(build.CSRC, "kv_hd64.hip"), "-o", obj])
    objs = [obj if s == "kv_hd64.hip" else os.path.join(build.OBJDIR, s.replace(".hip", ".o")) for s in build.SOURCES]
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-fno-gpu-rdc", *objs, "-o", ABLATION])
    print(ABLATION)


def main(out_path):
    import numpy as np
    import torch
    from micromix_amd import _lib, mixedgemm
    from micromix_amd.kvcache import PagedKVCache

    dev, Hq, Hkv, P, CALLS, REPS = torch.device("cuda:0"), 32, 8, 16, 10, 9
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def graph_of(fn):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(CALLS):
                fn()
        return g

    def race(contenders):
        """{name: fn} -> {name: (median, min, max)} in us per call: the graphs replayed in turn, REPS times after three warm rounds"""
        graphs = {n: graph_of(f) for n, f in contenders.items()}
        times = {n: [] for n in graphs}
        for rep in range(REPS + 3):
            for n, g in graphs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                g.replay()
                b.record()
                b.synchronize()
                if rep >= 3:
                    times[n].append(a.elapsed_time(b) * 1e3 / CALLS)
        return {n: (float(np.median(t)), min(t), max(t)) for n, t in times.items()}

    def fmt(t):
        return f"{t[0]:8.1f} ({t[1]:.1f} .. {t[2]:.1f})"

    nodepth = None
    if os.path.exists(ABLATION):
        nodepth = _lib._bind(ctypes.CDLL(ABLATION), _lib._KV_HD64_PROTOS)
    say(f"paged KV cache, head_dim 64: Hq {Hq}, Hkv {Hkv}, P {P}, shuffled pages; us per call in a hipGraph of {CALLS}, median (min .. max) of {REPS}")
    say(f"ablation library (-DMM_KV_HD64_NO_DEPTH): {'present' if nodepth else 'absent: rows (a-) not run'}")
    say()
    rng = np.random.default_rng(0)
    for B, T in ((1, 4096), (1, 32768), (8, 4096), (64, 1024)):
        pages = B * T // P
        indptr = torch.arange(B + 1, dtype=torch.int32, device=dev) * (T // P)
        indices = torch.from_numpy(rng.permutation(pages).astype(np.int32)).to(dev)
        last = torch.full((B,), P, dtype=torch.int32, device=dev)
        vals = torch.randn((pages, 1, 2, Hkv, P, 64), device=dev).to(torch.bfloat16)
        fp8 = PagedKVCache(1, Hkv, P, pages, B, kind="fp8_e4m3", device=dev, head_dim=64)
        amax = vals.float().abs().amax(-1, keepdim=True)
        e = torch.ceil(torch.log2(amax / 448.0)).clamp(-14, 15)
        fp8.kv_data.copy_((vals.float() * torch.exp2(-e)).to(torch.float8_e4m3fn))
        fp8.kv_param[..., 0:1] = torch.exp2(e).to(torch.float16)
        wide = torch.zeros((pages, 1, 2, Hkv, P, 128), dtype=torch.bfloat16, device=dev)
        wide[..., :64] = vals
        q = torch.randn((B, Hq, 64), device=dev).to(torch.bfloat16)
        qw = torch.zeros((B, Hq, 128), dtype=torch.bfloat16, device=dev)
        qw[..., :64] = q
        order = indices.long().view(B, T // P)
        kc, vc = (vals[order, 0, w].permute(0, 2, 1, 3, 4).reshape(B, Hkv, T, 64).contiguous() for w in (0, 1))
        ws = torch.empty((max(mixedgemm.paged_decode_hd64_workspace_bytes(B, Hq, Hkv, T), mixedgemm.paged_decode_workspace_bytes(B, Hq, Hkv, T), 16),),
                         dtype=torch.uint8, device=dev)
        o = torch.empty((B, Hq, 64), dtype=torch.bfloat16, device=dev)

        def raw(lib, data, param, kind):
            stream = torch.cuda.current_stream(dev).cuda_stream
            st = lib.mm_paged_decode_hd64(q.data_ptr(), data.data_ptr(), param.data_ptr() if param is not None else None, kind, pages, 1, 0, Hkv, P,
                                          indptr.data_ptr(), indices.data_ptr(), last.data_ptr(), B, Hq, T, 0.0, ws.data_ptr(), ws.numel(),
                                          o.data_ptr(), stream)
            assert st == 0, st

        runs = {"(a) bf16": lambda: mixedgemm.paged_decode(q, vals, None, indptr, indices, last, 0, T, workspace=ws),
                "(a) fp8": lambda: mixedgemm.paged_decode(q, fp8.kv_data, fp8.kv_param, indptr, indices, last, 0, T, workspace=ws)}
        if nodepth:
            runs["(a-) bf16 no depth"] = lambda: raw(nodepth, vals, None, _lib.MM_KV_BF16)
            runs["(a-) fp8 no depth"] = lambda: raw(nodepth, fp8.kv_data, fp8.kv_param, _lib.MM_KV_FP8_E4M3)
        runs["(b) 128-wide padded"] = lambda: mixedgemm.paged_decode(qw, wide, None, indptr, indices, last, 0, T, sm_scale=0.125, workspace=ws)
        runs["(c) torch SDPA"] = lambda: torch.nn.functional.scaled_dot_product_attention(
            q[:, :, None], kc.repeat_interleave(Hq // Hkv, 1), vc.repeat_interleave(Hq // Hkv, 1), scale=0.125)
        nc, cl = mixedgemm.paged_decode_hd64_plan(B, Hkv, T)
        say(f"decode {B} x {T}: {nc} chunks of {cl}")
        bytes_of = {"(a) bf16": vals.numel() * 2, "(a) fp8": vals.numel() + vals.numel() // 64 * 4}
        bytes_of.update({"(a-) bf16 no depth": bytes_of["(a) bf16"], "(a-) fp8 no depth": bytes_of["(a) fp8"]})
        for n, t in race(runs).items():
            say(f"  {n:22s} {fmt(t)} us" + (f"   {bytes_of[n] / t[0] / 1e6:5.2f} TB/s of its cache bytes" if n in bytes_of else ""))
        del vals, wide, kc, vc, fp8
    say()
    for B, n in ((64, 1), (1, 4096)):
        T = B * n
        for kind in ("bf16", "fp8_e4m3"):
            cache = PagedKVCache(1, Hkv, P, -(-T // P) + B, B, kind=kind, device=dev, head_dim=64)
            cache.extend(n)
            qkv = torch.randn((T, (Hq + 2 * Hkv) * 64), device=dev).to(torch.bfloat16)
            x = [qkv[:, a * 64: b * 64].view(T, -1, 64) for a, b in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv))]
            cos, sin = (torch.randn((T, 64), device=dev).to(torch.bfloat16) for _ in range(2))
            runs = {f"append_rope {kind}": lambda: cache.append_rope(0, *x, cos, sin)}
            if kind == "bf16":
                rows = torch.arange(T, device=dev)
                flat = cache.kv_data.view(-1, 2, Hkv, P, 64)

                def torch_way():
                    rot = lambda t: t * cos[:, None] + torch.cat([-t[..., 32:], t[..., :32]], -1) * sin[:, None]
                    qr, kr = rot(x[0]), rot(x[1])
                    flat[rows // P, 0, :, rows % P] = kr
                    flat[rows // P, 1, :, rows % P] = x[2]
                    return qr
                runs["torch RoPE + index copies (bf16)"] = torch_way
                if n > 1:
                    runs["prefill_fresh bf16 (append + dense attention)"] = lambda: cache.prefill_fresh(0, *x, cos, sin)
            say(f"append {B} x {n} token(s), {kind}")
            for name, t in race(runs).items():
                say(f"  {name:46s} {fmt(t)} us")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if "--build-ablation" in sys.argv:
        build_ablation()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else None)
