"""Times the residual add fused into the RMSNorm quantizer and the decode launches against the form it replaces, in one run on one box.

(a) the stand-alone quantizer:

    unfused   s = x + r (torch)  ->  mm_rmsnorm_quantize(s)       two launches, three more passes over rows * K * 2 bytes
    fused     mm_add_rmsnorm_quantize(x, r) -> s, the six buffers  one launch

K = 4096, split (2048, 128, 1920).  Ten calls per hipGraph, so that the host's launch work is out of the figure; three repetitions of
every point in alternation (unfused, fused, unfused, ...), all printed, so that the spread is visible.  rows = 16 and 256 lie where
mm_rmsnorm_quantize takes its LDS-DMA ring kernel (rows <= 2 x CUs) and the fused form cannot; 2 x CUs and 2 x CUs + 1 are the two
sides of that threshold; 4096 is prefill.

(b) one Llama-3-8B layer's linears with both norms at M = 1 and M = 8 as one hipGraph (hidden 4096, q | k | v 6144, o_proj, gate | up
2 x 14336, down_proj; attention replaced by a slice of q): the two residual adds as torch launches in front of forward_norm / FusedMLP
against `residual=`.  Three repetitions in alternation.

    python tools/time_add_rmsnorm.py [a|b]
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from micromix_amd import _lib
lib = _lib.load(); dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
K, split = 4096, (2048, 128, 1920)
CALLS, REPLAYS, REPS = 10, 20, 3
cus = torch.cuda.get_device_properties(0).multi_processor_count
w = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev)
idx = torch.randperm(K, generator=g).to(torch.int16).to(dev)
u8 = lambda n: torch.empty((n,), dtype=torch.uint8, device=dev)


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = torch.cuda.current_stream().cuda_stream
        for _ in range(CALLS):
            fn(st)
    return graph


def time_us(graph):
    graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (REPLAYS * CALLS) * 1000


which = sys.argv[1] if len(sys.argv) > 1 else "ab"
print(f"{torch.cuda.get_device_name(0)}, {cus} CUs; K = {K}, split {split}; us per call, {CALLS} calls per graph, {REPLAYS} replays", flush=True)
for rows in (16, 256, 2 * cus, 2 * cus + 1, 4096) if "a" in which else ():
    x = torch.randn((rows, K), generator=g).to(torch.bfloat16).to(dev)
    r = torch.randn((rows, K), generator=g).to(torch.bfloat16).to(dev)
    s = torch.empty_like(x)
    sf = [(rows // 128 + 1) * 128 * (k // 32) for k in split]
    o = [u8(rows * split[0] // 2), u8(rows * split[1] // 4 * 3), u8(rows * split[2])] + [u8(n) for n in sf]
    ptrs = [t.data_ptr() for t in o]

    def unfused(st):
        torch.add(x, r, out=s)
        assert lib.mm_rmsnorm_quantize(s.data_ptr(), w.data_ptr(), 1e-5, rows, K, idx.data_ptr(), *split, 0, *ptrs, st) == 0

    def fused(st):
        assert lib.mm_add_rmsnorm_quantize(x.data_ptr(), r.data_ptr(), s.data_ptr(), w.data_ptr(), 1e-5, rows, K, idx.data_ptr(), *split, 0, *ptrs, st) == 0

    def norm_only(st):
        assert lib.mm_rmsnorm_quantize(x.data_ptr(), w.data_ptr(), 1e-5, rows, K, idx.data_ptr(), *split, 0, *ptrs, st) == 0

    graphs = {"torch add + rmsnorm_quantize": graph_of(unfused), "add_rmsnorm_quantize": graph_of(fused), "(rmsnorm_quantize alone)": graph_of(norm_only)}
    times = {n: [] for n in graphs}
    for _ in range(REPS):
        for n, gr in graphs.items():
            times[n].append(time_us(gr))
    for n, t in times.items():
        print(f"rows={rows:5d}  {n:30s} " + "  ".join(f"{v:7.2f}" for v in t), flush=True)

if "b" in which:
    from micromix_amd.qlinear import FusedMLP, FusedQLinear, QLinearLayer
    H, INTER, DOWN = 4096, 14336, (7168, 512, 6656)
    lin = lambda n, k=H: torch.nn.Linear(k, n, bias=False, dtype=torch.bfloat16).to(dev)
    q = lambda l, i: QLinearLayer(l, p8_num=split[2], p6_num=split[1], reorder_index=i)
    i1, i2, i3 = (torch.randperm(H, generator=g) for _ in range(3))
    qkv = FusedQLinear([q(lin(4096), i1), q(lin(1024), i1), q(lin(1024), i1)])
    o_proj = q(lin(H), i2)
    mlp = FusedMLP(q(lin(INTER), i3), q(lin(INTER), i3), (0.02 * torch.randn((H, INTER), generator=g)).to(torch.bfloat16), DOWN)
    w_in, w_post = w, w.clone()
    CALLS = 1
    for M in (1, 8):
        x = torch.randn((1, M, H), generator=g).to(torch.bfloat16).to(dev)
        res = torch.randn((1, M, H), generator=g).to(torch.bfloat16).to(dev)

        def torch_adds(st):
            s1 = x + res
            qq, kk, vv = qkv.forward_norm(s1, w_in, 1e-5)
            a = o_proj(qq)
            s2 = a + s1
            return mlp(s2, w_post, 1e-5), s2

        def fused_adds(st):
            (qq, kk, vv), s1 = qkv.forward_norm(x, w_in, 1e-5, residual=res)
            a = o_proj(qq)
            return mlp(a, w_post, 1e-5, residual=s1)

        ya, yb = torch_adds(None), fused_adds(None)
        torch.cuda.synchronize()
        assert torch.equal(ya[0], yb[0]) and torch.equal(ya[1], yb[1])
        graphs = {"torch adds": graph_of(torch_adds), "residual= (fused)": graph_of(fused_adds)}
        times = {n: [] for n in graphs}
        for _ in range(REPS):
            for n, gr in graphs.items():
                times[n].append(time_us(gr))
        for n, t in times.items():
            print(f"layer linears + both norms, M={M}  {n:20s} " + "  ".join(f"{v:7.2f}" for v in t), flush=True)
print("done", flush=True)
