"""Eager host cost of the mixedgemm wrappers, one tree per process: prints 'name us' lines (profiles/host_layer_refactor_ab.txt).
The tree is the micromix_amd package found first on PYTHONPATH, with its own built library; to compare two commits run them in turn,
each in a fresh process:  PYTHONPATH=<tree> python tools/time_host_layer.py [calls]"""
import sys, time, statistics, torch
from micromix_amd import mixedgemm as mg
import micromix_amd
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(5)
rnd = lambda *s: torch.randn(s, generator=g).to(torch.bfloat16).to(dev)
CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 3000

def setup(M, K, N, I, split, dsplit):
    o = {"x": rnd(M, K), "r": rnd(M, K), "nw": rnd(K), "idx": torch.randperm(K, generator=g).to(torch.int16).to(dev), "gub": rnd(M, 2 * I)}
    o["b"] = mg.reorder_quantize_w4(rnd(N, K), o["idx"], *split)
    o["gu"] = mg.interleave_gate_up(mg.reorder_quantize_w4(rnd(I, K), o["idx"], *split), mg.reorder_quantize_w4(rnd(I, K), o["idx"], *split))
    o["down"] = mg.downproj_quantize_w4(rnd(N, I), *dsplit)
    o["qx"] = mg.reorder_quantize_x(o["x"], o["idx"], *split)
    return o

def timeit(name, f):
    for _ in range(200):
        f()
    torch.cuda.synchronize()
    meds = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            f()
        torch.cuda.synchronize()
        meds.append((time.perf_counter() - t0) / CALLS * 1e6)
    print(f"{name} {statistics.median(meds):.3f}", flush=True)

M, K, N, I, split, dsplit = 2, 256, 128, 128, (128, 128, 0), (128, 0, 0)
o = setup(M, K, N, I, split, dsplit)
il = lambda a, b: [t for p in zip(a, b) for t in p]
src, offs = rnd(4, K), torch.tensor([0, 2, 4], dtype=torch.int32, device=dev)
table = mg.moe_expert_table([o["idx"]] * 2, [o["b"]] * 2, *split)
qsrc = mg.moe_quantize(src, None, offs, table)
mm_args = il(o["qx"], o["b"])
cases = {
    "matmul": lambda: mg.matmul(*mm_args),
    "reorder_quantize_x": lambda: mg.reorder_quantize_x(o["x"], o["idx"], *split),
    "activate_quantize_x": lambda: mg.activate_quantize_x(o["x"], o["r"], *split),
    "rmsnorm_quantize_x": lambda: mg.rmsnorm_quantize_x(o["x"], o["nw"], 1e-5, o["idx"], *split),
    "add_rmsnorm_quantize_x": lambda: mg.add_rmsnorm_quantize_x(o["x"], o["r"], o["nw"], 1e-5, o["idx"], *split),
    "gate_up_activate": lambda: mg.gate_up_activate(o["qx"], o["gu"], *dsplit),
    "gate_up_activate_decode": lambda: mg.gate_up_activate_decode(o["x"], o["idx"], o["gu"], *dsplit),
    "rmsnorm_gate_up_activate_decode": lambda: mg.rmsnorm_gate_up_activate_decode(o["x"], o["nw"], 1e-5, o["idx"], o["gu"], *dsplit),
    "add_rmsnorm_gate_up_activate_decode": lambda: mg.add_rmsnorm_gate_up_activate_decode(o["x"], o["r"], o["nw"], 1e-5, o["idx"], o["gu"], *dsplit),
    "down_activate_decode": lambda: mg.down_activate_decode(o["gub"], o["down"], *dsplit),
    "qlinear_decode": lambda: mg.qlinear_decode(o["x"], o["idx"], *o["b"], *split),
    "rmsnorm_qlinear_decode": lambda: mg.rmsnorm_qlinear_decode(o["x"], o["nw"], 1e-5, o["idx"], *o["b"], *split),
    "add_rmsnorm_qlinear_decode": lambda: mg.add_rmsnorm_qlinear_decode(o["x"], o["r"], o["nw"], 1e-5, o["idx"], *o["b"], *split),
    "reorder_quantize_x_grouped": lambda: mg.reorder_quantize_x_grouped([o["x"], o["r"]], [o["idx"]] * 2, *split),
    "matmul_grouped": lambda: mg.matmul_grouped([o["qx"]] * 2, [o["b"]] * 2),
    "moe_quantize": lambda: mg.moe_quantize(src, None, offs, table),
    "moe_activate_quantize": lambda: mg.moe_activate_quantize(src, src, offs, table),
    "moe_matmul": lambda: mg.moe_matmul(qsrc, offs, table, 4),
}
print("# tree", micromix_amd.__file__, flush=True)
for n, f in cases.items():
    timeit(n, f)
big = setup(1, 4096, 4096, 128, (2048, 1024, 1024), (128, 0, 0))
bs = (2048, 1024, 1024)
big_mm = il(big["qx"], big["b"])
timeit("matmul@1x4096x4096", lambda: mg.matmul(*big_mm))
timeit("qlinear_decode@1x4096x4096", lambda: mg.qlinear_decode(big["x"], big["idx"], *big["b"], *bs))
timeit("rmsnorm_quantize_x@1x4096", lambda: mg.rmsnorm_quantize_x(big["x"], big["nw"], 1e-5, big["idx"], *bs))
