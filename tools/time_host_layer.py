"""Eager host cost of the mixedgemm wrappers, one tree per process: prints 'name us' lines (profiles/host_layer_refactor_ab.txt,
profiles/binding_refactor_host_path.txt).  Public API only, so it runs on any tree.
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
# the paged-cache, attention, verification, sampling and MoE wrappers at the shapes of tests/test_wrapper_errors_kv_moe_gpu.py: an int4
# cache of 4 pages, 2 layers, 2 kv heads, page size 16; B = 2, Hq = 4, T = 3 new tokens; logits [3, 64]; MoE T = 4, E = 2, top_k = 2, H = 128
ints = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)
kv = (torch.zeros((4, 2, 2, 2, 16, 64), dtype=torch.uint8, device=dev), torch.zeros((4, 2, 2, 2, 16, 2), dtype=torch.float16, device=dev))
table_ = (ints(0, 2, 3), ints(0, 1, 2), ints(2, 5))          # kv_indptr, kv_indices, last_page_len: 18 and 5 tokens
indptr, k3, v3, q3, q2, cos, sin = ints(0, 2, 3), rnd(3, 2, 128), rnd(3, 2, 128), rnd(3, 4, 128), rnd(2, 4, 128), rnd(3, 128), rnd(3, 128)
tree = torch.tensor([1, 3, 1], dtype=torch.int64, device=dev)
pages, moves, groups = (ints(0, 2), ints(3, 1), ints(16, 5)), (ints(0, 1, 1), ints(1), ints(0)), (ints(0, 1, 2), ints(0, 1), ints(0, 0))
logits, u = rnd(3, 64), torch.rand((3,), generator=g).to(dev)
temp, topk, topp = torch.full((3,), 0.7, device=dev), torch.full((3,), 5, dtype=torch.int32, device=dev), torch.full((3,), 0.9, device=dev)
toks = (ints(5, 6, 7), ints(5, 9, 7), ints(5, 7))
gate, xm, ys = rnd(4, 2), rnd(4, 128), rnd(8, 128)
ids, w = mg.moe_route(gate, 2)
eoffs, stok, slot = mg.moe_plan(ids, 2)
idx2 = torch.randperm(128, generator=g).to(torch.int16).to(dev)
w1, w3 = (mg.reorder_quantize_w4(rnd(128, K), o["idx"], *split) for _ in range(2))
gu_table = mg.moe_gate_up_table([o["idx"]] * 2, [w1] * 2, [w3] * 2, [idx2] * 2, split, dsplit)
qa = mg.moe_quantize(src, stok, eoffs, table)
cases.update({
    "kv_append": lambda: mg.kv_append(*kv, *table_, k3, v3, indptr, 1),
    "rope_kv_append": lambda: mg.rope_kv_append(*kv, *table_, q3, k3, v3, cos, sin, indptr, 1),
    "kv_copy_pages": lambda: mg.kv_copy_pages(*kv, *pages),
    "kv_move_rows": lambda: mg.kv_move_rows(*kv, table_[0], table_[1], *moves),
    "paged_decode@64": lambda: mg.paged_decode(q2, *kv, *table_, 1, 64),
    "paged_decode@64 window": lambda: mg.paged_decode(q2, *kv, *table_, 1, 64, window=4),
    "paged_decode_shared": lambda: mg.paged_decode_shared(q2, *kv, *table_, 1, *groups, 16, 64),
    "paged_prefill@64": lambda: mg.paged_prefill(q3, *kv, *table_, indptr, 1, 64),
    "paged_prefill@64 window": lambda: mg.paged_prefill(q3, *kv, *table_, indptr, 1, 64, window=4),
    "paged_prefill@64 tree": lambda: mg.paged_prefill(q3, *kv, *table_, indptr, 1, 64, tree_mask=tree),
    "argmax_rows": lambda: mg.argmax_rows(logits),
    "sample_rows": lambda: mg.sample_rows(logits, u),
    "sample_rows filters": lambda: mg.sample_rows(logits, u, temperature=temp, top_k=topk, top_p=topp),
    "verify_greedy": lambda: mg.verify_greedy(*toks, indptr, table_[0], table_[2], 16),
    "verify_greedy tree": lambda: mg.verify_greedy(*toks, indptr, table_[0], table_[2], 16, tree_mask=tree),
    "moe_route": lambda: mg.moe_route(gate, 2),
    "moe_plan": lambda: mg.moe_plan(ids, 2),
    "moe_gather": lambda: mg.moe_gather(xm, stok),
    "moe_combine": lambda: mg.moe_combine(ys, ids, w, slot),
    "moe_expert_table": lambda: mg.moe_expert_table([o["idx"]] * 2, [o["b"]] * 2, *split),
    "moe_gate_up_activate": lambda: mg.moe_gate_up_activate(qa, eoffs, gu_table, 4, dsplit),
})      # (moe_gate_up_table is built once per layer and spends its time in torch: not timed)
print("# tree", micromix_amd.__file__, flush=True)
for n, f in cases.items():
    timeit(n, f)
big = setup(1, 4096, 4096, 128, (2048, 1024, 1024), (128, 0, 0))
bs = (2048, 1024, 1024)
big_mm = il(big["qx"], big["b"])
timeit("matmul@1x4096x4096", lambda: mg.matmul(*big_mm))
timeit("qlinear_decode@1x4096x4096", lambda: mg.qlinear_decode(big["x"], big["idx"], *big["b"], *bs))
timeit("rmsnorm_quantize_x@1x4096", lambda: mg.rmsnorm_quantize_x(big["x"], big["nw"], 1e-5, big["idx"], *bs))
