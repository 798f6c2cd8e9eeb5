"""What the paged-cache, attention, verification, sampling and MoE wrappers refuse, wrapper by wrapper, and which C entries their
valid calls reach: the sibling of tests/test_wrapper_errors_gpu.py for the wrappers that file does not cover.  Each bad call carries
the exception type and the message the wrapper has always raised (the expressions are the message literals of mixedgemm.py before
these wrappers shared their checks), and raises before a launch; where two things are wrong at once the earlier check speaks.  One
valid call per wrapper, and per cache kind, checks the shapes and dtypes that come back.  test_wrapper_calls_its_entries runs the
valid calls, and their `window=` / `tree_mask=` forms, over a recording stand-in for the library and holds the sequence of mm_*
symbols to tests/golden/wrapper_entries_v1.json (tools/record_wrapper_entries.py): an un-windowed call stays on the un-windowed
entry, a workspace query included.

The smallest shapes the entries take: a cache of 4 pages, 2 layers, 2 kv heads, page size 16, head dim 128 as int4, fp8 and bf16;
B = 2 sequences, Hq = 4, T = 3 new tokens; logits [3, 64]; MoE T = 4 tokens, E = 2, top_k = 2, H = 128, expert tables at K = 256 split
(128, 128, 0)."""
import json
import os

import pytest
import torch

from micromix_amd import _lib, mixedgemm as mg

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wrapper_entries_v1.json")
PAGES, L, HKV, P, B, HQ, T, ROWS, VOCAB = 4, 2, 2, 16, 2, 4, 3, 3, 64
MT, E, TOPK, H, K, I = 4, 2, 2, 128, 256, 128
NSLOT = MT * TOPK
SPLIT, SPLIT2 = (128, 128, 0), (128, 0, 0)
LONG = 1024                                   # a max_seq_len at which decode and prefill split the tokens and need a workspace
BF, U8, I32, I64, F32 = torch.bfloat16, torch.uint8, torch.int32, torch.int64, torch.float32
KINDS = ("int4", "fp8", "bf16")


# ---- the bad operands: a default operand, changed ----
def f32(t):
    return t.float()


def i64(t):
    return t.long()


def cpu(t):
    return t.cpu()


def nc(t):
    """the same shape and dtype, every stride doubled"""
    return torch.stack((t, t), dim=-1)[..., 0]


def val(v):
    return lambda _: v


def new(shape, dtype):
    return lambda t: torch.zeros(shape, dtype=dtype, device="cuda:0")


def first(change):
    """a 6-tuple with its first tensor changed"""
    return lambda six: (change(six[0]), *six[1:])


def narrow(six):
    return (six[0][:, :-4].contiguous(), *six[1:])


def short(six):
    return (*six[:3], six[3][:-1], *six[4:])


def dtype_of(name, want="bfloat16", got="float32"):
    return (TypeError, rf"{name} must be torch\.{want}, got torch\.{got}")


def cpu_of(name):
    return (RuntimeError, rf"{name} must be a device tensor \(HIP\); the MicroMix ops have no CPU path")


def contiguous_of(name):
    return (RuntimeError, rf"{name} must be contiguous")


def runtime(text):
    return (RuntimeError, text)


def value(text):
    return (ValueError, text)


HEADS = runtime(r"the 3 query heads are not a multiple of the cache's 2 kv heads")
WORKSPACE = runtime(r"workspace must be a contiguous device tensor of at least \d+ bytes on cuda:0")
SM_SCALE = value(r"sm_scale must be positive")
WINDOW = value(r"window must be None, 0 \(no window\) or a positive token count")
LAYER = runtime(r"layer_idx 2 outside the cache's 2 layers")
INT4_SHAPE = runtime(r"kv_data with a kv_param must be \[max_pages, L, 2, Hkv, P, 64\] uint8 \(int4\) or \[max_pages, L, 2, Hkv, P, 128\] "
                     r"uint8 / float8_e4m3fn \(fp8\); a bf16 cache \[max_pages, L, 2, Hkv, P, 128\] takes kv_param None")
BF16_SHAPE = runtime(r"bf16 kv_data \(kv_param None\) must be \[max_pages, L, 2, Hkv, P, 128\]; an int4 cache \(\[\.\.\., 64\] uint8\) and an "
                     r"fp8 cache \(\[\.\.\., 128\] uint8 / float8_e4m3fn\) need their fp16 kv_param")
PARAM_SHAPE = runtime(r"kv_param must be \[max_pages, L, 2, Hkv, P, 2\] fp16, matching kv_data")
INDPTR = runtime(r"kv_indptr must have B \+ 1 entries \(B = last_page_len\.numel\(\)\)")
LOGITS_2D = runtime(r"logits must be \[rows, vocab\] with vocab >= 1")
LOGITS_STRIDE = runtime(r"logits must have unit stride along the vocabulary \(the rows may be any distance >= vocab apart\)")
LOGITS_OVERLAP = runtime(r"logits rows overlap: row stride 0 < vocab 64")
ROUNDING = value(r"rounding must be 'reference' or 'fused'")
SPLIT_OF = lambda what: runtime(rf"Value error in run_{what}: KN, KS, KO must be non-negative multiples of 128 that sum to K")
# the cache checks every cache wrapper makes, on an int4 cache (kv_data of the wrong kind is the bf16 message, and the other way round)
CACHE = [({"kv_data": cpu}, cpu_of("kv_data")), ({"kv_data": f32}, dtype_of("kv_data", "uint8")), ({"kv_data": nc}, contiguous_of("kv_data")),
         ({"kv_param": f32}, dtype_of("kv_param", "float16")), ({"kv_param": cpu}, cpu_of("kv_param")),
         ({"kv_param": val(None)}, dtype_of("kv_data", "bfloat16", "uint8")),
         ({"kv_data": new((PAGES, L, 2, HKV, P, 32), U8)}, INT4_SHAPE), ({"kv_data": new((PAGES, L, 2, HKV, P, 64), BF), "kv_param": val(None)}, BF16_SHAPE),
         ({"kv_param": new((PAGES, L, 2, HKV, P), torch.float16)}, PARAM_SHAPE)]
TABLE = [({"kv_indptr": i64}, dtype_of("kv_indptr", "int32", "int64")), ({"kv_indices": cpu}, cpu_of("kv_indices")),
         ({"last_page_len": nc}, contiguous_of("last_page_len")), ({"kv_indptr": new((B,), I32)}, INDPTR), ({"layer_idx": val(2)}, LAYER),
         ({"layer_idx": val(-1)}, runtime(r"layer_idx -1 outside the cache's 2 layers"))]
QUERY = [({"q": f32}, dtype_of("q")), ({"q": cpu}, cpu_of("q")), ({"q": nc}, contiguous_of("q"))]


@pytest.fixture(scope="module")
def o(dev):
    return operands(dev)


def operands(dev):
    """every operand, built once"""
    g = torch.Generator().manual_seed(7)
    rnd = lambda *shape: torch.randn(shape, generator=g).to(BF).to(dev)
    ints = lambda *v: torch.tensor(v, dtype=I32, device=dev)
    t = {"cache": {"int4": (torch.zeros((PAGES, L, 2, HKV, P, 64), dtype=U8, device=dev), torch.zeros((PAGES, L, 2, HKV, P, 2), dtype=torch.float16, device=dev)),
                   "fp8": (torch.zeros((PAGES, L, 2, HKV, P, 128), dtype=U8, device=dev), torch.zeros((PAGES, L, 2, HKV, P, 2), dtype=torch.float16, device=dev)),
                   "bf16": (torch.zeros((PAGES, L, 2, HKV, P, 128), dtype=BF, device=dev), None)},
         # sequence 0 holds 18 tokens on pages 0, 1, sequence 1 holds 5 on page 2; the last 2 and 1 of them are the T = 3 new ones
         "kv_indptr": ints(0, 2, 3), "kv_indices": ints(0, 1, 2), "last_page_len": ints(2, 5), "append_indptr": ints(0, 2, 3), "qo_indptr": ints(0, 2, 3),
         "layer_idx": 1, "max_seq_len": 64, "k": rnd(T, HKV, 128), "v": rnd(T, HKV, 128), "q3": rnd(T, HQ, 128), "q2": rnd(B, HQ, 128),
         "cos": rnd(T, 128), "sin": rnd(T, 128), "tree_mask": torch.tensor([1, 3, 1], dtype=I64, device=dev),
         "src_pages": ints(0, 2), "dst_pages": ints(3, 1), "rows": ints(16, 5), "move_indptr": ints(0, 1, 1), "src_pos": ints(1), "dst_pos": ints(0),
         "group_indptr": ints(0, 1, 2), "group_members": ints(0, 1), "shared_len": ints(0, 0), "max_shared_len": 16, "max_suffix_len": 64,
         "logits": rnd(ROWS, VOCAB), "u": torch.rand((ROWS,), generator=g).to(dev),
         "target_tok": ints(5, 6, 7), "draft_tok": ints(5, 9, 7), "root_tok": ints(5, 7), "page_size": P,
         "gate_logits": rnd(MT, E), "top_k": TOPK, "num_experts": E, "x": rnd(MT, H), "y_sorted": rnd(NSLOT, H), "src": rnd(MT, K),
         "idx": torch.randperm(K, generator=g).to(torch.int16).to(dev), "idx2": torch.randperm(I, generator=g).to(torch.int16).to(dev),
         "max_rows": MT, "split2": SPLIT2}
    t["w1"], t["w3"] = (mg.reorder_quantize_w4(rnd(I, K), t["idx"], *SPLIT) for _ in range(2))
    t["reorder_indices"], t["Bs"], t["w3s"], t["reorder_indices2"] = [t["idx"]] * E, [t["w1"]] * E, [t["w3"]] * E, [t["idx2"]] * E
    t["split"], t["bias"] = SPLIT, rnd(I)
    t["topk_ids"], t["topk_w"] = mg.moe_route(t["gate_logits"], TOPK)
    t["expert_offsets"], t["sorted_token"], t["slot_of"] = mg.moe_plan(t["topk_ids"], E)
    t["table1"] = mg.moe_expert_table(t["reorder_indices"], t["Bs"], *SPLIT)
    t["table"] = mg.moe_gate_up_table(t["reorder_indices"], t["Bs"], t["w3s"], t["reorder_indices2"], SPLIT, SPLIT2)
    t["A"] = mg.moe_quantize(t["src"], t["sorted_token"], t["expert_offsets"], t["table1"])
    good = mg.moe_gate_up_activate(t["A"], t["expert_offsets"], t["table"], MT, SPLIT2)
    t["out_narrow"], t["out_short"] = narrow(good), short(good)
    torch.cuda.synchronize()
    return t


# wrapper -> (positional parameters, keyword parameters, operands that differ from the fixture's names); an operand is o[name]
CACHE_ARGS = ("kv_data", "kv_param", "kv_indptr", "kv_indices", "last_page_len")
SIGNATURES = {
    "kv_append": ((*CACHE_ARGS, "k", "v", "append_indptr", "layer_idx"), (), {}),
    "rope_kv_append": ((*CACHE_ARGS, "q", "k", "v", "cos", "sin", "append_indptr", "layer_idx"), (), {"q": "q3"}),
    "kv_copy_pages": (("kv_data", "kv_param", "src_pages", "dst_pages", "rows"), (), {}),
    "kv_move_rows": (("kv_data", "kv_param", "kv_indptr", "kv_indices", "move_indptr", "src_pos", "dst_pos"), (), {}),
    "paged_decode": (("q", *CACHE_ARGS, "layer_idx", "max_seq_len", "sm_scale", "workspace"), ("window",), {"q": "q2"}),
    "paged_decode_shared": (("q", *CACHE_ARGS, "layer_idx", "group_indptr", "group_members", "shared_len", "max_shared_len", "max_suffix_len", "sm_scale",
                             "workspace"), ("out",), {"q": "q2"}),
    "paged_prefill": (("q", *CACHE_ARGS, "qo_indptr", "layer_idx", "max_seq_len", "sm_scale", "workspace"), ("window", "tree_mask"), {"q": "q3", "tree_mask": None}),
    "argmax_rows": (("logits",), ("out", "workspace"), {}),
    "sample_rows": (("logits", "u"), ("temperature", "top_k", "top_p", "min_p", "out", "workspace"), {"top_k": None}),
    "verify_greedy": (("target_tok", "draft_tok", "root_tok", "qo_indptr", "kv_indptr", "last_page_len", "page_size"),
                      ("tree_mask", "result", "move_src", "move_dst"), {"tree_mask": None}),
    "moe_route": (("logits", "top_k"), ("topk_ids", "topk_w"), {"logits": "gate_logits", "topk_ids": None, "topk_w": None}),
    "moe_plan": (("topk_ids", "num_experts"), ("expert_offsets", "sorted_token", "slot_of"), {"expert_offsets": None, "sorted_token": None, "slot_of": None}),
    "moe_gather": (("x", "sorted_token"), ("out",), {}),
    "moe_combine": (("y_sorted", "topk_ids", "topk_w", "slot_of"), ("out",), {}),
    "moe_expert_table": (("reorder_indices", "Bs", "KN", "KS", "KO", "biases"), (), {}),
    "moe_gate_up_table": (("reorder_indices", "Bs", "w3s", "reorder_indices2", "split", "split2"), ("biases1", "biases3"), {}),
    "moe_gate_up_activate": (("A", "expert_offsets", "table", "max_rows", "split2"), ("rounding", "out"), {}),
}


def call(name, o, kind="int4", **changes):
    """mixedgemm.<name> on the fixture's operands, `changes` applied to them: {parameter: function of the default operand, or the name of
    another operand of the fixture}"""
    positional, keywords, renamed = SIGNATURES[name]
    a = dict(o, KN=SPLIT[0], KS=SPLIT[1], KO=SPLIT[2], kv_data=o["cache"][kind][0], kv_param=o["cache"][kind][1])
    a.update({p: (o[src] if src is not None else None) for p, src in renamed.items()})
    for p, change in changes.items():
        a[p] = a[change] if isinstance(change, str) else change(a.get(p))
    return getattr(mg, name)(*(a.get(p) for p in positional), **{p: a[p] for p in keywords if a.get(p) is not None})


OUT3, OUT2 = [((T, HQ, 128), BF)], [((B, HQ, 128), BF)]
IDX = [((ROWS,), I32)]
MOE_SF = (NSLOT // 128 + E) * 128 * (128 // 32)
# wrapper -> (what a valid call returns: None or [(shape, dtype)]; the bad calls, in the wrapper's own order of checks where two are wrong)
WRAPPERS = {
    "kv_append": (None, CACHE + TABLE + [
        ({"append_indptr": i64}, dtype_of("append_indptr", "int32", "int64")), ({"k": f32}, dtype_of("k")), ({"v": cpu}, cpu_of("v")), ({"k": nc}, contiguous_of("k")),
        ({"k": new((T, HKV, 64), BF)}, runtime(r"k and v must both be \[T, 2, 128\] bf16")), ({"v": new((T + 1, HKV, 128), BF)}, runtime(r"k and v must both be \[T, 2, 128\] bf16")),
        ({"append_indptr": new((B,), I32)}, runtime(r"append_indptr must have B \+ 1 entries")),
        ({"layer_idx": val(2), "k": f32}, LAYER)]),
    "rope_kv_append": (OUT3, CACHE + TABLE + [
        ({"append_indptr": nc}, contiguous_of("append_indptr")), ({"append_indptr": new((B,), I32)}, runtime(r"append_indptr must have B \+ 1 entries")),
        ({"q": f32}, dtype_of("q")), ({"cos": cpu}, cpu_of("cos")), ({"sin": f32}, dtype_of("sin")),
        ({"q": new((T, HQ, 64), BF)}, runtime(r"q must be \[T, H, 128\] or \[T, H \* 128\] bf16")), ({"k": new((T, HQ, 128), BF)}, runtime(r"k has 4 heads, the cache has 2")),
        ({"v": new((T + 1, HKV, 128), BF)}, runtime(r"q, k and v must hold the same T tokens")), ({"q": new((T, 3, 128), BF)}, HEADS),
        ({"cos": new((T, 64), BF)}, runtime(r"cos and sin must both be \[T = 3, 128\] \(or \[bsz, q_len, 128\] with bsz \* q_len = T\) bf16")),
        ({"append_indptr": new((B,), I32), "q": f32}, runtime(r"append_indptr must have B \+ 1 entries"))]),
    "kv_copy_pages": (None, CACHE + [
        ({"src_pages": i64}, dtype_of("src_pages", "int32", "int64")), ({"dst_pages": cpu}, cpu_of("dst_pages")), ({"rows": nc}, contiguous_of("rows")),
        ({"dst_pages": new((3,), I32)}, runtime(r"src_pages, dst_pages and rows must be one-dimensional and of one length")),
        ({"rows": new((2, 1), I32)}, runtime(r"src_pages, dst_pages and rows must be one-dimensional and of one length")),
        ({"src_pages": i64, "dst_pages": new((3,), I32)}, dtype_of("src_pages", "int32", "int64"))]),
    "kv_move_rows": (None, CACHE + [
        ({"kv_indptr": i64}, dtype_of("kv_indptr", "int32", "int64")), ({"move_indptr": cpu}, cpu_of("move_indptr")), ({"kv_indices": nc}, contiguous_of("kv_indices")),
        ({"src_pos": new((1, 1), I32)}, runtime(r"src_pos must be one-dimensional")),
        ({"move_indptr": new((B,), I32)}, runtime(r"kv_indptr and move_indptr must both have B \+ 1 entries")),
        ({"dst_pos": new((2,), I32)}, runtime(r"src_pos and dst_pos must be of one length")),
        ({"move_indptr": new((B,), I32), "dst_pos": new((2,), I32)}, runtime(r"kv_indptr and move_indptr must both have B \+ 1 entries"))]),
    "paged_decode": (OUT2, QUERY + CACHE + TABLE + [
        ({"window": val(-1)}, WINDOW), ({"q": new((T, HQ, 128), BF)}, runtime(r"q must be \[B = 2, Hq, 128\] bf16")), ({"q": new((B, 3, 128), BF)}, HEADS),
        ({"max_seq_len": val(-1)}, runtime(r"max_seq_len must be >= 0")), ({"max_seq_len": val(LONG), "workspace": new((16,), U8)}, WORKSPACE),
        ({"max_seq_len": val(LONG), "workspace": lambda _: torch.zeros((1 << 20,), dtype=U8)}, WORKSPACE),
        ({"sm_scale": val(0.0)}, SM_SCALE), ({"sm_scale": val(-1.0)}, SM_SCALE),
        ({"window": val(-1), "q": f32}, WINDOW), ({"q": new((B, 3, 128), BF), "sm_scale": val(0.0)}, HEADS)]),
    "paged_decode_shared": (OUT2, QUERY + CACHE + TABLE + [
        ({"q": new((T, HQ, 128), BF)}, runtime(r"q must be \[B = 2, Hq, 128\] bf16")), ({"q": new((B, 3, 128), BF)}, HEADS),
        ({"group_indptr": i64}, dtype_of("group_indptr", "int32", "int64")), ({"shared_len": cpu}, cpu_of("shared_len")),
        ({"group_indptr": new((B,), I32)}, runtime(r"group_indptr must be a one-dimensional int32 tensor of 3 entries \(B = 2\)")),
        ({"group_members": new((B + 1,), I32)}, runtime(r"group_members must be a one-dimensional int32 tensor of 2 entries \(B = 2\)")),
        ({"max_shared_len": val(-1)}, runtime(r"max_shared_len and max_suffix_len must lie in \[0, 2\^29\]")),
        ({"max_suffix_len": val((1 << 29) + 1)}, runtime(r"max_shared_len and max_suffix_len must lie in \[0, 2\^29\]")),
        ({"workspace": new((16,), U8)}, WORKSPACE), ({"out": new((B, HQ, 64), BF)}, runtime(r"out must be \[2, 4, 128\] bf16")),
        ({"out": new((B, HQ, 128), F32)}, dtype_of("out")), ({"sm_scale": val(0.0)}, SM_SCALE),
        ({"group_indptr": new((B,), I32), "out": new((B, HQ, 64), BF)}, runtime(r"group_indptr must be a one-dimensional int32 tensor of 3 entries \(B = 2\)"))]),
    "paged_prefill": (OUT3, QUERY + CACHE + TABLE + [
        ({"window": val(-1)}, WINDOW),
        ({"window": val(4), "tree_mask": lambda _: torch.ones((T,), dtype=I64, device="cuda:0")},
         value(r"paged_prefill has no sliding-window form of the tree mask: pass window or tree_mask, not both")),
        ({"qo_indptr": i64}, dtype_of("qo_indptr", "int32", "int64")), ({"qo_indptr": new((B,), I32)}, runtime(r"qo_indptr must have B \+ 1 entries \(B = last_page_len\.numel\(\)\)")),
        ({"q": new((T, HQ, 64), BF)}, runtime(r"q must be \[T, Hq, 128\] bf16, T = qo_indptr\[-1\]")), ({"q": new((T, 3, 128), BF)}, HEADS),
        ({"tree_mask": new((T,), I32)}, dtype_of("tree_mask", "int64", "int32")),
        ({"tree_mask": new((T + 1,), I64)}, runtime(r"tree_mask must be a one-dimensional int64 tensor of T = 3 words")),
        ({"max_seq_len": val(-1)}, runtime(r"max_seq_len must be >= 0")), ({"max_seq_len": val(LONG), "workspace": new((16,), U8)}, WORKSPACE),
        ({"sm_scale": val(0.0)}, SM_SCALE),
        ({"qo_indptr": new((B,), I32), "q": new((T, 3, 128), BF)}, runtime(r"qo_indptr must have B \+ 1 entries \(B = last_page_len\.numel\(\)\)"))]),
    "argmax_rows": (IDX, [
        ({"logits": val(None)}, (TypeError, r"logits must be a torch\.Tensor")), ({"logits": f32}, dtype_of("logits")), ({"logits": cpu}, cpu_of("logits")),
        ({"logits": new((VOCAB,), BF)}, LOGITS_2D), ({"logits": lambda t: torch.cat((t, t), 1)[:, ::2]}, LOGITS_STRIDE), ({"logits": lambda t: t[:1].expand(ROWS, VOCAB)}, LOGITS_OVERLAP),
        ({"out": new((ROWS,), I64)}, dtype_of("out", "int32", "int64")), ({"out": new((ROWS + 1,), I32)}, runtime(r"out must be int32 \[3\]")),
        ({"logits": f32, "out": new((ROWS + 1,), I32)}, dtype_of("logits"))]),
    "sample_rows": (IDX, [
        ({"logits": val(None)}, (TypeError, r"logits must be a torch\.Tensor")), ({"logits": f32}, dtype_of("logits")), ({"logits": cpu}, cpu_of("logits")),
        ({"logits": new((VOCAB,), BF)}, LOGITS_2D), ({"logits": lambda t: torch.cat((t, t), 1)[:, ::2]}, LOGITS_STRIDE), ({"logits": lambda t: t[:1].expand(ROWS, VOCAB)}, LOGITS_OVERLAP),
        ({"u": val(None)}, (TypeError, r"u must be a torch\.float32 device tensor \[3\] \(torch\.rand\), got NoneType")),
        ({"u": val(0.5)}, (TypeError, r"u must be a torch\.float32 device tensor \[3\] \(torch\.rand\), got float")),
        ({"u": lambda t: t.double()}, dtype_of("u", "float32", "float64")), ({"u": cpu}, cpu_of("u")), ({"u": nc}, contiguous_of("u")),
        ({"u": new((ROWS + 1,), F32)}, runtime(r"u must be torch\.float32 \[3\], one entry per row")),
        ({"temperature": val("hot")}, (TypeError, r"temperature must be None, a number or a torch\.float32 device tensor \[3\], got str")),
        ({"top_p": val(True)}, (TypeError, r"top_p must be None, a number or a torch\.float32 device tensor \[3\], got bool")),
        ({"top_k": val(2.0)}, (TypeError, r"top_k must be an int or a torch\.int32 device tensor \[3\], got float")),
        ({"top_k": new((ROWS,), I64)}, dtype_of("top_k", "int32", "int64")), ({"min_p": new((ROWS, 1), F32)}, runtime(r"min_p must be torch\.float32 \[3\], one entry per row")),
        ({"out": new((ROWS,), I64)}, dtype_of("out", "int32", "int64")), ({"out": new((ROWS + 1,), I32)}, runtime(r"out must be int32 \[3\]")),
        ({"workspace": new((16,), U8)}, WORKSPACE),
        ({"u": new((ROWS + 1,), F32), "out": new((ROWS + 1,), I32)}, runtime(r"u must be torch\.float32 \[3\], one entry per row"))]),
    "verify_greedy": ([((B, 66), I32), ((T,), I32), ((T,), I32)], [
        ({"target_tok": i64}, (TypeError, r"target_tok must be torch\.int32, got torch\.int64: convert it with target_tok\.to\(torch\.int32\)")),
        ({"root_tok": i64}, (TypeError, r"root_tok must be torch\.int32, got torch\.int64: convert it with root_tok\.to\(torch\.int32\)")),
        ({"target_tok": cpu}, cpu_of("target_tok")), ({"draft_tok": lambda t: t.short()}, dtype_of("draft_tok", "int32", "int16")), ({"draft_tok": cpu}, cpu_of("draft_tok")),
        ({"qo_indptr": nc}, contiguous_of("qo_indptr")), ({"root_tok": new((B, 1), I32)}, runtime(r"root_tok must be one-dimensional")),
        ({"draft_tok": new((T + 1,), I32)}, runtime(r"target_tok and draft_tok must be of one length")),
        ({"qo_indptr": new((B,), I32)}, runtime(r"qo_indptr and kv_indptr must have B \+ 1 entries and last_page_len B \(B = root_tok\.numel\(\)\)")),
        ({"last_page_len": new((B + 1,), I32)}, runtime(r"qo_indptr and kv_indptr must have B \+ 1 entries and last_page_len B \(B = root_tok\.numel\(\)\)")),
        ({"page_size": val(0)}, value(r"page_size must be positive")), ({"tree_mask": new((T,), I32)}, dtype_of("tree_mask", "int64", "int32")),
        ({"tree_mask": new((T + 1,), I64)}, runtime(r"tree_mask must be int64 \[3\], one word per row")),
        ({"result": new((B, 64), I32)}, runtime(r"result must be int32 \[2, 66\]")), ({"result": new((B, 66), I64)}, dtype_of("result", "int32", "int64")),
        ({"move_src": new((T + 1,), I32)}, runtime(r"move_src must be int32 \[3\]")), ({"move_dst": new((T, 1), I32)}, runtime(r"move_dst must be int32 \[3\]")),
        ({"page_size": val(0), "result": new((B, 64), I32)}, value(r"page_size must be positive"))]),
    "moe_route": ([((MT, TOPK), I32), ((MT, TOPK), BF)], [
        ({"logits": f32}, dtype_of("logits")), ({"logits": cpu}, cpu_of("logits")), ({"logits": nc}, contiguous_of("logits")),
        ({"logits": new((MT, E, 1), BF)}, runtime(r"logits must be \[T, E\] bf16")), ({"topk_ids": new((MT, 1), I32)}, runtime(r"topk_ids must be \[4, 2\], got \[4, 1\]")),
        ({"topk_w": new((MT, TOPK), F32)}, dtype_of("topk_w")), ({"topk_ids": new((MT, TOPK), I64)}, dtype_of("topk_ids", "int32", "int64")),
        ({"topk_ids": new((MT, 1), I32), "topk_w": new((MT, TOPK), F32)}, runtime(r"topk_ids must be \[4, 2\], got \[4, 1\]"))]),
    "moe_plan": ([((E + 1,), I32), ((NSLOT,), I32), ((MT, TOPK), I32)], [
        ({"topk_ids": i64}, dtype_of("topk_ids", "int32", "int64")), ({"topk_ids": cpu}, cpu_of("topk_ids")), ({"topk_ids": nc}, contiguous_of("topk_ids")),
        ({"topk_ids": new((NSLOT,), I32)}, runtime(r"topk_ids must be \[T, top_k\] int32")), ({"expert_offsets": new((E,), I32)}, runtime(r"expert_offsets must be \[3\], got \[2\]")),
        ({"sorted_token": new((MT,), I32)}, runtime(r"sorted_token must be \[8\], got \[4\]")), ({"slot_of": new((TOPK, MT), I32)}, runtime(r"slot_of must be \[4, 2\], got \[2, 4\]")),
        ({"expert_offsets": new((E,), I32), "slot_of": new((TOPK, MT), I32)}, runtime(r"expert_offsets must be \[3\], got \[2\]"))]),
    "moe_gather": ([((NSLOT, H), BF)], [
        ({"x": f32}, dtype_of("x")), ({"x": cpu}, cpu_of("x")), ({"x": nc}, contiguous_of("x")), ({"x": new((MT, H, 1), BF)}, runtime(r"x must be \[T, H\] bf16")),
        ({"sorted_token": i64}, dtype_of("sorted_token", "int32", "int64")), ({"out": new((MT, H), BF)}, runtime(r"out must be \[8, 128\], got \[4, 128\]")),
        ({"sorted_token": i64, "out": new((MT, H), BF)}, dtype_of("sorted_token", "int32", "int64"))]),
    "moe_combine": ([((MT, H), BF)], [
        ({"y_sorted": f32}, dtype_of("y_sorted")), ({"y_sorted": cpu}, cpu_of("y_sorted")), ({"y_sorted": nc}, contiguous_of("y_sorted")),
        ({"topk_ids": i64}, dtype_of("topk_ids", "int32", "int64")), ({"y_sorted": new((MT, H), BF)}, runtime(r"topk_ids must be \[T, top_k\] and y_sorted \[T \* top_k, H\]")),
        ({"topk_w": new((MT, 1), BF)}, runtime(r"topk_w must be \[4, 2\], got \[4, 1\]")), ({"slot_of": new((NSLOT,), I32)}, runtime(r"slot_of must be \[4, 2\], got \[8\]")),
        ({"out": new((NSLOT, H), BF)}, runtime(r"out must be \[4, 128\], got \[8, 128\]")),
        ({"topk_w": new((MT, 1), BF), "out": new((NSLOT, H), BF)}, runtime(r"topk_w must be \[4, 2\], got \[4, 1\]"))]),
    "moe_expert_table": ("table", [
        ({"reorder_indices": lambda v: v[:1]}, value(r"1 <= E <= 64 experts, one reorder index \(and bias entry\) each")),
        ({"Bs": val([])}, value(r"1 <= E <= 64 experts, one reorder index \(and bias entry\) each")), ({"KS": val(100)}, SPLIT_OF("moe_expert_table")),
        ({"Bs": lambda v: [narrow(v[0]), v[1]]}, runtime(r"the packed weights of expert 0 do not match the split in either weight mode")),
        ({"reorder_indices": lambda v: [v[0].int(), v[1]]}, dtype_of(r"reorder_index\[0\]", "int16", "int32")),
        ({"reorder_indices": lambda v: [v[0], v[1][:128]]}, runtime(r"expert 1: the reorder index must have 256 entries")),
        ({"Bs": lambda v: [v[0], first(cpu)(v[1])]}, cpu_of("expert 1 weight operand")), ({"Bs": lambda v: [v[0], first(nc)(v[1])]}, contiguous_of("expert 1 weight operand")),
        ({"Bs": lambda v: [v[0], narrow(v[1])]}, runtime(r"expert 1: packed weights do not match N / split / weight mode of expert 0")),
        ({"Bs": lambda v: [v[0], short(v[1])]}, runtime(r"expert 1: packed weights do not match N / split / weight mode of expert 0")),
        ({"biases": lambda _: [None, torch.zeros((I + 1,), dtype=BF, device="cuda:0")]}, runtime(r"expert 1: bias must be a bfloat16 tensor with N elements")),
        ({"KS": val(100), "Bs": lambda v: [narrow(v[0]), v[1]]}, SPLIT_OF("moe_expert_table"))]),
    "moe_gate_up_table": ("table", [
        ({"w3s": lambda v: v[:1]}, value(r"moe_gate_up_table: 1 <= E <= 64 experts with w1, w3 and both reorder indices each")),
        ({"biases1": lambda _: [None, torch.zeros((I,), dtype=BF, device="cuda:0")]}, value(r"moe_gate_up_table: w1 / w3 must have no bias \(the fused epilogue adds none\)")),
        ({"Bs": lambda v: [tuple(t[:64] for t in v[0]), v[1]]}, value(r"moe_gate_up_table: I = 64 must be a multiple of 128")),
        ({"split2": val((100, 28, 0))}, value(r"moe_gate_up_table: split2 = \(100, 28, 0\) must be three non-negative multiples of 128 that add up to I = 128")),
        ({"split2": val((128, 128, 0))}, value(r"moe_gate_up_table: split2 = \(128, 128, 0\) must be three non-negative multiples of 128 that add up to I = 128")),
        ({"w3s": lambda v: [v[0], narrow(v[1])]}, value(r"moe_gate_up_table: expert 1: w3 must be fp4 weights \(MM_W_FP4\) of \[128, \.\] rows matching split1")),
        ({"Bs": lambda v: [v[0], short(v[1])]}, value(r"moe_gate_up_table: expert 1: a scale tensor of w1 holds fewer than _sf_bytes_w\(I, Kseg\) bytes")),
        ({"reorder_indices2": lambda v: [v[0][:64], v[1]]}, value(r"moe_gate_up_table: expert 0: w2's reorder index must have I = 128 entries")),
        ({"split2": val((100, 28, 0)), "w3s": lambda v: [v[0], narrow(v[1])]},
         value(r"moe_gate_up_table: split2 = \(100, 28, 0\) must be three non-negative multiples of 128 that add up to I = 128"))]),
    "moe_gate_up_activate": ([((NSLOT, 64), U8), ((NSLOT, 0), U8), ((NSLOT, 0), U8), ((MOE_SF,), U8), ((0,), U8), ((0,), U8)], [
        ({"rounding": val("bad")}, ROUNDING), ({"table": "table1"}, runtime(r"table must be a moe_gate_up_table \(N = 2 I, I a multiple of 128\)")),
        ({"split2": val((100, 28, 0))}, SPLIT_OF("moe_gate_up_activate")), ({"A": lambda six: tuple(t.cpu() for t in six)}, cpu_of("activation segment")),
        ({"A": first(nc)}, contiguous_of("activation segment")), ({"A": first(f32)}, dtype_of("activation segment", "uint8")),
        ({"A": narrow}, runtime(r"activation segment must be \[8, 64\], got \[8, 60\]")),
        ({"A": short}, runtime(r"an activation scale tensor is smaller than moe_sf_bytes\(n, E, Kseg\)")),
        ({"expert_offsets": new((E,), I32)}, runtime(r"expert_offsets must be \[3\], got \[2\]")),
        ({"out": "out_narrow"}, runtime(r"packed output must be \[8, 64\], got \[8, 60\]")),
        ({"out": "out_short"}, runtime(r"a scale output is smaller than moe_sf_bytes\(n, E, Kseg\)")),
        ({"rounding": val("bad"), "A": narrow}, ROUNDING), ({"split2": val((100, 28, 0)), "A": narrow}, SPLIT_OF("moe_gate_up_activate"))]),
}
# the valid calls: the plain one of every wrapper, and the forms that reach another entry
VARIANTS = {"paged_decode": {"": {}, "window": {"window": val(4)}, "workspace": {"max_seq_len": val(LONG)}, "window+long": {"window": val(4), "max_seq_len": val(LONG)}},
            "paged_prefill": {"": {}, "window": {"window": val(4)}, "tree_mask": {"tree_mask": lambda _: torch.tensor([1, 3, 1], dtype=I64, device="cuda:0")},
                              "workspace": {"max_seq_len": val(LONG)}},
            "verify_greedy": {"": {}, "tree_mask": {"tree_mask": lambda _: torch.tensor([1, 3, 1], dtype=I64, device="cuda:0")}},
            "sample_rows": {"": {}, "filters": {"temperature": val(0.7), "top_k": val(5), "top_p": val(0.9), "min_p": val(0.05)}},
            "kv_copy_pages": {"": {}, "whole": {"rows": val(None)}}}
CACHE_WRAPPERS = ("kv_append", "rope_kv_append", "kv_copy_pages", "kv_move_rows", "paged_decode", "paged_decode_shared", "paged_prefill")


def shapes(got):
    if got is None:
        return None
    if isinstance(got, mg.MoEExpertTable):
        return "table"
    return [(tuple(t.shape), t.dtype) for t in ([got] if isinstance(got, torch.Tensor) else got)]


def valid_calls(o):
    """(label, wrapper, kind, changes) of every valid call"""
    for name in WRAPPERS:
        for kind in (KINDS if name in CACHE_WRAPPERS else ("int4",)):
            for label, changes in VARIANTS.get(name, {"": {}}).items():
                tag = ", ".join(s for s in (label, kind if name in CACHE_WRAPPERS else "") if s)
                yield f"{name}[{tag}]" if tag else name, name, kind, changes


@pytest.mark.parametrize("name", list(WRAPPERS))
def test_wrapper_refuses_and_returns(o, name, monkeypatch):
    want, bad = WRAPPERS[name]
    real, launched = _lib.load(), []

    class Watching:
        """the library, noting every entry that is called: a bad call must raise before it reaches one that takes a stream"""
        def __getattr__(self, entry):
            fn = getattr(real, entry)

            def noted(*args):
                launched.append(entry)
                return fn(*args)
            return noted

    for changes, (exc, match) in bad:
        monkeypatch.setattr(_lib, "_lib", Watching())
        with pytest.raises(exc, match=match):
            call(name, o, **changes)
        monkeypatch.setattr(_lib, "_lib", real)
        assert not [e for e in launched if not e.endswith(("_workspace_bytes", "_supported", "error"))], (name, sorted(changes), launched)
        del launched[:]
    for label, _, kind, changes in valid_calls(o):
        if label.split("[")[0] == name:
            got = call(name, o, kind, **changes)
            torch.cuda.synchronize()
            assert shapes(got) == want, label
            if want == "table":
                assert got.tensor.dtype is I64 and tuple(got.tensor.shape) == (E, 8) and got.E == E and got.K == K and got.split == SPLIT
                assert got.N == (2 * I if name == "moe_gate_up_table" else I) and got.wmode == _lib.MM_W_FP4 and not got.has_bias


def record_entries(o):
    """{label: the mm_* symbols the valid call reached, in order}, over a stand-in that forwards to the real library"""
    real, seen, out = _lib.load(), [], {}

    class Recording:
        def __getattr__(self, entry):
            fn = getattr(real, entry)            # (a symbol the library lacks stays an AttributeError: hasattr() keeps working)

            def forward(*args):
                seen.append(entry)
                return fn(*args)
            return forward

    _lib._lib = Recording()
    try:
        for label, name, kind, changes in valid_calls(o):
            del seen[:]
            call(name, o, kind, **changes)
            out[label] = list(seen)
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
    return out


def test_wrapper_calls_its_entries(o):
    want = json.load(open(GOLDEN))
    got = record_entries(o)
    assert sorted(got) == sorted(want)
    for label in want:
        assert got[label] == want[label], label
