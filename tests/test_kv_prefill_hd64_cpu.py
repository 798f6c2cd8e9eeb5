"""CPU tests of causal multi-token attention over the paged cache for 64-wide heads (include/micromix_kv_prefill_hd64.h): the symbols
and prototypes, the plan and the workspace worked by hand, the statuses the C entry gives without device work, and what the Python
side refuses before any device work.  No kernel is launched here."""
import ctypes

import pytest
import torch

from micromix_amd import _lib, build, mixedgemm
from micromix_amd.kvcache import PagedKVCache

OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED
BF16, FP8, INT4 = _lib.MM_KV_BF16, _lib.MM_KV_FP8_E4M3, _lib.MM_KV_INT4


def test_symbols_prototypes_and_build_lists():
    assert _lib.KV_PREFILL_HD64_EXPORTS == ("mm_paged_prefill_hd64_workspace_bytes", "mm_paged_prefill_hd64_plan", "mm_paged_prefill_hd64")
    lib = _lib.load()
    assert lib.mm_version() == 660
    assert len(lib.mm_paged_prefill_hd64.argtypes) == 22 and len(lib.mm_paged_prefill_hd64_plan.argtypes) == 10
    assert lib.mm_paged_prefill_hd64_workspace_bytes.restype is ctypes.c_size_t
    assert _lib.KV_PREFILL_HD64 == dict(MM_KV_PREFILL_HD64_ROWS=128, MM_KV_PREFILL_HD64_ROWS_FEW=64, MM_KV_PREFILL_HD64_TILE=64)
    assert "kv_prefill_hd64.hip" in build.SOURCES and any(h.endswith("micromix_kv_prefill_hd64.h") for h in build.HEADERS)
    assert {"paged_prefill_hd64_plan", "paged_prefill_hd64_workspace_bytes"} <= set(mixedgemm.__all__)


@pytest.mark.parametrize("args,plan,floats", [
    # g = 4, 1200 rows over 2 sequences: 128 rows, 32 tokens a tile, 300 // 32 + 2 tiles; 256 positions are one chunk
    ((300, 2, 8, 2, 256), (128, 32, 11, 1, 256), 0),
    # ... 2048 positions: min(ceil(1024 / 22), 2048 / 256) = 8 chunks of 256; partials tiles * Hkv * chunks * rows * 66
    ((300, 2, 8, 2, 2048), (128, 32, 11, 8, 256), 11 * 2 * 8 * 128 * 66),
    # a draft of 5 per sequence: 10 * 4 <= 64 * 2, the 64-row kernel, 16 tokens a tile, 0 + 2 tiles
    ((10, 2, 8, 2, 2048), (64, 16, 2, 8, 256), 2 * 2 * 8 * 64 * 66),
    # g = 7: 128 // 7 = 18 tokens a tile; 36 work items want 29 chunks, 1300 positions allow 6: ceil(1300 / 6) = 217 -> 256
    ((300, 2, 14, 2, 1300), (128, 18, 18, 6, 256), 18 * 2 * 6 * 128 * 66),
    ((300, 2, 8, 2, 0), (128, 32, 11, 1, 64), 0),
])
def test_plan_and_workspace_by_hand(args, plan, floats):
    assert tuple(mixedgemm.paged_prefill_hd64_plan(*args)) == plan
    assert mixedgemm.paged_prefill_hd64_workspace_bytes(*args) == 4 * floats


def test_plan_and_workspace_refusals():
    assert mixedgemm.paged_prefill_hd64_workspace_bytes(300, 2, 34, 2, 2048) == 0          # g = 17
    with pytest.raises(RuntimeError):
        mixedgemm.paged_prefill_hd64_plan(300, 2, 9, 2, 2048)


# a valid call's arguments by name; every case changes some and names the status (none of them reaches the device)
GOOD = dict(q=1 << 16, qo=256, T=30, data=4096, param=8192, kind=BF16, pages=8, L=2, layer=0, Hkv=2, P=16, ip=64, ix=128, lp=192, B=2, Hq=8,
            n=200, ws=0, wsb=0, o=2 << 16)
CASES = [
    (dict(T=0), OK), (dict(B=0), OK), (dict(T=0, q=0, o=0, data=0, qo=0), OK),
    (dict(kind=INT4), UNS), (dict(kind=INT4, T=0), UNS), (dict(Hq=34), UNS), (dict(Hq=34, q=0), UNS), (dict(kind=2), BAD), (dict(Hq=9), BAD),
    (dict(n=-1), BAD), (dict(T=-1), BAD), (dict(P=0), BAD), (dict(layer=2), BAD), (dict(kind=INT4, Hq=9), BAD),
    (dict(q=0), BAD), (dict(qo=0), BAD), (dict(o=0), BAD), (dict(q=(1 << 16) + 8), BAD), (dict(o=(2 << 16) + 8), BAD), (dict(qo=258), BAD),
    (dict(ip=66), BAD), (dict(data=4104), BAD), (dict(kind=FP8, param=0), BAD),
    (dict(n=1300), BAD), (dict(n=1300, ws=3 << 16, wsb=100), BAD), (dict(n=1300, ws=(3 << 16) + 8, wsb=1 << 24), BAD),
]


@pytest.mark.parametrize("change,status", CASES, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in CASES])
def test_statuses_without_device_work(change, status):
    a = {**GOOD, **change}
    got = _lib.load().mm_paged_prefill_hd64(a["q"], a["qo"], a["T"], *(a[n] for n in ("data", "param", "kind", "pages", "L", "layer", "Hkv", "P", "ip", "ix", "lp", "B")),
                                            a["Hq"], a["n"], 0.0, a["ws"], a["wsb"], a["o"], None)
    assert got == status


def cache64():
    return PagedKVCache(num_layers=2, num_kv_heads=2, page_size=4, max_pages=8, batch=2, kind="bf16", device="cpu", head_dim=64)


@pytest.mark.parametrize("refused", [
    lambda c: mixedgemm.paged_prefill(None, c.kv_data, None, c.kv_indptr, c.kv_indices, c.last_page_len, c.append_indptr, 0, 8, window=4),
    lambda c: mixedgemm.paged_prefill(None, c.kv_data, None, c.kv_indptr, c.kv_indices, c.last_page_len, c.append_indptr, 0, 8,
                                      tree_mask=torch.zeros(1, dtype=torch.int64)),
    lambda c: c.attend_new(0, torch.zeros((0, 8, 128), dtype=torch.bfloat16)),
    lambda c: c.attend_new(0, torch.zeros((0, 8, 64), dtype=torch.float16)),
    lambda c: c.attend_new(0, torch.zeros((0, 8, 64), dtype=torch.bfloat16), tree=torch.zeros(0, dtype=torch.int64)),
], ids=["window", "tree_mask", "q_width", "q_dtype", "tree"])
def test_refused_before_device_work(refused):
    with pytest.raises(ValueError, match="head_dim 64"):
        refused(cache64())
