"""CPU tests of the paged KV cache for 64-wide heads (include/micromix_kv_hd64.h): the symbols, prototypes, build lists and constants;
the statuses the C entries give without device work; PagedKVCache(head_dim=64) on the CPU: its tensors, and what it refuses before any
device work.  No kernel is launched here."""
import ctypes

import pytest
import torch

from micromix_amd import _lib, build
from micromix_amd.kvcache import PagedKVCache

OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED
BF16, FP8, INT4 = _lib.MM_KV_BF16, _lib.MM_KV_FP8_E4M3, _lib.MM_KV_INT4


def test_symbols_prototypes_build_lists_and_constants():
    assert _lib.KV_HD64_EXPORTS == ("mm_rope_kv_append_hd64", "mm_paged_decode_hd64_workspace_bytes", "mm_paged_decode_hd64_split",
                                    "mm_paged_decode_hd64")
    assert not set(_lib.KV_HD64_EXPORTS) & set(_lib.EXPORTS)
    lib = _lib.load()
    assert lib.mm_version() == 660
    assert len(lib.mm_rope_kv_append_hd64.argtypes) == 26 and len(lib.mm_paged_decode_hd64.argtypes) == 20
    assert lib.mm_paged_decode_hd64_workspace_bytes.restype is ctypes.c_size_t
    assert _lib.KV_HD64 == dict(MM_KV_HD64_APPEND_TOKENS=16, MM_KV_HD64_DECODE_TILE=64, MM_KV_HD64_DECODE_WAVES=4)
    assert "kv_hd64.hip" in build.SOURCES and any(h.endswith("micromix_kv_hd64.h") for h in build.HEADERS)
    assert lib.mm_paged_decode_hd64_workspace_bytes(9, 8, 2, 256) == 0
    assert lib.mm_paged_decode_hd64_workspace_bytes(9, 8, 2, 1300) == 9 * 8 * 6 * 66 * 4      # six chunks of 256
    assert lib.mm_paged_decode_hd64_workspace_bytes(9, 34, 2, 1300) == 0                       # g = 17: refused


# a valid call's arguments by name; every case changes some and names the status (none of them reaches the device)
APPEND = dict(data=4096, param=8192, kind=FP8, pages=8, L=2, layer=1, Hkv=2, P=16, ip=64, ix=128, lp=192, B=2, q=1 << 16, k=2 << 16, v=3 << 16,
              s=512, Hq=4, cos=4 << 16, sin=5 << 16, cs=64, app=256, T=30, qo=6 << 16, ko=7 << 16, vo=8 << 16)
APPEND_CASES = [
    (dict(T=0), OK), (dict(T=0, q=0, k=0, v=0, qo=0, data=0), OK), (dict(cos=0, sin=0, q=0, qo=0, T=0), OK),
    (dict(kind=INT4), UNS), (dict(kind=INT4, T=0), UNS), (dict(kind=2), BAD), (dict(T=-1), BAD), (dict(Hq=5), BAD), (dict(layer=2), BAD),
    (dict(s=248), BAD), (dict(s=516), BAD), (dict(cs=56), BAD), (dict(Hq=2, Hkv=2, s=64), BAD), (dict(kind=INT4, s=248), BAD),
    (dict(q=(1 << 16) + 8), BAD), (dict(vo=(8 << 16) + 4), BAD), (dict(data=4104), BAD), (dict(app=258), BAD),
    (dict(param=0), BAD), (dict(k=0), BAD), (dict(app=0), BAD), (dict(B=0), BAD), (dict(cos=0), BAD), (dict(q=0), BAD),
    (dict(cos=0, sin=0, qo=0), BAD),
]
DECODE = dict(q=1 << 16, data=4096, param=8192, kind=BF16, pages=8, L=2, layer=0, Hkv=2, P=16, ip=64, ix=128, lp=192, B=2, Hq=8, n=200,
              ws=0, wsb=0, o=2 << 16)
DECODE_CASES = [
    (dict(B=0), OK), (dict(B=0, q=0, o=0, data=0), OK),
    (dict(kind=INT4), UNS), (dict(Hq=34), UNS), (dict(Hq=34, q=0), UNS), (dict(Hq=9), BAD), (dict(n=-1), BAD), (dict(P=0), BAD),
    (dict(q=0), BAD), (dict(o=0), BAD), (dict(q=(1 << 16) + 8), BAD), (dict(ip=66), BAD), (dict(kind=FP8, param=0), BAD),
    (dict(n=1300), BAD), (dict(n=1300, ws=3 << 16, wsb=100), BAD), (dict(n=1300, ws=(3 << 16) + 8, wsb=1 << 20), BAD),
]


CASES = [(APPEND, c, st) for c, st in APPEND_CASES] + [(DECODE, c, st) for c, st in DECODE_CASES]


@pytest.mark.parametrize("good,change,status", CASES, ids=[("append:" if g is APPEND else "decode:") + ",".join(f"{k}={v}" for k, v in c.items()) for g, c, _ in CASES])
def test_statuses_without_device_work(good, change, status):
    a, lib = {**good, **change}, _lib.load()
    geometry = [a[n] for n in ("data", "param", "kind", "pages", "L", "layer", "Hkv", "P", "ip", "ix", "lp", "B")]
    if good is APPEND:
        got = lib.mm_rope_kv_append_hd64(*geometry, *(a[n] for n in ("q", "k", "v", "s", "Hq", "cos", "sin", "cs", "app", "T", "qo", "ko", "vo")), None)
    else:
        got = lib.mm_paged_decode_hd64(a["q"], *geometry, a["Hq"], a["n"], 0.0, a["ws"], a["wsb"], a["o"], None)
    assert got == status


def cache(**kw):
    return PagedKVCache(**{**dict(num_layers=2, num_kv_heads=2, page_size=4, max_pages=8, batch=2, kind="bf16", device="cpu"), **kw})


def test_cache_tensors():
    c = cache(head_dim=64)
    assert c.kv_data.shape == (8, 2, 2, 2, 4, 64) and c.kv_data.dtype is torch.bfloat16 and c.kv_param is None
    c = cache(head_dim=64, kind="fp8_e4m3")
    assert c.kv_data.shape == (8, 2, 2, 2, 4, 64) and c.kv_data.dtype is torch.float8_e4m3fn and c.kv_param.shape == (8, 2, 2, 2, 4, 2)
    for kind, last, dtype in (("int4", 64, torch.uint8), ("fp8_e4m3", 128, torch.uint8), ("bf16", 128, torch.bfloat16)):
        c = cache(kind=kind)                                                       # the default builds what it always did
        assert c.head_dim == 128 and c.kv_data.shape == (8, 2, 2, 2, 4, last) and c.kv_data.dtype is dtype
        assert (c.kv_param is None) == (kind == "bf16")
    c = cache(head_dim=64)
    c.extend([5, 2])
    c.truncate(0, 3)
    c.reset(1)
    assert c.seq_lens == [3, 0] and c.pages_in_use == 1


@pytest.mark.parametrize("refused", [
    lambda: cache(head_dim=64, kind="int4"), lambda: cache(head_dim=64, window=8), lambda: cache(head_dim=32),
    lambda: cache(head_dim=64).fork(0, 1), lambda: cache(head_dim=64).attend_new(0, None), lambda: cache(head_dim=64).tree_mask([None, None]),
    lambda: cache(head_dim=64).step_launch(None, 1, max_seq_len=8), lambda: cache(head_dim=64).attend(0, None, shared=True),
    lambda: cache(head_dim=64).attend_new_dense(0, None), lambda: cache(head_dim=64).accept([[], []]),
    lambda: cache(head_dim=64).verify(None, None, None), lambda: cache(head_dim=64).upload_state(8),
], ids=["int4", "window", "head_dim", "fork", "attend_new", "tree_mask", "step_launch", "shared", "attend_new_dense", "accept", "verify", "upload_state"])
def test_cache_refuses_before_device_work(refused):
    with pytest.raises(ValueError, match="head_dim"):
        refused()
