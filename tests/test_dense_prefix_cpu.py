"""CPU tests of dense attention over a cached prefix (include/micromix_kvgather.h: mm_kv_gather_dense; include/micromix_attention_prefix.h:
mm_dense_attention_prefix, its workspace and plan queries): the headers, the symbols and the Python names; the statuses the C entries
give without device work; the plan."""
import ctypes
import inspect

import pytest

from micromix_amd import _lib, build, mixedgemm
from micromix_amd.kvcache import PagedKVCache

OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED


def plan(Tq, B, Hq, bound):
    nc, chunk = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.load().mm_dense_attention_prefix_plan(Tq, B, Hq, bound, ctypes.byref(nc), ctypes.byref(chunk)) == nc.value
    return nc.value, chunk.value


def test_symbols_prototypes_build_list_and_names():
    """fails without the feature: the headers, the symbols and the Python names do not exist there"""
    assert _lib.KVGATHER_EXPORTS == ("mm_kv_gather_dense",) and _lib.ATTENTION_EXPORTS == ("mm_dense_attention",)
    assert _lib.ATTENTION_PREFIX_EXPORTS == ("mm_dense_attention_prefix_plan", "mm_dense_attention_prefix_workspace_bytes", "mm_dense_attention_prefix")
    assert {"micromix_kvgather.h", "micromix_attention_prefix.h"} <= {h.rsplit("/", 1)[-1] for h in build.HEADERS} and "kv_gather.hip" in build.SOURCES
    lib = _lib.load()
    assert lib.mm_version() == 660 and all(hasattr(lib, n) for n in _lib.KVGATHER_EXPORTS + _lib.ATTENTION_PREFIX_EXPORTS)
    assert lib.mm_dense_attention_prefix_workspace_bytes.restype is ctypes.c_size_t
    for name in ("kv_gather_dense", "dense_attention_prefix", "dense_attention_prefix_workspace_bytes", "dense_attention_prefix_plan"):
        assert name in mixedgemm.__all__
    assert list(inspect.signature(mixedgemm.dense_attention_prefix).parameters) == ["q", "k", "v", "qo_indptr", "kv_indptr", "max_kv_len",
                                                                                    "sm_scale", "workspace"]
    assert list(inspect.signature(PagedKVCache.attend_new_dense).parameters) == ["self", "layer", "q", "max_seq_len", "sm_scale"]


# a valid call's arguments by name; no case reaches the device.  nc > 1 here, so the workspace is looked at last
GOOD = dict(q=4096, k=8192, v=12288, sq=512, sk=256, sv=256, qo=64, kvp=128, B=2, Tq=300, Tk=900, Hq=4, Hkv=2, hd=128, bound=700, ws=1 << 20,
            wsb=1 << 40, o=16384)
PREFIX_CASES = [
    (dict(Tq=0), OK), (dict(B=0), OK), (dict(Tq=-1), BAD), (dict(Tk=-1), BAD), (dict(bound=-1), BAD), (dict(Tk=-1, Tq=0), BAD),
    (dict(bound=-1, hd=64), BAD), (dict(q=0), BAD), (dict(kvp=0), BAD), (dict(kvp=130), BAD), (dict(qo=66), BAD), (dict(sk=248), BAD),
    (dict(hd=64), UNS), (dict(Hq=5, sq=640), UNS), (dict(sk=(1 << 22) + 8), UNS), (dict(ws=0), BAD), (dict(ws=(1 << 20) + 8), BAD),
    (dict(wsb=1024), BAD), (dict(ws=0, hd=64), UNS), (dict(ws=0, bound=256, Tq=0), OK)]


@pytest.mark.parametrize("change,status", PREFIX_CASES, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in PREFIX_CASES])
def test_prefix_statuses_without_device_work(change, status):
    a = {**GOOD, **change}
    assert plan(GOOD["Tq"], GOOD["B"], GOOD["Hq"], GOOD["bound"])[0] > 1
    assert status == _lib.load().mm_dense_attention_prefix(a["q"], a["k"], a["v"], a["sq"], a["sk"], a["sv"], a["qo"], a["kvp"], a["B"], a["Tq"],
                                                           a["Tk"], a["Hq"], a["Hkv"], a["hd"], a["bound"], 0.1, a["ws"], a["wsb"], a["o"], None)


CACHE = dict(data=4096, param=8192, kind=_lib.MM_KV_INT4, pages=8, L=2, layer=1, Hkv=2, P=16, hd=128, ip=64, idx=128, last=192, B=2, out=256,
             T=100, k=16384, v=32768, sk=256, sv=256)
GATHER_CASES = [
    (dict(T=0), OK), (dict(B=0), OK), (dict(T=-1), BAD), (dict(layer=2), BAD), (dict(kind=2), BAD), (dict(P=0), BAD), (dict(hd=64), UNS),
    (dict(sk=248), BAD), (dict(sv=260), BAD), (dict(sk=128), BAD), (dict(sk=248, T=0), BAD), (dict(out=0), BAD), (dict(out=258), BAD),
    (dict(k=0), BAD), (dict(v=32776), BAD), (dict(data=4104), BAD), (dict(param=0), BAD), (dict(idx=0), BAD)]


@pytest.mark.parametrize("change,status", GATHER_CASES, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in GATHER_CASES])
def test_gather_statuses_without_device_work(change, status):
    a = {**CACHE, **change}
    assert status == _lib.load().mm_kv_gather_dense(a["data"], a["param"], a["kind"], a["pages"], a["L"], a["layer"], a["Hkv"], a["P"], a["hd"],
                                                    a["ip"], a["idx"], a["last"], a["B"], a["out"], a["T"], a["k"], a["v"], a["sk"], a["sv"], None)


@pytest.mark.parametrize("Tq,B,Hq", [(512, 1, 32), (130, 1, 4), (4096, 1, 32), (320, 64, 32), (1, 1, 1)])
def test_plan(Tq, B, Hq):
    """chunk is a multiple of the kv tile and there is at most one chunk per 256 tokens of the bound; the chunks cover the bound, and the
    span they cover never shrinks when the bound grows; the workspace is the partial rows of every (tile, head, chunk), none for one
    chunk; counts the entry refuses, and nothing to do, plan one chunk"""
    BQ, BK, covered = _lib.ATTENTION["MM_DENSE_ATTN_BQ"], _lib.ATTENTION["MM_DENSE_ATTN_BK"], 0
    for bound in list(range(0, 2200, 7)) + [8192, 32768, 32769, 1 << 20]:
        nc, chunk = plan(Tq, B, Hq, bound)
        assert nc >= 1 and chunk % BK == 0 and nc * chunk >= max(bound, covered) and nc <= max(-(-bound // 256), 1)
        assert nc * (Tq // BQ + B) * Hq < _lib.ATTENTION_PREFIX["MM_DENSE_PREFIX_TARGET"] + (Tq // BQ + B) * Hq or nc == 1
        covered = nc * chunk
        want = (Tq // BQ + B) * Hq * nc * BQ * (128 + 2) * 4 if nc > 1 else 0
        assert _lib.load().mm_dense_attention_prefix_workspace_bytes(Tq, B, Hq, bound) == want
    assert plan(512, 1, 32, 32768) == (4, 8192)
    for refused in ((-1, B, Hq, 4096), (Tq, -1, Hq, 4096), (Tq, B, 0, 4096), (Tq, B, Hq, -1), (0, B, Hq, 4096), (Tq, 0, Hq, 4096)):
        assert plan(*refused) == (1, BK) and _lib.load().mm_dense_attention_prefix_workspace_bytes(*refused) == 0
