"""CPU tests of the one-launch decode step (include/micromix_decode_step.h): exports and build lists, the workspace query against
mm_paged_decode's, the statuses without device work, what PagedKVCache.decode_step refuses.  No kernel is launched here."""
import ctypes

import pytest

from micromix_amd import _lib, build, mixedgemm
from micromix_amd.kvcache import PagedKVCache

OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED
BF16, FP8, INT4 = _lib.MM_KV_BF16, _lib.MM_KV_FP8_E4M3, _lib.MM_KV_INT4


def test_symbols_prototypes_and_build_lists():
    assert _lib.DECODE_STEP_EXPORTS == ("mm_rope_append_decode_workspace_bytes", "mm_rope_append_decode")
    assert not set(_lib.DECODE_STEP_EXPORTS) & set(_lib.EXPORTS)
    lib = _lib.load()
    assert lib.mm_version() == 660
    assert len(lib.mm_rope_append_decode.argtypes) == 28 and lib.mm_rope_append_decode.argtypes[16] is ctypes.c_int64
    assert lib.mm_rope_append_decode_workspace_bytes.restype is ctypes.c_size_t
    assert "decode_step.hip" in build.SOURCES and "mx_kv_decode.h" in build.HEADERS and any(h.endswith("micromix_decode_step.h") for h in build.HEADERS)
    assert {"rope_append_decode", "rope_append_decode_workspace_bytes"} <= set(mixedgemm.__all__)


@pytest.mark.parametrize("args", [(9, 8, 2, 256), (9, 8, 2, 1300), (1, 32, 8, 4096), (64, 32, 8, 1024), (4, 8, 3, 500), (9, 34, 2, 1300),
                                  (0, 8, 2, 100), (2, 8, 2, -1)], ids=str)
def test_workspace_is_paged_decodes(args):
    lib = _lib.load()
    assert lib.mm_rope_append_decode_workspace_bytes(*args) == lib.mm_paged_decode_workspace_bytes(*args)
    assert mixedgemm.rope_append_decode_workspace_bytes(*args) == lib.mm_paged_decode_workspace_bytes(*args)


# a valid call's arguments by name; every case changes some and names the status (none of them reaches the device)
GOOD = dict(data=4096, param=8192, kind=INT4, pages=8, L=2, layer=1, Hkv=2, P=16, hd=128, ip=64, ix=128, lp=192, B=2, q=1 << 16, k=2 << 16,
            v=3 << 16, s=1536, Hq=8, cos=4 << 16, sin=5 << 16, cs=128, n=200, ws=0, wsb=0, qo=6 << 16, o=7 << 16)
CASES = [
    (dict(B=0), OK), (dict(B=0, q=0, k=0, v=0, cos=0, sin=0, o=0, data=0, param=0), OK),
    (dict(hd=64), UNS), (dict(hd=64, B=0), UNS), (dict(Hq=34, s=4352), UNS), (dict(Hq=34, s=4352, q=0), UNS),
    (dict(kind=2), BAD), (dict(layer=2), BAD), (dict(P=0), BAD), (dict(hd=0), BAD), (dict(B=-1), BAD), (dict(Hq=9), BAD), (dict(Hq=0), BAD),
    (dict(n=-1), BAD), (dict(s=1022), BAD), (dict(s=1537), BAD), (dict(cs=126), BAD), (dict(cs=129), BAD), (dict(Hq=34, s=1536), BAD),
    (dict(q=0), BAD), (dict(k=0), BAD), (dict(v=0), BAD), (dict(cos=0), BAD), (dict(sin=0), BAD), (dict(o=0), BAD), (dict(data=0), BAD),
    (dict(param=0), BAD), (dict(kind=FP8, param=0), BAD), (dict(ix=0), BAD),
    (dict(q=(1 << 16) + 2), BAD), (dict(qo=(6 << 16) + 2), BAD), (dict(o=(7 << 16) + 1), BAD),
    (dict(n=1300), BAD), (dict(n=1300, ws=3 << 16, wsb=100), BAD), (dict(n=1300, ws=(3 << 16) + 8, wsb=1 << 20), BAD),
]


@pytest.mark.parametrize("change,status", CASES, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in CASES])
def test_statuses_without_device_work(change, status):
    a = {**GOOD, **change}
    names = ("data", "param", "kind", "pages", "L", "layer", "Hkv", "P", "hd", "ip", "ix", "lp", "B", "q", "k", "v", "s", "Hq", "cos", "sin", "cs", "n")
    assert _lib.load().mm_rope_append_decode(*(a[n] for n in names), 0.0, a["ws"], a["wsb"], a["qo"], a["o"], None) == status


def cache(**kw):
    return PagedKVCache(**{**dict(num_layers=2, num_kv_heads=2, page_size=4, max_pages=8, batch=2, kind="bf16", device="cpu"), **kw})


@pytest.mark.parametrize("kw,new,match", [(dict(head_dim=64), 1, "head_dim 64"), (dict(window=8), 1, "window=8"), ({}, [2, 1], "one new token")],
                         ids=["head_dim", "window", "tokens"])
def test_decode_step_refuses_before_device_work(kw, new, match):
    c = cache(**kw)
    c.extend(new)
    with pytest.raises(ValueError, match=match):
        c.decode_step(0, None, None, None, None, None)
