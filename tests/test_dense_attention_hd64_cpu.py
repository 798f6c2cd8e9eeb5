"""CPU tests of the cache-less route for 64-wide heads (include/micromix_attention_hd64.h: mm_dense_attention_hd64, mm_rope_qk_hd64): the
header, the symbols, the prototypes, the build lists and the tile constants; the statuses the C entries give without device work; the
argument checks of mixedgemm.dense_attention / rope_qk that need no device.  No kernel is launched here."""
import ctypes

import pytest
import torch

from micromix_amd import _lib, build, mixedgemm

OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED


def test_symbols_prototypes_build_lists_and_constants():
    assert _lib.ATTENTION_HD64_EXPORTS == ("mm_dense_attention_hd64", "mm_rope_qk_hd64")
    assert not set(_lib.ATTENTION_HD64_EXPORTS) & set(_lib.EXPORTS) and _lib.ATTENTION_EXPORTS == ("mm_dense_attention",)
    lib = _lib.load()
    assert lib.mm_version() == 660
    v, i, f, ll, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.c_int64
    assert lib.mm_dense_attention_hd64.restype is i and list(lib.mm_dense_attention_hd64.argtypes) == [v, v, v, ll, ll, ll, v, i, i, i, i, i, f, v, v]
    assert lib.mm_rope_qk_hd64.restype is i and list(lib.mm_rope_qk_hd64.argtypes) == [v, v, i64, i, i, v, v, i64, i, v, v, v]
    assert _lib.ATTENTION_HD64 == dict(MM_DENSE_ATTN_HD64_BQ=128, MM_DENSE_ATTN_HD64_BK=64, MM_DENSE_ATTN_HD64_MAX_STRIDE=1 << 22,
                                       MM_ROPE_HD64_TOKENS=16)
    assert not any(hasattr(_lib, n) for n in _lib.ATTENTION_HD64)
    assert "dense_attention_hd64.hip" in build.SOURCES and any(h.endswith("micromix_attention_hd64.h") for h in build.HEADERS)


# a valid call's arguments by name; every case changes some and names the status (none of them reaches the device)
GOOD = dict(q=4096, k=8192, v=12288, sq=256, sk=128, sv=128, ip=64, B=2, T=300, Hq=4, Hkv=2, W=0, o=16384)
ATTENTION_CASES = [
    (dict(T=0), OK), (dict(B=0), OK), (dict(T=0, q=0, k=0, v=0, o=0, ip=0), OK), (dict(T=0, W=5), OK),
    (dict(T=-1), BAD), (dict(B=-1), BAD), (dict(Hq=0), BAD), (dict(Hkv=0), BAD), (dict(W=-1), BAD),
    (dict(W=-1, T=0), BAD), (dict(W=-1, Hq=5, sq=320), BAD),                         # window < 0 ahead of the early MM_OK and of UNSUPPORTED
    (dict(q=0), BAD), (dict(k=0), BAD), (dict(v=0), BAD), (dict(o=0), BAD), (dict(ip=0), BAD),
    (dict(q=4104), BAD), (dict(o=16392), BAD), (dict(ip=66), BAD),
    (dict(sq=260), BAD), (dict(sq=248), BAD), (dict(sk=120), BAD), (dict(sv=64), BAD),
    (dict(Hq=5, sq=320, q=0), BAD),                                                  # BAD_ARG ahead of UNSUPPORTED
    (dict(Hq=5, sq=320), UNS), (dict(T=0, Hq=5), UNS),                               # UNSUPPORTED ahead of the early MM_OK
    (dict(sk=(1 << 22) + 8), UNS),
    (dict(T=(1 << 31) - 1, B=1 << 24, Hq=128, Hkv=128, sq=1 << 13, sk=1 << 13, sv=1 << 13), UNS),
]
ROPE_GOOD = dict(q=4096, k=8192, s=384, Hq=4, Hkv=2, cos=12288, sin=16384, cs=64, T=300, qo=20480, ko=24576)
ROPE_CASES = [
    (dict(T=0), OK), (dict(T=0, q=0, k=0, cos=0, sin=0, qo=0, ko=0), OK),
    (dict(T=-1), BAD), (dict(Hq=0), BAD), (dict(Hkv=0), BAD), (dict(Hq=5), BAD), (dict(T=0, s=248), BAD),
    (dict(s=248), BAD), (dict(s=388), BAD), (dict(cs=56), BAD), (dict(cs=68), BAD),
    (dict(q=0), BAD), (dict(k=0), BAD), (dict(cos=0), BAD), (dict(sin=0), BAD), (dict(qo=0), BAD), (dict(ko=0), BAD),
    (dict(q=4104), BAD), (dict(sin=16392), BAD), (dict(ko=24584), BAD),
]


def ids(cases):
    return [",".join(f"{k}={v}" for k, v in c.items()) for c, _ in cases]


@pytest.mark.parametrize("change,status", ATTENTION_CASES, ids=ids(ATTENTION_CASES))
def test_attention_statuses_without_device_work(change, status):
    a = {**GOOD, **change}
    got = _lib.load().mm_dense_attention_hd64(a["q"], a["k"], a["v"], a["sq"], a["sk"], a["sv"], a["ip"], a["B"], a["T"], a["Hq"], a["Hkv"],
                                              a["W"], 0.1, a["o"], None)
    assert got == status


@pytest.mark.parametrize("change,status", ROPE_CASES, ids=ids(ROPE_CASES))
def test_rope_statuses_without_device_work(change, status):
    a = {**ROPE_GOOD, **change}
    got = _lib.load().mm_rope_qk_hd64(a["q"], a["k"], a["s"], a["Hq"], a["Hkv"], a["cos"], a["sin"], a["cs"], a["T"], a["qo"], a["ko"], None)
    assert got == status


def bf(*shape):
    return torch.zeros(shape, dtype=torch.bfloat16)


@pytest.mark.parametrize("call,args,message", [
    (mixedgemm.dense_attention, (bf(4, 4, 64), bf(4, 2, 128), bf(4, 2, 128)), "agree on the head dimension"),       # mixed 64 / 128
    (mixedgemm.dense_attention, (bf(4, 4, 64), bf(4, 2, 64), bf(4, 128)), "agree on the head dimension"),           # 2-D is never 64-wide
    (mixedgemm.dense_attention_window, (bf(4, 4, 128), bf(4, 2, 128), bf(4, 2, 64), 3), "agree on the head dimension"),
    (mixedgemm.dense_attention_prefix, (bf(4, 4, 64), bf(4, 2, 64), bf(4, 2, 64), None, None, 4), "128-wide heads only"),
    (mixedgemm.dense_attention, (bf(4, 5, 64), bf(4, 2, 64), bf(4, 2, 64)), "not a multiple"),                      # Hq % Hkv != 0
    (mixedgemm.dense_attention, (bf(4, 4, 64), bf(4, 2, 64), bf(4, 2, 64)), "no CPU path"),
    (mixedgemm.rope_qk, (bf(4, 4, 64), bf(4, 2, 128), bf(4, 64), bf(4, 64)), "agree on the head dimension"),
    (mixedgemm.rope_qk, (bf(4, 4, 64), bf(4, 2, 64), bf(4, 128), bf(4, 128)), r"cos and sin must be \[T, 64\]"),    # cos / sin of the wrong width
    (mixedgemm.rope_qk, (bf(4, 4, 64), bf(4, 2, 64), bf(4, 64), bf(4, 32)), r"cos and sin must be \[T, 64\]"),
    (mixedgemm.rope_qk, (bf(4, 4, 64), bf(4, 2, 64), bf(4, 64), bf(4, 64)), "no CPU path"),
])
def test_python_argument_checks(call, args, message):
    with pytest.raises(RuntimeError, match=message):
        call(*args)
