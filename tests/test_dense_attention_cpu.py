"""CPU tests of dense causal attention (include/micromix_attention.h: mm_dense_attention): the header, the symbol, the prototype, the
build lists and the Python name; the statuses the C entry gives without device work; the argument checks of mixedgemm.dense_attention
that need no device.  No kernel is launched here."""
import ctypes
import inspect

import pytest
import torch

from micromix_amd import _lib, build, mixedgemm

OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED


def test_symbol_prototype_build_lists_and_export():
    """fails without the feature: the header, the symbol, ATTENTION_EXPORTS and the Python name do not exist there"""
    assert "mm_dense_attention" in _lib.header_text("micromix_attention.h")
    assert _lib.ATTENTION_EXPORTS == ("mm_dense_attention",) and "mm_dense_attention" not in _lib.EXPORTS
    lib = _lib.load()
    assert lib.mm_version() == 660 and hasattr(lib, "mm_dense_attention")
    v, i, f, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    assert lib.mm_dense_attention.restype is i and list(lib.mm_dense_attention.argtypes) == [v, v, v, ll, ll, ll, v, i, i, i, i, i, f, v, v]
    assert _lib.ATTENTION == dict(MM_DENSE_ATTN_BQ=128, MM_DENSE_ATTN_BK=64, MM_DENSE_ATTN_MAX_STRIDE=1 << 22)
    assert not any(hasattr(_lib, n) for n in _lib.ATTENTION)
    assert "dense_attention.hip" in build.SOURCES and any(h.endswith("micromix_attention.h") for h in build.HEADERS)
    assert "dense_attention" in mixedgemm.__all__
    assert list(inspect.signature(mixedgemm.dense_attention).parameters) == ["q", "k", "v", "seq_indptr", "sm_scale"]


# a valid call's arguments by name; every case changes some and names the status (none of them reaches the device)
GOOD = dict(q=4096, k=8192, v=12288, sq=512, sk=256, sv=256, ip=64, B=2, T=300, Hq=4, Hkv=2, hd=128, o=16384)
STATUS_CASES = [
    (dict(T=0), OK), (dict(B=0), OK), (dict(T=0, q=0, k=0, v=0, o=0, ip=0), OK),
    (dict(T=-1), BAD), (dict(B=-1), BAD), (dict(Hq=0), BAD), (dict(Hkv=0), BAD),
    (dict(q=0), BAD), (dict(k=0), BAD), (dict(v=0), BAD), (dict(o=0), BAD), (dict(ip=0), BAD),
    (dict(q=4104), BAD), (dict(o=16392), BAD), (dict(ip=66), BAD),
    (dict(sq=516), BAD), (dict(sq=504), BAD), (dict(sk=248), BAD), (dict(sv=128), BAD),
    (dict(hd=64), UNS), (dict(Hq=5, sq=640), UNS), (dict(sk=(1 << 22) + 8), UNS), (dict(T=0, hd=64), UNS),
    (dict(T=(1 << 31) - 1, B=1 << 24, Hq=128, Hkv=128, sq=1 << 14, sk=1 << 14, sv=1 << 14), UNS),
]


@pytest.mark.parametrize("change,status", STATUS_CASES, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in STATUS_CASES])
def test_statuses_without_device_work(change, status):
    a = {**GOOD, **change}
    got = _lib.load().mm_dense_attention(a["q"], a["k"], a["v"], a["sq"], a["sk"], a["sv"], a["ip"], a["B"], a["T"], a["Hq"], a["Hkv"], a["hd"],
                                         0.1, a["o"], None)
    assert got == status


def bf(*shape):
    return torch.zeros(shape, dtype=torch.bfloat16)


@pytest.mark.parametrize("args,error", [
    ((bf(4, 4, 128).float(), bf(4, 2, 128), bf(4, 2, 128)), TypeError),                        # a wrong dtype
    ((bf(4, 4, 128), bf(4, 2, 128), bf(4, 2, 128).half()), TypeError),
    ((bf(4, 4, 64), bf(4, 2, 64), bf(4, 2, 64)), RuntimeError),                                 # a head dimension other than 128
    ((bf(4, 4 * 128 + 64), bf(4, 256), bf(4, 256)), RuntimeError),
    ((bf(4, 5, 128), bf(4, 2, 128), bf(4, 2, 128)), RuntimeError),                              # Hq % Hkv != 0
    ((bf(4, 4, 128), bf(4, 2, 128), bf(4, 1, 128)), RuntimeError),                              # v with other heads than k
    ((bf(4, 4, 128), bf(5, 2, 128), bf(4, 2, 128)), RuntimeError),                              # k / v with another token count
    ((bf(4, 4, 128), bf(4, 2, 128), bf(3, 2, 128)), RuntimeError),
    ((bf(4, 4, 128), bf(4, 2, 128), bf(4, 2, 128), torch.zeros(0, dtype=torch.int32)), RuntimeError),       # seq_indptr: B + 1 >= 1 entries,
    ((bf(4, 4, 128), bf(4, 2, 128), bf(4, 2, 128), torch.zeros((2, 2), dtype=torch.int32)), RuntimeError),  # one dimension,
    ((bf(4, 4, 128), bf(4, 2, 128), bf(4, 2, 128), torch.zeros(2, dtype=torch.int64)), RuntimeError),       # int32
    ((bf(4, 4, 128), bf(4, 2, 128), bf(4, 2, 128)), RuntimeError),                              # no CPU path
])
def test_python_argument_checks(args, error):
    with pytest.raises(error):
        mixedgemm.dense_attention(*args)
