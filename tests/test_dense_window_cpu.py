"""CPU tests of sliding-window dense attention (include/micromix_attention_window.h: mm_dense_attention_window): the header, the symbol,
the prototype and the Python names; the statuses the C entry gives without device work; the argument errors for `window`."""
import ctypes
import inspect

import pytest
import torch

from micromix_amd import _lib, build, mixedgemm
from micromix_amd.kvcache import PagedKVCache

OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED


def test_symbol_prototype_build_list_and_names():
    """fails without the feature: the header, the symbol, the Python name and the keyword do not exist there"""
    assert "mm_dense_attention_window" in _lib.header_text("micromix_attention_window.h")
    assert any(h.endswith("micromix_attention_window.h") for h in build.HEADERS)
    assert _lib.ATTENTION_WINDOW_EXPORTS == ("mm_dense_attention_window",) and _lib.ATTENTION_EXPORTS == ("mm_dense_attention",)
    lib = _lib.load()
    fn = lib.mm_dense_attention_window
    assert lib.mm_version() == 660 and fn.restype is ctypes.c_int and list(fn.argtypes) == list(lib.mm_dense_attention.argtypes) + [ctypes.c_int]
    assert "dense_attention_window" in mixedgemm.__all__
    assert list(inspect.signature(mixedgemm.dense_attention_window).parameters) == ["q", "k", "v", "window", "seq_indptr", "sm_scale"]
    windowed = inspect.signature(PagedKVCache.prefill_fresh).parameters["windowed"]
    assert windowed.default is False and windowed.kind is inspect.Parameter.KEYWORD_ONLY


# a valid call's arguments by name, as tests/test_dense_attention_cpu.py has them; no case reaches the device
GOOD = dict(q=4096, k=8192, v=12288, sq=512, sk=256, sv=256, ip=64, B=2, T=300, Hq=4, Hkv=2, hd=128, o=16384, W=64)
STATUS_CASES = [
    (dict(W=0), BAD), (dict(W=-1), BAD), (dict(W=0, T=0), BAD), (dict(W=0, hd=64), BAD),      # ahead of the early MM_OK and of UNSUPPORTED
    (dict(T=0), OK), (dict(B=0, W=1 << 30), OK), (dict(T=-1), BAD), (dict(q=0), BAD), (dict(ip=66), BAD), (dict(sk=248), BAD),
    (dict(hd=64), UNS), (dict(Hq=5, sq=640), UNS), (dict(sk=(1 << 22) + 8), UNS)]


@pytest.mark.parametrize("change,status", STATUS_CASES, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in STATUS_CASES])
def test_statuses_without_device_work(change, status):
    a = {**GOOD, **change}
    assert status == _lib.load().mm_dense_attention_window(a["q"], a["k"], a["v"], a["sq"], a["sk"], a["sv"], a["ip"], a["B"], a["T"], a["Hq"],
                                                           a["Hkv"], a["hd"], 0.1, a["o"], None, a["W"])


@pytest.mark.parametrize("window,error", [(0, ValueError), (-3, ValueError), (4.0, ValueError), (True, ValueError), (None, ValueError),
                                          (4, RuntimeError)])                # a good window: dense_attention's "no CPU path"
def test_python_window_argument(window, error):
    q, kv = torch.zeros((4, 4, 128), dtype=torch.bfloat16), torch.zeros((4, 2, 128), dtype=torch.bfloat16)
    with pytest.raises(error):
        mixedgemm.dense_attention_window(q, kv, kv, window)
