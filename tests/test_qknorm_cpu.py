"""CPU tests of QK-norm (include/micromix_qknorm.h): exports, prototypes and build lists, statuses without device work, what 64-wide
heads refuse, and the two preconditions of the GPU tests' inputs: where the sum is exact the oracle is HF's chain bit for bit, and the
Gaussian case tells the header's tree from other orders.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest
import torch

from micromix_amd import _lib, build, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import qknorm_oracle as qo

OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED
PARENTS = {"mm_rope_kv_append_qknorm": "mm_rope_kv_append", "mm_rope_prefill_qknorm": "mm_rope_prefill",
           "mm_rope_append_decode_qknorm": "mm_rope_append_decode"}


def test_symbols_prototypes_and_build_lists():
    assert _lib.QKNORM_EXPORTS == tuple(PARENTS) and not set(_lib.QKNORM_EXPORTS) & set(_lib.EXPORTS) and _lib.QKNORM == {}
    lib = _lib.load()
    assert lib.mm_version() == 660
    for name, parent in PARENTS.items():
        mine, theirs = getattr(lib, name).argtypes, getattr(lib, parent).argtypes
        assert list(mine) == [*theirs[:-1], ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, theirs[-1]], name
    assert "mx_qknorm.h" in build.HEADERS and any(h.endswith("micromix_qknorm.h") for h in build.HEADERS)


# valid calls' arguments (fake addresses; none of the cases reaches the device); the weights and eps go before the stream
KV = dict(data=4096, param=8192, kind=_lib.MM_KV_INT4, pages=8, L=2, layer=1, Hkv=2, P=16, hd=128, ip=64, ix=128, lp=192, B=2)
QKV = dict(q=1 << 16, k=2 << 16, v=3 << 16, s=1536, Hq=8, cos=4 << 16, sin=5 << 16, cs=128)
TAILS = {"mm_rope_kv_append_qknorm": dict(app=256, T=2, qo=6 << 16),
         "mm_rope_prefill_qknorm": dict(app=256, T=2, qo=6 << 16, ko=7 << 16, vo=0),
         "mm_rope_append_decode_qknorm": dict(n=200, sm=0.0, ws=0, wsb=0, qo=6 << 16, o=7 << 16)}
NORM = dict(qw=8 << 16, kw=9 << 16, eps=1e-6)
CASES = [(dict(qw=0), BAD), (dict(kw=0), BAD), (dict(qw=(8 << 16) + 8), BAD), (dict(kw=(9 << 16) + 4), BAD), (dict(eps=0.0), BAD),
         (dict(eps=-1e-6), BAD), (dict(eps=float("inf")), BAD), (dict(eps=float("nan")), BAD), (dict(hd=64), UNS), (dict(q=0), BAD),
         (dict(T=0, B=0, qw=0, kw=0), OK), (dict(T=0, B=0, eps=0.0), BAD)]


@pytest.mark.parametrize("entry", list(PARENTS))
@pytest.mark.parametrize("change,status", CASES, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in CASES])
def test_statuses_without_device_work(entry, change, status):
    a = {**KV, **QKV, **TAILS[entry], **NORM, **change}
    assert getattr(_lib.load(), entry)(*(a[n] for n in (*KV, *QKV, *TAILS[entry], *NORM)), None) == status


def test_head_dim_64_raises_value_error_before_device_work():
    norm = (torch.ones(128, dtype=torch.bfloat16), torch.ones(128, dtype=torch.bfloat16), 1e-6)
    c = PagedKVCache(num_layers=2, num_kv_heads=2, page_size=4, max_pages=8, batch=2, kind="bf16", device="cpu", head_dim=64)
    c.extend(1)
    x = torch.zeros((2, 2, 64), dtype=torch.bfloat16)
    for call in (lambda: c.append_rope(0, x, x, x, None, None, qk_norm=norm), lambda: c.prefill_fresh(0, x, x, x, None, None, qk_norm=norm),
                 lambda: c.decode_step(0, x, x, x, None, None, qk_norm=norm), lambda: mixedgemm.rope_qk(x, x, None, None, qk_norm=norm),
                 lambda: mixedgemm.rope_kv_append(c.kv_data, None, None, None, None, x, x, x, None, None, None, 0, qk_norm=norm),
                 lambda: mixedgemm.rope_kv_append_dense(c.kv_data, None, None, None, None, x, x, x, None, None, None, 0, qk_norm=norm),
                 lambda: mixedgemm.rope_append_decode(c.kv_data, None, None, None, None, x, x, x, None, None, 0, 8, qk_norm=norm)):
        with pytest.raises(ValueError, match="head_dim 64"):
            call()


def test_where_the_sum_is_exact_the_oracle_is_hfs_chain():
    """integers |x| <= 15: every partial sum of squares is an integer below 2^24, exact in any order"""
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.integers(-15, 16, (4096, 128)).astype(np.float32)).to(torch.bfloat16)
    w = torch.from_numpy(1 + 0.25 * rng.standard_normal(128).astype(np.float32)).to(torch.bfloat16)
    h = x.float()
    h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + 1e-6)
    hf = w * h.to(torch.bfloat16)
    bits = lambda t: t.contiguous().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(bits(hf), qo.qknorm(bits(x), bits(w), 1e-6))


@pytest.mark.parametrize("order", [qo.NATURAL, "linear"], ids=str)
def test_the_gaussian_case_tells_the_tree_from_another_order(order):
    """counted for seed 5: bits 0..5 in natural order move 4 q rows and 1 k row, a left-to-right sum 18 and 2"""
    q, k, _, qw, kw, eps = qo.gaussian_case()
    for x, w in ((q, qw), (k, kw)):
        assert (qo.qknorm(x, w, eps) != qo.qknorm(x, w, eps, order)).any()
