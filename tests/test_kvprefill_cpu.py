"""CPU tests of causal multi-token attention over the paged KV cache (mm_paged_prefill, mixedgemm.paged_prefill,
PagedKVCache.attend_new): symbols, status codes without device work, the host-only split, Python argument checks, and the oracle
against the decode oracle and torch SDPA.  No kernel is launched here."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_oracle as ko
import kv_prefill_oracle as kpo


def test_symbols_declared_and_exported():
    lib = _lib.load()
    for name in ("mm_paged_prefill_workspace_bytes", "mm_paged_prefill"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.mm_version() >= 610


def test_status_codes_without_device_work():
    lib = _lib.load()
    z, one = None, 16                       # non-null dummy pointers are never touched when the sizes are rejected
    tbl = (one, one, one)

    def prefill(kind=0, max_pages=4, L=2, layer=1, Hkv=8, P=16, hd=128, B=1, Hq=32, T=4, msl=64, q=one, qo=one, data=one, param=one,
                o=one, ws=z, wsb=0):
        return lib.mm_paged_prefill(q, qo, T, data, param, kind, max_pages, L, layer, Hkv, P, hd, *tbl, B, Hq, msl, 0.0, ws, wsb, o, z)

    assert prefill(hd=64) == _lib.MM_ERR_UNSUPPORTED
    assert prefill(Hq=8 * 17) == _lib.MM_ERR_UNSUPPORTED                      # g = 17
    for bad in (dict(kind=2), dict(P=0), dict(layer=2), dict(layer=-1), dict(L=0), dict(Hkv=0), dict(max_pages=0), dict(B=-1),
                dict(Hq=30), dict(Hq=0), dict(T=-1), dict(msl=-1)):
        assert prefill(**bad) == _lib.MM_ERR_BAD_ARG, bad
    for null in ("q", "qo", "data", "param", "o"):
        assert prefill(**{null: z}) == _lib.MM_ERR_BAD_ARG, null
    assert prefill(T=0) == _lib.MM_OK and prefill(B=0) == _lib.MM_OK          # nothing to do
    need = lib.mm_paged_prefill_workspace_bytes(512, 1, 32, 8, 32768)
    assert need > 0
    big = dict(T=512, msl=32768)
    assert prefill(**big) == _lib.MM_ERR_BAD_ARG                              # split needs a workspace
    assert prefill(**big, ws=one, wsb=need - 1) == _lib.MM_ERR_BAD_ARG        # too small
    assert prefill(**big, ws=one + 8, wsb=need) == _lib.MM_ERR_BAD_ARG        # not 16-byte aligned


def test_workspace_depends_on_host_values_only():
    lib = _lib.load()
    ws = lib.mm_paged_prefill_workspace_bytes
    assert ws(4096, 1, 32, 8, 4096) == 0                                      # full prefill: enough tiles without a split
    assert ws(512, 1, 32, 8, 0) == 0 and ws(512, 1, 32, 8, 200) == 0          # nothing / too little to split
    a, b = ws(512, 1, 32, 8, 4096), ws(512, 1, 32, 8, 32768)
    assert 0 < a <= b
    tiles = 512 // 16 + 1                                                      # g = 4: 16 query tokens per tile; + B surplus
    assert a % (tiles * 8 * 64 * 130 * 4) == 0                                 # (tiles, Hkv, chunks, 64 rows, 128 + (m, l)) fp32
    assert ws(320, 64, 32, 8, 1029) > 0                                        # speculative verify 64 x 5 over 1k
    for bad in ((0, 1, 32, 8, 4096), (512, 0, 32, 8, 4096), (512, 1, 30, 8, 4096), (512, 1, 32, 8, -1), (512, 1, 8 * 17, 8, 4096)):
        assert ws(*bad) == 0, bad
    # identical host values give identical sizes whatever the page table will hold
    assert ws(64, 4, 32, 8, 2048) == ws(64, 4, 32, 8, 2048)


def test_python_argument_errors():
    i32 = lambda n: torch.zeros((n,), dtype=torch.int32)
    data = torch.zeros((4, 2, 2, 8, 16, 64), dtype=torch.uint8)
    param = torch.zeros((4, 2, 2, 8, 16, 2), dtype=torch.float16)
    q = torch.zeros((5, 32, 128), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.paged_prefill(q, data, param, i32(2), i32(4), i32(1), i32(2), 0, 16)
    with pytest.raises(TypeError):
        mixedgemm.paged_prefill(q.float(), data, param, i32(2), i32(4), i32(1), i32(2), 0, 16)
    c = PagedKVCache(1, 8, 16, 8, 2, kind="int4", device="cpu")
    c.extend([3, 2])
    assert c.num_new_tokens == 5
    with pytest.raises(RuntimeError, match="5 tokens announced"):
        c.attend_new(0, torch.zeros((4, 32, 128), dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="5 tokens announced"):
        c.attend_new(0, torch.zeros((5, 32), dtype=torch.bfloat16))


def _random_cache(kind, lens, Hkv, P, rng, L=1, layer=0):
    """host cache with random contents and a shuffled page table"""
    npg = [-(-n // P) for n in lens]
    max_pages = sum(npg) + 2
    perm = rng.permutation(max_pages)[: sum(npg)].astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(npg)]).astype(np.int32)
    last = np.array([n - (k - 1) * P if k else 0 for n, k in zip(lens, npg)], dtype=np.int32)
    if kind == "int4":
        data = rng.integers(0, 256, (max_pages, L, 2, Hkv, P, 64)).astype(np.uint8)
        param = np.stack([rng.uniform(0.05, 0.3, (max_pages, L, 2, Hkv, P)), rng.uniform(0, 1, (max_pages, L, 2, Hkv, P))],
                         -1).astype(np.float16)
    else:
        data = (rng.standard_normal((max_pages, L, 2, Hkv, P, 128)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        param = None
    return data, param, indptr, perm, last


def _bf16_bits(x):
    return (np.asarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_oracle_single_token_equals_decode_oracle(kind):
    rng = np.random.default_rng(1)
    lens = [0, 1, 17, 40]
    data, param, indptr, indices, last = _random_cache(kind, lens, 4, 8, rng)
    q = _bf16_bits(rng.standard_normal((4, 16, 128)))
    want = ko.attention(q, data, param, indptr, indices, last, 0)
    got = kpo.attention(q, data, param, indptr, indices, last, np.arange(5), 0)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)


def test_oracle_square_prefill_equals_sdpa_causal():
    rng = np.random.default_rng(2)
    n, Hq, Hkv = 37, 8, 2
    data, param, indptr, indices, last = _random_cache("bf16", [n], Hkv, 16, rng)
    q = _bf16_bits(rng.standard_normal((n, Hq, 128)))
    got = kpo.attention(q, data, param, indptr, indices, last, np.array([0, n]), 0)
    K, V = ko.dequantized(data, param, indptr, indices, last, 0, 0)                  # [Hkv, n, 128]
    qt = torch.from_numpy(ko.bf16_to_f32(q).astype(np.float64)).transpose(0, 1)      # [Hq, n, 128]
    kt = torch.from_numpy(K).repeat_interleave(Hq // Hkv, 0)
    vt = torch.from_numpy(V).repeat_interleave(Hq // Hkv, 0)
    ref = torch.nn.functional.scaled_dot_product_attention(qt, kt, vt, is_causal=True).transpose(0, 1).numpy()
    assert np.allclose(got, ref, rtol=1e-10, atol=1e-10)


def test_oracle_bottom_right_and_uncounted_tokens():
    """2 new tokens over 5 cached: they sit at positions 5 and 6; a table that does not count them gives zeros"""
    rng = np.random.default_rng(3)
    data, param, indptr, indices, last = _random_cache("bf16", [7], 1, 4, rng)
    q = _bf16_bits(rng.standard_normal((2, 1, 128)))
    got = kpo.attention(q, data, param, indptr, indices, last, np.array([0, 2]), 0)
    one = lambda t: kpo.attention(q[t:t + 1], data, param, indptr, indices, last, np.array([0, 1]), 0)[0]
    # position 6 sees all 7 tokens: the single-token (decode) answer
    assert np.allclose(got[1], one(1))
    K, V = ko.dequantized(data, param, indptr, indices, last, 0, 0)
    s = K[0, :6] @ ko.bf16_to_f32(q[0, 0]).astype(np.float64) / np.sqrt(128)
    p = np.exp(s - s.max())
    assert np.allclose(got[0, 0], p @ V[0, :6] / p.sum())
    # a table of 1 token with 2 queries: the first query's position is -1, it attends nothing
    short = kpo.attention(q, data, param, np.array([0, 1]), indices, np.array([1], dtype=np.int32), np.array([0, 2]), 0)
    assert np.count_nonzero(short[0]) == 0 and np.allclose(short[1, 0], V[0, 0])
    empty = kpo.attention(q, data, param, np.array([0, 0]), indices, np.array([0], dtype=np.int32), np.array([0, 2]), 0)
    assert np.count_nonzero(empty) == 0
