"""CPU tests of the paged KV cache surface: symbols, status codes without device work, Python argument checks, and the oracle's
quantization rule against the reference's quantize_int_group.  No kernel is launched here."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_oracle as ko


def test_symbols_declared_and_exported():
    lib = _lib.load()
    for name in ("mm_kv_append", "mm_paged_decode_workspace_bytes", "mm_paged_decode"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.mm_version() >= 600
    assert (_lib.MM_KV_INT4, _lib.MM_KV_BF16) == (0, 1)


def test_status_codes_without_device_work():
    lib = _lib.load()
    z, one = None, 16                       # non-null dummy pointers are never touched when the sizes are rejected
    tbl = (one, one, one)
    ok = dict(max_pages=4, L=2, layer=1, Hkv=8, P=16, hd=128, B=1)

    def append(kind=0, max_pages=4, L=2, layer=1, Hkv=8, P=16, hd=128, B=1, T=1, data=one, param=one):
        return lib.mm_kv_append(data, param, kind, max_pages, L, layer, Hkv, P, hd, *tbl, B, one, one, one, T, z)

    def decode(kind=0, max_pages=4, L=2, layer=1, Hkv=8, P=16, hd=128, B=1, Hq=32, msl=64, q=one, o=one, ws=z, wsb=0):
        return lib.mm_paged_decode(q, one, one, kind, max_pages, L, layer, Hkv, P, hd, *tbl, B, Hq, msl, 0.0, ws, wsb, o, z)

    assert append(hd=64) == _lib.MM_ERR_UNSUPPORTED
    assert decode(hd=256) == _lib.MM_ERR_UNSUPPORTED
    assert decode(Hq=8 * 17) == _lib.MM_ERR_UNSUPPORTED                       # g = 17
    for bad in (dict(kind=2), dict(P=0), dict(layer=2), dict(layer=-1), dict(L=0), dict(Hkv=0), dict(max_pages=0), dict(B=-1)):
        assert append(**bad) == _lib.MM_ERR_BAD_ARG, bad
        assert decode(**bad) == _lib.MM_ERR_BAD_ARG, bad
    assert append(T=-1) == _lib.MM_ERR_BAD_ARG
    assert append(data=z) == _lib.MM_ERR_BAD_ARG
    assert append(param=z) == _lib.MM_ERR_BAD_ARG                            # int4 needs params
    assert append(T=0) == _lib.MM_OK and append(B=0) == _lib.MM_OK           # nothing to do
    assert decode(Hq=30) == _lib.MM_ERR_BAD_ARG                               # not a multiple of Hkv
    assert decode(msl=-1) == _lib.MM_ERR_BAD_ARG
    assert decode(q=z) == _lib.MM_ERR_BAD_ARG and decode(o=z) == _lib.MM_ERR_BAD_ARG
    assert decode(B=0) == _lib.MM_OK
    need = lib.mm_paged_decode_workspace_bytes(1, 32, 8, 32768)
    assert need > 0
    assert decode(msl=32768) == _lib.MM_ERR_BAD_ARG                           # split needs a workspace
    assert decode(msl=32768, ws=one, wsb=need - 1) == _lib.MM_ERR_BAD_ARG     # too small
    assert decode(msl=32768, ws=one + 8, wsb=need) == _lib.MM_ERR_BAD_ARG     # not 16-byte aligned


def test_workspace_depends_on_host_values_only():
    lib = _lib.load()
    assert lib.mm_paged_decode_workspace_bytes(64, 32, 8, 1024) == 0         # enough work without a split: one launch
    assert lib.mm_paged_decode_workspace_bytes(1, 32, 8, 0) == 0
    assert lib.mm_paged_decode_workspace_bytes(1, 32, 8, 100) == 0
    a, b = lib.mm_paged_decode_workspace_bytes(1, 32, 8, 4096), lib.mm_paged_decode_workspace_bytes(1, 32, 8, 32768)
    assert 0 < a <= b and a % (32 * 130 * 4) == 0
    assert lib.mm_paged_decode_workspace_bytes(1, 30, 8, 4096) == 0           # invalid head counts


def test_python_argument_errors():
    i32 = lambda n: torch.zeros((n,), dtype=torch.int32)
    data = torch.zeros((4, 2, 2, 8, 16, 64), dtype=torch.uint8)
    param = torch.zeros((4, 2, 2, 8, 16, 2), dtype=torch.float16)
    k = torch.zeros((1, 8, 128), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.kv_append(data, param, i32(2), i32(4), i32(1), k, k, i32(2), 0)
    with pytest.raises(TypeError):
        mixedgemm.kv_append(data.float(), param, i32(2), i32(4), i32(1), k, k, i32(2), 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.paged_decode(torch.zeros((1, 32, 128), dtype=torch.bfloat16), data, param, i32(2), i32(4), i32(1), 0, 16)
    with pytest.raises(TypeError):
        mixedgemm.paged_decode(torch.zeros((1, 32, 128)), data, param, i32(2), i32(4), i32(1), 0, 16)
    with pytest.raises(ValueError):
        PagedKVCache(1, 8, 16, 4, 1, kind="fp8", device="cpu")
    with pytest.raises(ValueError):
        PagedKVCache(1, 8, 0, 4, 1, device="cpu")


def test_page_allocator_bookkeeping_on_host():
    c = PagedKVCache(2, 2, 4, 8, 3, kind="bf16", device="cpu")
    c.extend([5, 0, 4])
    assert c.seq_lens == [5, 0, 4] and c.kv_indptr.tolist() == [0, 2, 2, 3] and c.last_page_len.tolist() == [1, 0, 4]
    assert c.append_indptr.tolist() == [0, 5, 5, 9] and c.num_new_tokens == 9
    pages0 = c.kv_indices[:2].tolist()
    assert len(set(c.kv_indices[:3].tolist())) == 3
    c.extend(1)
    assert c.seq_lens == [6, 1, 5] and c.kv_indptr.tolist() == [0, 2, 3, 5] and c.last_page_len.tolist() == [2, 1, 1]
    assert c.kv_indices[:2].tolist() == pages0
    c.reset(0)
    assert c.seq_lens == [0, 1, 5] and c.kv_indptr.tolist() == [0, 0, 1, 3] and len(c._free) == 8 - 3
    with pytest.raises(RuntimeError, match="out of pages"):
        c.extend([40, 0, 0])


def quantize_int_group(w, nbits, group_size):
    """the reference's rule (model/qLlamaLayer.py:13-23), returning the codes as well"""
    w = w.reshape(-1, group_size)
    mx, mn = w.amax(dim=-1, keepdim=True), w.amin(dim=-1, keepdim=True)
    qmax = 2 ** nbits - 1
    scales = (mx - mn).clamp(min=1e-5) / qmax
    base = torch.round(-mn / scales).clamp_(min=0, max=qmax)
    codes = torch.clamp(torch.round(w / scales) + base, 0, qmax)
    return codes, scales, base, (codes - base) * scales


def test_oracle_rule_matches_quantize_int_group():
    """rows whose range is 15 x a power of two: the fp16 scale is exact, so the two rules agree code for code"""
    rng = np.random.default_rng(0)
    rows = []
    for e in range(-8, 6):
        s = 2.0 ** e
        for _ in range(20):
            lo = np.float32(rng.integers(-15, 1) * s + rng.integers(-3, 4) * s / 8)       # includes rows that do not straddle zero
            r = (lo + rng.random(128) * 15 * s).astype(np.float32)
            r[0], r[1] = lo, lo + np.float32(15 * s)
            rows.append(rng.permutation(r))
    x = np.stack(rows).astype(np.float32)
    assert np.allclose(x.max(1) - x.min(1), 15 * 2.0 ** np.repeat(np.arange(-8, 6), 20))
    codes, s, z = ko.quantize_row(x)
    tc, ts, tb, deq = quantize_int_group(torch.from_numpy(x), 4, 128)
    assert np.array_equal(s.astype(np.float32), ts.numpy()[:, 0])
    assert np.array_equal(codes, tc.numpy().astype(np.uint8))
    assert np.array_equal(z.astype(np.float32), (tb * ts).numpy()[:, 0])
    # dequantized: code * s - zero == (code - base) * s exactly here
    assert np.array_equal(codes.astype(np.float32) * s.astype(np.float32)[:, None] - z.astype(np.float32)[:, None], deq.numpy())


def test_oracle_packing_and_saturation():
    codes = np.arange(128, dtype=np.uint8) % 16
    packed = ko.pack_codes(codes)
    assert packed[0] == 0x10 and packed[7] == 0xFE and np.array_equal(ko.unpack_codes(packed), codes)
    c, s, z = ko.quantize_row(np.linspace(0, 3e6, 128, dtype=np.float32))
    assert s == np.float16(65504) and np.isfinite(z) and c.max() == 15                   # saturated scale, top codes clip
    c, s, z = ko.quantize_row(np.full(128, 3.0, dtype=np.float32))                        # constant row: scale from the 1e-5 floor
    assert s == np.float16(np.float32(1e-5) / np.float32(15)) and (c == 15).all() and z == 0
