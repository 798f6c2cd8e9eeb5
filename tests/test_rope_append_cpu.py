"""CPU tests of the fused RoPE + KV append surface (mm_rope_kv_append, mixedgemm.rope_kv_append, PagedKVCache.append_rope): the numpy
oracle against torch's bf16 expression bit for bit, the symbol, the status codes without device work and the Python argument checks.
No kernel is launched here."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import rope_oracle as ro


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(b):
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16).copy()).view(torch.bfloat16)


def torch_rope(x, cos, sin):
    """HF apply_rotary_pos_emb (unsqueeze_dim = the head dim) on bf16 tensors: x [T, H, 128], cos / sin [T, 128]"""
    cos, sin = cos.unsqueeze(1), sin.unsqueeze(1)
    rot = torch.cat((-x[..., 64:], x[..., :64]), dim=-1)
    return (x * cos) + (rot * sin)


def check_against_torch(x_bits, cos_bits, sin_bits):
    want = bits(torch_rope(from_bits(x_bits), from_bits(cos_bits), from_bits(sin_bits)))
    got = ro.rope(x_bits, cos_bits, sin_bits)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} elements differ from torch's bf16 RoPE"


@pytest.mark.parametrize("scale", [1e-3, 1.0, 37.0])
def test_oracle_is_torch_bf16_rope_on_gaussian_rows(scale):
    rng = np.random.default_rng(int(scale * 1000))
    T, H = 257, 5
    x = ro.f32_to_bf16(rng.standard_normal((T, H, 128)).astype(np.float32) * np.float32(scale))
    cos, sin = ro.llama3_tables(rng.integers(0, 131072, T))
    check_against_torch(x, cos, sin)


def test_oracle_is_torch_bf16_rope_on_zeros_and_ties():
    """rows drawn from values whose products and sums land exactly between two bf16 numbers (1.5 * (1 + 2^-7), 2 + 2^-7, ...) and from
    +-0.0: round-half-even in each of the three roundings, and the sign of a zero"""
    rng = np.random.default_rng(5)
    f = np.float32
    vals = np.array([0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 2.0 ** -7, -(2.0 ** -7), 3 * 2.0 ** -7, -3 * 2.0 ** -7, 1 + 2.0 ** -7,
                     -(1 + 2.0 ** -7), 1.5 + 2.0 ** -7, 2.5, 4 + 2.0 ** -5, 1 + 3 * 2.0 ** -7], dtype=f)
    tabs = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 1 + 2.0 ** -7, -(1 + 2.0 ** -7), 1.5, 1 - 2.0 ** -8, 2.0 ** -7], dtype=f)
    T, H = 64, 3
    x = ro.f32_to_bf16(vals[rng.integers(0, len(vals), (T, H, 128))])
    cos = ro.f32_to_bf16(tabs[rng.integers(0, len(tabs), (T, 128))])
    sin = ro.f32_to_bf16(tabs[rng.integers(0, len(tabs), (T, 128))])
    xf, cf = ro.ko.bf16_to_f32(x), ro.ko.bf16_to_f32(cos)[:, None, :]
    prod = (xf * cf).view(np.uint32)
    assert ((prod & 0xFFFF) == 0x8000).sum() > 100, "the case is meant to hold products that are exact ties"
    check_against_torch(x, cos, sin)
    # the two extreme tables: identity, and rotate_half itself
    one, zero = np.full((T, 128), 0x3F80, np.uint16), np.zeros((T, 128), np.uint16)
    g = ro.f32_to_bf16(rng.standard_normal((T, H, 128)).astype(f))
    assert np.array_equal(ro.rope(g, one, zero), g)
    assert np.array_equal(ro.rope(g, zero, one), np.concatenate([g[..., 64:] ^ 0x8000, g[..., :64]], axis=-1))


def test_llama3_tables_match_hf_formula():
    pos = torch.tensor([0, 1, 4096, 131071])
    inv = 1.0 / (500000.0 ** (torch.arange(0, 128, 2, dtype=torch.int64).float() / 128))
    freqs = pos[:, None].float() * inv[None, :]
    emb = torch.cat((freqs, freqs), dim=-1)
    cos, sin = ro.llama3_tables(pos.numpy())
    # numpy's and torch's float32 pow may differ in the last place of inv_freq: at most 131071 * 2^-24 in the angle, so in cos and sin,
    # plus half a bf16 ulp of a value below 1 on either side (2^-8)
    for got, want in ((cos, emb.cos()), (sin, emb.sin())):
        assert np.abs(ro.ko.bf16_to_f32(got) - want.numpy()).max() <= 131071 * 2.0 ** -24 + 2.0 ** -8
    assert cos[0].tolist() == [0x3F80] * 128 and sin[0].tolist() == [0] * 128


def test_symbol_declared_and_exported():
    lib = _lib.load()
    assert "mm_rope_kv_append" in _lib.EXPORTS and hasattr(lib, "mm_rope_kv_append")
    assert lib.mm_version() >= 620
    assert "rope_kv_append" in mixedgemm.__all__ and callable(PagedKVCache.append_rope)


def test_status_codes_without_device_work():
    lib = _lib.load()
    z, one = None, 16                       # non-null dummy pointers are never touched when the arguments are rejected

    def call(kind=0, max_pages=4, L=2, layer=1, Hkv=8, P=16, hd=128, B=1, Hq=32, T=1, stride=48 * 128, cs=128, data=one, param=one,
             q=one, k=one, v=one, cos=one, sin=one, app=one, out=one, tbl=one):
        return lib.mm_rope_kv_append(data, param, kind, max_pages, L, layer, Hkv, P, hd, tbl, tbl, tbl, B, q, k, v, stride, Hq, cos, sin, cs,
                                     app, T, out, z)

    assert call(hd=64) == _lib.MM_ERR_UNSUPPORTED
    assert call(T=0) == _lib.MM_OK
    assert call(T=0, q=z, k=z, v=z, cos=z, sin=z, out=z) == _lib.MM_OK          # nothing to do, nothing to look at
    for name in ("data", "param", "q", "k", "v", "cos", "sin", "app", "out", "tbl"):
        assert call(**{name: z}) == _lib.MM_ERR_BAD_ARG, name
    assert call(kind=1, param=z, T=0) == _lib.MM_OK                              # the bf16 cache has no params
    for bad in (dict(stride=48 * 128 + 1), dict(cs=129), dict(stride=32 * 128 - 2), dict(cs=126), dict(stride=-2), dict(Hq=30), dict(Hq=0),
                dict(Hq=-8), dict(T=-1), dict(q=18), dict(k=18), dict(v=18), dict(cos=18), dict(sin=18), dict(out=18), dict(B=0),
                dict(kind=2), dict(P=0), dict(layer=2), dict(layer=-1), dict(L=0), dict(Hkv=0), dict(max_pages=0), dict(B=-1)):
        assert call(**bad) == _lib.MM_ERR_BAD_ARG, bad
    assert call(Hq=8 * 17, stride=8 * 19 * 128, T=0) == _lib.MM_OK               # no limit on g
    assert call(stride=32 * 128, T=0) == _lib.MM_OK                              # a stride of exactly the q row (Hq = Hkv callers)


def test_python_argument_errors():
    i32 = lambda n: torch.zeros((n,), dtype=torch.int32)
    data = torch.zeros((4, 2, 2, 8, 16, 64), dtype=torch.uint8)
    param = torch.zeros((4, 2, 2, 8, 16, 2), dtype=torch.float16)
    q, k = torch.zeros((1, 32, 128), dtype=torch.bfloat16), torch.zeros((1, 8, 128), dtype=torch.bfloat16)
    cs = torch.zeros((1, 128), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.rope_kv_append(data, param, i32(2), i32(4), i32(1), q, k, k, cs, cs, i32(2), 0)
    with pytest.raises(TypeError):
        mixedgemm.rope_kv_append(data.float(), param, i32(2), i32(4), i32(1), q, k, k, cs, cs, i32(2), 0)
    c = PagedKVCache(2, 8, 16, 4, 1, kind="bf16", device="cpu")
    c.extend(1)
    with pytest.raises(RuntimeError, match="announced by extend"):
        c.append_rope(0, torch.zeros((2, 32, 128), dtype=torch.bfloat16), k, k, cs, cs)
