"""CPU tests of the fp8 (e4m3) kind of the paged KV cache: the oracle's row and element rules (tests/kv_fp8_oracle.py) against their
definitions, the status codes that need no device work, the Python argument checks and the cache object's shapes.  No kernel runs."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
from oracle import mx_oracle as mo
import kv_fp8_oracle as fo
import kv_oracle as ko


def bf16(x):
    with np.errstate(over="ignore"):          # a row scaled past float32 becomes inf and is dropped by the caller
        return mo.f32_to_bf16(np.asarray(x, dtype=np.float32))


def row_with_amax(amax_bits, rng):
    """a row of bf16 bits whose largest magnitude is the bf16 number amax_bits (at a random place, with a random sign)"""
    amax = ko.bf16_to_f32(np.uint16(amax_bits)).astype(np.float64)
    r = bf16(rng.uniform(-1, 1, 128) * amax)
    r = np.where((r & 0x7FFF) > amax_bits, amax_bits, r).astype(np.uint16)
    r[rng.integers(128)] = amax_bits | (0x8000 if rng.integers(2) else 0)
    return r


def test_exponent_is_minimal_at_every_edge():
    """amax = 448 * 2^k, one bf16 step below and one above, for every k that maps into [-14, 15] and one beyond each end: the bit rule
    equals the definition, e = k at and below the edge and k + 1 one step above it (clamped at the ends)"""
    rng = np.random.default_rng(0)
    for k in range(fo.E_MIN - 1, fo.E_MAX + 2):
        edge = ((135 + k) << 7) | 96                                  # 448 * 2^k = 1.75 * 2^(k + 8) as bf16 bits
        assert ko.bf16_to_f32(np.uint16(edge)) == np.float32(448.0 * 2.0 ** k)
        for bits, want in ((edge - 1, k), (edge, k), (edge + 1, k + 1)):
            row = row_with_amax(bits, rng)
            e = int(fo.row_exponent(ko.bf16_to_f32(row)))
            assert e == int(fo.row_exponent_bits(row)) == min(max(want, fo.E_MIN), fo.E_MAX), (k, hex(bits))
            amax = float(ko.bf16_to_f32(np.uint16(bits)))
            assert amax <= 448.0 * 2.0 ** e or e == fo.E_MAX
            assert e == fo.E_MIN or amax > 448.0 * 2.0 ** (e - 1), "e is not the smallest"


def test_bit_rule_equals_definition_on_random_rows():
    rng = np.random.default_rng(1)
    x = bf16(rng.standard_normal((4000, 128)) * 2.0 ** rng.integers(-150, 128, (4000, 1)).astype(np.float64))
    x = x[np.isfinite(ko.bf16_to_f32(x)).all(-1)]
    assert len(x) > 3000
    assert np.array_equal(fo.row_exponent(ko.bf16_to_f32(x)), fo.row_exponent_bits(x))


def test_zero_and_denormal_rows():
    z = np.zeros((1, 128), dtype=np.uint16)
    codes, e = fo.quantize_row(z)
    assert e == fo.E_MIN and not codes.any()
    z[0, 5], z[0, 6] = 0x8000, 0x0001                               # -0.0 keeps its sign; a bf16 denormal rounds to zero at 2^14
    codes, e = fo.quantize_row(z)
    assert e == fo.E_MIN and codes[0, 5] == 0x80 and codes[0, 6] == 0 and np.count_nonzero(codes) == 1
    assert np.array_equal(fo.param_pair(e).view(np.uint16), [[(15 - 14) << 10, 0]])


def test_codes_are_never_nan_and_rows_saturate():
    rng = np.random.default_rng(2)
    x = bf16(rng.standard_normal((2000, 128)) * 2.0 ** rng.integers(-30, 128, (2000, 1)).astype(np.float64))
    x = x[np.isfinite(ko.bf16_to_f32(x)).all(-1)]
    x[0] = 0x7F7F                                                    # the largest bf16 everywhere: far above 448 * 2^15
    x[1] = 0xFF7F
    codes, e = fo.quantize_row(x)
    assert not ((codes & 0x7F) == 0x7F).any()
    assert e[0] == 15 and (codes[0] == 0x7E).all() and (codes[1] == 0xFE).all()
    sat = np.abs(ko.bf16_to_f32(x).astype(np.float64)) >= 448.0 * 2.0 ** 15
    assert sat.sum() > 256 and ((codes[sat] & 0x7F) == 0x7E).all()


def test_dequantized_values_are_bf16_and_within_2_pow_minus_4():
    rng = np.random.default_rng(3)
    x = bf16(rng.standard_normal((3000, 128)) * 2.0 ** rng.integers(-20, 21, (3000, 1)).astype(np.float64))
    codes, e = fo.quantize_row(x)
    deq = fo.dequantize(codes, fo.param_pair(e))                      # asserts that every value is a bf16 number
    val, ref = ko.bf16_to_f32(deq).astype(np.float64), ko.bf16_to_f32(x).astype(np.float64)
    normal = np.abs(ref) >= 2.0 ** (e[:, None] - 6)                   # normal in e4m3 at the row's scale
    assert normal.mean() > 0.9
    assert (np.abs(val - ref)[normal] <= 2.0 ** -4 * np.abs(ref)[normal]).all()
    half_step = np.broadcast_to(2.0 ** (e[:, None] - 10.0), ref.shape)            # half a subnormal step of the row's scale
    assert (np.abs(val - ref)[~normal] <= half_step[~normal]).all()
    assert np.array_equal(np.signbit(val), np.signbit(ref))
    # fp16 holds every scale exactly
    assert np.array_equal(fo.param_pair(e)[..., 0].astype(np.float64), 2.0 ** e)


def test_ties_round_to_the_even_code():
    """halfway between two e4m3 neighbours, in the normal (1 + (2 m + 1) / 16) and the subnormal ((2 m + 1) / 2 * 2^-9) range"""
    row = np.zeros(128, dtype=np.float32)
    row[0] = 448.0                                                   # e = 0
    for m in range(7):
        row[1 + m] = 1.0 + (2 * m + 1) / 16.0
        row[9 + m] = -(2 * m + 1) / 2.0 * 2.0 ** -9
    row[20] = 2.0 ** -10                                             # half the smallest subnormal: to code 0 (even)
    codes, e = fo.quantize_row(bf16(row)[None])
    assert e == 0 and codes[0, 0] == 0x7E
    for m in range(7):
        assert codes[0, 1 + m] == 0x38 + (m + 1) // 2 * 2, m
        assert codes[0, 9 + m] == 0x80 | ((m + 1) // 2 * 2), m
    assert codes[0, 20] == 0


def test_symbol_and_status_codes_without_device_work():
    lib = _lib.load()
    assert "mm_kv_dtype_supported" in _lib.EXPORTS and _lib.MM_KV_FP8_E4M3 == 3
    assert [lib.mm_kv_dtype_supported(c) for c in (-1, 0, 1, 2, 3, 4, 255)] == [0, 1, 1, 0, 1, 0, 0]
    assert lib.mm_version() == 660
    z, one = None, 16
    tbl = (one, one, one)

    def append(kind=3, B=1, T=1, param=one):
        return lib.mm_kv_append(one, param, kind, 4, 2, 1, 8, 16, 128, *tbl, B, one, one, one, T, z)

    def rope(kind=3, B=1, T=1, param=one):
        return lib.mm_rope_kv_append(one, param, kind, 4, 2, 1, 8, 16, 128, *tbl, B, one, one, one, 32 * 128, 32, one, one, 128, one, T, one, z)

    def decode(kind=3, B=1, param=one, window=None):
        a = (one, one, param, kind, 4, 2, 1, 8, 16, 128, *tbl, B, 32, 64, 0.0, z, 0, one, z)
        return lib.mm_paged_decode(*a) if window is None else lib.mm_paged_decode_window(*a, window)

    def prefill(kind=3, B=1, T=1, param=one, window=None):
        a = (one, one, T, one, param, kind, 4, 2, 1, 8, 16, 128, *tbl, B, 32, 64, 0.0, z, 0, one, z)
        return lib.mm_paged_prefill(*a) if window is None else lib.mm_paged_prefill_window(*a, window)

    assert append(T=0) == append(B=0) == rope(T=0) == _lib.MM_OK
    assert decode(B=0) == decode(B=0, window=5) == prefill(T=0) == prefill(B=0) == prefill(T=0, window=5) == _lib.MM_OK
    for call in (append, rope, decode, prefill):
        assert call(param=z) == _lib.MM_ERR_BAD_ARG, call.__name__        # fp8 needs its params, as int4 does
        assert call(kind=2) == _lib.MM_ERR_BAD_ARG, call.__name__         # code 2 stays unassigned
        assert call(kind=4) == _lib.MM_ERR_BAD_ARG, call.__name__
    assert decode(param=z, window=5) == prefill(param=z, window=5) == _lib.MM_ERR_BAD_ARG


def test_python_argument_errors():
    i32 = lambda n: torch.zeros((n,), dtype=torch.int32)
    data = torch.zeros((4, 2, 2, 8, 16, 128), dtype=torch.uint8)
    param = torch.zeros((4, 2, 2, 8, 16, 2), dtype=torch.float16)
    k = torch.zeros((1, 8, 128), dtype=torch.bfloat16)
    for d in (data, data.view(torch.float8_e4m3fn)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            mixedgemm.kv_append(d, param, i32(2), i32(4), i32(1), k, k, i32(2), 0)
        with pytest.raises(RuntimeError, match="no CPU path"):
            mixedgemm.paged_decode(torch.zeros((1, 32, 128), dtype=torch.bfloat16), d, param, i32(2), i32(4), i32(1), 0, 16)
    # a float8_e4m3fn cache is taken as its bytes (before this kind existed: TypeError); other dtypes still are not
    with pytest.raises(TypeError):
        mixedgemm.kv_append(data.view(torch.int8), param, i32(2), i32(4), i32(1), k, k, i32(2), 0)
    with pytest.raises(TypeError):
        mixedgemm.kv_append(data.view(torch.float8_e5m2), param, i32(2), i32(4), i32(1), k, k, i32(2), 0)


def test_cache_object_shapes():
    c = PagedKVCache(2, 4, 16, 8, 3, kind="fp8_e4m3", device="cpu", window=40)
    assert c.kv_data.dtype is torch.uint8 and tuple(c.kv_data.shape) == (8, 2, 2, 4, 16, 128)
    assert c.kv_param.dtype is torch.float16 and tuple(c.kv_param.shape) == (8, 2, 2, 4, 16, 2)
    assert c.kind == "fp8_e4m3" and c.window == 40
    c.extend([5, 0, 17])
    assert c.seq_lens == [5, 0, 17] and c.kv_indptr.tolist() == [0, 1, 1, 3]
    with pytest.raises(ValueError, match="fp8_e4m3"):
        PagedKVCache(1, 8, 16, 4, 1, kind="fp8", device="cpu")
    with pytest.raises(ValueError):
        PagedKVCache(1, 8, 16, 4, 1, kind="fp8_e5m2", device="cpu")


def test_oracle_append_walks_the_page_table():
    """ragged append with an empty sequence and a released page: only the target slots change, and they hold the row rule's bytes"""
    rng = np.random.default_rng(4)
    P, Hkv, lens, new = 4, 2, [6, 0, 9], [3, 0, 9]
    indptr, indices, last = np.array([0, 2, 2, 5]), np.array([3, 1, 0, -1, 4], dtype=np.int32), np.array([2, 0, 1])
    data = np.full((5, 1, 2, Hkv, P, 128), 0x7F, dtype=np.uint8)
    param = np.full((5, 1, 2, Hkv, P, 2), 0x7E00, dtype=np.uint16).view(np.float16)
    k, v = bf16(rng.standard_normal((12, Hkv, 128))), bf16(rng.standard_normal((12, Hkv, 128)) * 64)
    fo.append(data, param, indptr, indices, last, k, v, np.array([0, 3, 3, 12]), 0)
    written = (data != 0x7F).any(-1)                                   # [page, L, which, head, slot]
    want = np.zeros_like(written)
    want[3, 0, :, :, 3] = want[1, 0, :, :, :2] = True                  # sequence 0: positions 3, 4, 5
    want[0, 0, :, :, :] = want[4, 0, :, :, 0] = True                   # sequence 2: positions 0..3 and 8; 4..7 lie on the released page
    assert np.array_equal(written, want)
    codes, e = fo.quantize_row(v[3 + 8])
    assert np.array_equal(data[4, 0, 1, :, 0], codes) and np.array_equal(param[4, 0, 1, :, 0], fo.param_pair(e))
    assert np.array_equal(param.view(np.uint16)[..., 0] != 0x7E00, want)
