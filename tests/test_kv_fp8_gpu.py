"""GPU tests of the fp8 (e4m3) kind of the paged KV cache (MM_KV_FP8_E4M3; PagedKVCache(kind="fp8_e4m3")).  The row and element rules
are proved on the CPU in tests/test_kv_fp8_cpu.py; here every comparison but those of section 3 is bit for bit.

1 append   kv_append and rope_kv_append, byte for byte against tests/kv_fp8_oracle.py: Gaussian rows at scales 2^-20 .. 2^20, the amax
           edges 448 * 2^k and one bf16 step to either side, ties in the normal and the subnormal range, saturating rows, zero rows,
           -0.0; P in {1, 16, 24}, a ragged append_indptr with an empty sequence, a token on a released page
2 twin     paged_decode / paged_prefill over an fp8 cache are BIT-EQUAL to the same call over a bf16 cache that holds the dequantized
           values: every row scale is a power of two, so it factors out of each dot product, of p * s_v and of every rounding between
3 fp64     against the fp64 oracles over the dequantized cache, with the bounds of test_kvcache_gpu.py / test_kvprefill_gpu.py
4 needle   one token takes the softmax mass to far below 2^-20: the output is its (dequantized) V row within 1 bf16 ulp, the needle on
           the first and last token of a tile, a page and a chunk
5 poison   0x7F codes and NaN params in every slot outside the sequences and on every released page: bit-equal to the clean cache
6 object   PagedKVCache(kind="fp8_e4m3", window=W): one hipGraph of append + attend / attend_new replayed across page releases
7 end      kv_data and kv_param placed so that the last row touched ends where its allocation ends (a correct run)

No bound here comes from what a kernel produced."""
import ctypes

import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
from oracle import mx_oracle as mo
import kv_exact_cases as kc
import kv_fp8_oracle as fo
import kv_oracle as ko
import kv_window_cases as wc
import kv_window_oracle as kwo
import rope_oracle as ro
import test_kvcache_gpu as t_dec
import test_kvprefill_gpu as t_pre

pytestmark = pytest.mark.gpu

L, LAYER = 2, 1
NAN16 = 0x7E00


def i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def tb(bits, dev):
    """uint16 bf16 bits -> bf16 tensor"""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16).to(dev)


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def rows(rng, shape, lo=-3, hi=3):
    """bf16 bits: N(0, 1) times 2^k, k in lo .. hi drawn per row"""
    k = rng.integers(lo, hi + 1, tuple(shape[:-1]) + (1,)).astype(np.float64)
    return mo.f32_to_bf16((rng.standard_normal(shape) * 2.0 ** k).astype(np.float32))


def empty(max_pages, Hkv, P, dev, poison):
    data = torch.full((max_pages, L, 2, Hkv, P, 128), 0x7F if poison else 0, dtype=torch.uint8, device=dev)
    param = torch.full((max_pages, L, 2, Hkv, P, 2), NAN16 if poison else 0, dtype=torch.int16, device=dev).view(torch.float16)
    return data, param


def make_cache(kb, vb, lens, P, dev, poison=False, seed=0):
    """an fp8 cache whose layer LAYER holds the sequences' K / V (kv_append), shuffled pages, page 0 unreferenced; everything else keeps
    the initial fill: zeros, or 0x7F codes with NaN params (poison)"""
    indptr, indices, last, max_pages = kc.page_table(lens, P, seed)
    data, param = empty(max_pages, kb.shape[1], P, dev, poison)
    tbl = [i32(a, dev) for a in (indptr, indices, last)]
    mixedgemm.kv_append(data, param, *tbl, tb(kb, dev), tb(vb, dev), i32(kc.indptr_of(lens), dev), LAYER)
    return dict(data=data, param=param, tbl=tbl, tbl_h=(indptr, indices, last), lens=list(lens), P=P)


def gauss_cache(lens, Hkv, P, dev, seed, poison=False):
    rng = np.random.default_rng(seed)
    cache = make_cache(rows(rng, (sum(lens), Hkv, 128)), rows(rng, (sum(lens), Hkv, 128)), lens, P, dev, poison, seed)
    return cache, rng


def dequantized_host(cache):
    return fo.dequantize(cache["data"].cpu().numpy(), cache["param"].cpu().numpy())


def twin_of(cache):
    """the bf16 cache that holds the fp8 cache's dequantized values, same page table"""
    return dict(cache, data=tb(dequantized_host(cache), cache["data"].device), param=None)


def decode(cache, q, msl, W=None, tbl=None):
    return mixedgemm.paged_decode(q, cache["data"], cache["param"], *(tbl or cache["tbl"]), LAYER, msl, window=W)


def prefill(cache, q, new, msl, W=None, tbl=None):
    return mixedgemm.paged_prefill(q, cache["data"], cache["param"], *(tbl or cache["tbl"]), i32(kc.indptr_of(new), q.device), LAYER, msl,
                                   window=W)


def same_bits(a, b, what):
    a, b = bits(a).astype(np.int64), bits(b).astype(np.int64)
    bad = a != b
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} outputs differ, first at {tuple(int(i) for i in np.argwhere(bad)[0])}: "
                           f"{int(a[bad][0]):#06x} vs {int(b[bad][0]):#06x}")


# ---- 1. append -------------------------------------------------------------------------------------------------------------------
def edge_rows(rng, n_gauss):
    """uint16 [n, 128]: the rows named in the module docstring"""
    out = [rows(rng, (n_gauss, 128), -20, 20)]
    edges = []
    for k in range(fo.E_MIN - 1, fo.E_MAX + 2):
        edge = ((135 + k) << 7) | 96                                       # 448 * 2^k
        for amax in (edge - 1, edge, edge + 1):
            r = mo.f32_to_bf16((rng.uniform(-1, 1, 128) * float(ko.bf16_to_f32(np.uint16(amax)))).astype(np.float32))
            r = np.where((r & 0x7FFF) > amax, amax, r).astype(np.uint16)
            r[rng.integers(128)] = amax | (0x8000 if rng.integers(2) else 0)
            edges.append(r)
    out.append(np.stack(edges))
    for k in (-14, -3, 0, 5, 15):                                          # ties at the row scale 2^k: normal and subnormal halves
        t = np.zeros(128, dtype=np.float64)
        t[0] = 448.0
        for e in range(-6, 8):
            for m in range(8):
                t[1 + (e + 6) * 8 + m] = (1.0 + (2 * m + 1) / 16.0) * 2.0 ** e * (-1) ** m
        t[113:120] = [(2 * m + 1) / 2.0 * 2.0 ** -9 for m in range(7)]
        t[120:127] = [-(2 * m + 1) / 2.0 * 2.0 ** -9 for m in range(7)]
        t[127] = 2.0 ** -10
        t = np.where(np.abs(t) > 448.0, 0.0, t) * 2.0 ** k
        tie = mo.f32_to_bf16(t.astype(np.float32))
        assert np.array_equal(ko.bf16_to_f32(tie).astype(np.float64), t), "the tie values must be bf16 numbers"
        out.append(tie[None])
    sat = rows(rng, (4, 128), 100, 120)                                    # amax far above 448 * 2^15: the clamp acts
    sat[0, :4] = [0x7F7F, 0xFF7F, 0x7F00, 0x0001]
    assert (np.abs(ko.bf16_to_f32(sat).astype(np.float64)).max(-1) > 448.0 * 2.0 ** 15).all() and np.isfinite(ko.bf16_to_f32(sat)).all()
    out.append(sat)
    zero = np.zeros((3, 128), dtype=np.uint16)
    zero[1, ::3] = 0x8000                                                  # -0.0 among +0.0
    zero[2, 5], zero[2, 9], zero[2, 70] = 0x8000, 0x0001, 0x807F           # a denormal row with a -0.0
    out.append(zero)
    return np.concatenate(out)


@pytest.fixture(scope="module")
def append_inputs():
    rng = np.random.default_rng(11)
    Hkv = 2
    er = edge_rows(rng, 40)
    n = len(er) // Hkv * Hkv
    k = rng.permutation(er[:n]).reshape(-1, Hkv, 128)
    v = rng.permutation(er[:n]).reshape(-1, Hkv, 128)
    return k, v


def append_layout(T, P, rng):
    """four sequences, the second empty, appended to priors of 0 / 0 / 5 / P + 1 tokens; one page entry of the last sequence is -1"""
    new = [T // 3, 0, T // 3, T - 2 * (T // 3)]
    prior = [0, 0, 5, P + 1]
    lens = [a + n for a, n in zip(prior, new)]
    indptr, indices, last, max_pages = kc.page_table(lens, P, 5, free_page0=False)
    indices = indices.copy()
    gone = int(indptr[3]) + (prior[3] + new[3] // 2) // P                  # a page in the middle of the last sequence's new tokens
    indices[gone] = -1
    return new, lens, (indptr, indices, last), max_pages


@pytest.mark.parametrize("P", [1, 16, 24])
def test_kv_append_bytes(dev, append_inputs, P):
    kb, vb = append_inputs
    T, Hkv = kb.shape[0], kb.shape[1]
    new, lens, tbl_h, max_pages = append_layout(T, P, None)
    data, param = empty(max_pages, Hkv, P, dev, poison=True)
    want_d, want_p = data.cpu().numpy(), param.cpu().numpy()
    app = kc.indptr_of(new)
    mixedgemm.kv_append(data, param, *(i32(a, dev) for a in tbl_h), tb(kb, dev), tb(vb, dev), i32(app, dev), LAYER)
    torch.cuda.synchronize()
    fo.append(want_d, want_p, *tbl_h, kb, vb, app, LAYER)
    got_d, got_p = data.cpu().numpy(), param.cpu().numpy().view(np.uint16)
    written = (want_d != 0x7F).any(-1).sum()
    assert T * Hkv * 2 - 2 * Hkv * P <= written < T * Hkv * 2, "the released page must have dropped some tokens, and only those"
    bad = got_d != want_d
    assert not bad.any(), f"{int(bad.sum())} cache bytes differ; first at {tuple(int(i) for i in np.argwhere(bad)[0])}"
    assert np.array_equal(got_p, want_p.view(np.uint16)), "params differ"
    assert not ((got_d[:, LAYER] & 0x7F) == 0x7F)[(want_d[:, LAYER] != 0x7F).any(-1)].any(), "a NaN code was written"


@pytest.mark.parametrize("P", [1, 16, 24])
def test_rope_kv_append_bytes(dev, append_inputs, P):
    """the cache bytes equal kv_append(rope(k), v); k at moderate scales so that the rotation stays finite"""
    _, vb = append_inputs
    rng = np.random.default_rng(12)
    T, Hkv, Hq = vb.shape[0], vb.shape[1], 6
    kb, qb = rows(rng, (T, Hkv, 128), -20, 20), rows(rng, (T, Hq, 128))
    cos, sin = ro.llama3_tables(rng.integers(0, 100000, T))
    new, lens, tbl_h, max_pages = append_layout(T, P, None)
    data, param = empty(max_pages, Hkv, P, dev, poison=True)
    want_d, want_p = data.cpu().numpy(), param.cpu().numpy()
    app = kc.indptr_of(new)
    q_rot = mixedgemm.rope_kv_append(data, param, *(i32(a, dev) for a in tbl_h), tb(qb, dev), tb(kb, dev), tb(vb, dev), tb(cos, dev),
                                     tb(sin, dev), i32(app, dev), LAYER)
    torch.cuda.synchronize()
    fo.append(want_d, want_p, *tbl_h, ro.rope(kb, cos, sin), vb, app, LAYER)
    assert np.array_equal(data.cpu().numpy(), want_d), "cache bytes differ from kv_append(rope(k), v)"
    assert np.array_equal(param.cpu().numpy().view(np.uint16), want_p.view(np.uint16)), "params differ"
    assert np.array_equal(bits(q_rot), ro.rope(qb, cos, sin)), "rotated q differs"
    # and from the op itself: kv_append of the rotated k writes the same bytes
    data2, param2 = empty(max_pages, Hkv, P, dev, poison=True)
    mixedgemm.kv_append(data2, param2, *(i32(a, dev) for a in tbl_h), tb(ro.rope(kb, cos, sin), dev), tb(vb, dev), i32(app, dev), LAYER)
    assert torch.equal(data, data2) and torch.equal(param.view(torch.int16), param2.view(torch.int16))


def test_python_geometry_errors(dev):
    param = torch.zeros((4, 2, 2, 8, 16, 2), dtype=torch.float16, device=dev)
    for shape in ((4, 2, 2, 8, 16, 96), (4, 2, 3, 8, 16, 128), (4, 2, 2, 8, 16)):
        with pytest.raises(RuntimeError, match=r"64\] uint8 \(int4\).*128\] uint8 / float8_e4m3fn \(fp8\).*bf16 cache"):
            mixedgemm._kv_geometry(torch.zeros(shape, dtype=torch.uint8, device=dev), param, dev.index)
    data = torch.zeros((4, 2, 2, 8, 16, 128), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="kv_param must be"):
        mixedgemm._kv_geometry(data, param[:, :, :, :, :8].contiguous(), dev.index)
    kind, max_pages, Ln, Hkv, P, seen = mixedgemm._kv_geometry(data.view(torch.float8_e4m3fn), param, dev.index)
    assert (kind, max_pages, Ln, Hkv, P) == (3, 4, 2, 8, 16) and seen.dtype is torch.uint8 and seen.data_ptr() == data.data_ptr()
    assert mixedgemm._kv_geometry(torch.zeros((4, 2, 2, 8, 16, 64), dtype=torch.uint8, device=dev), param, dev.index)[0] == _lib.MM_KV_INT4
    with pytest.raises(RuntimeError, match="int4 cache.*fp8 cache.*kv_param"):
        mixedgemm._kv_geometry(torch.zeros((4, 2, 2, 8, 16, 64), dtype=torch.bfloat16, device=dev), None, dev.index)


def test_float8_tensor_is_the_same_cache(dev):
    cache, rng = gauss_cache([40, 3], 2, 16, dev, 13)
    q = tb(rows(rng, (2, 8, 128)), dev)
    as_f8 = dict(cache, data=cache["data"].view(torch.float8_e4m3fn))
    same_bits(decode(as_f8, q, 40), decode(cache, q, 40), "float8_e4m3fn view")
    k = tb(rows(rng, (43, 2, 128)), dev)
    d2, p2 = empty(cache["data"].size(0), 2, 16, dev, False)
    mixedgemm.kv_append(d2.view(torch.float8_e4m3fn), p2, *cache["tbl"], k, k, i32(kc.indptr_of([40, 3]), dev), LAYER)
    assert d2[:, LAYER].any() and not d2[:, 0].any()


# ---- 2. twin equality ------------------------------------------------------------------------------------------------------------
LENS = [1, 31, 32, 33, 127, 128, 129, 300]
WINDOWS = [None, 1, 32, 33, 64, 129]
GS, PS = [1, 4, 8, 16], [1, 16, 24]


@pytest.fixture(scope="module")
def twin_caches(dev):
    """per page size: the fp8 cache of LENS (two kv heads) and its bf16 twin, built once"""
    out = {}
    for P in PS:
        cache, rng = gauss_cache(LENS, 2, P, dev, 20 + P)
        out[P] = (cache, twin_of(cache))
    return out


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("g", GS)
def test_twin_decode(dev, twin_caches, g, P):
    cache, twin = twin_caches[P]
    rng = np.random.default_rng(100 * g + P)
    q = tb(rows(rng, (len(LENS), 2 * g, 128)), dev)
    for W in WINDOWS:
        for msl in (max(LENS), 5000):
            same_bits(decode(cache, q, msl, W), decode(twin, q, msl, W), f"decode g={g} P={P} W={W} bound {msl}")


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("g", GS)
def test_twin_prefill(dev, twin_caches, g, P):
    cache, twin = twin_caches[P]
    rng = np.random.default_rng(200 * g + P)
    for n in (1, 5, 64 // g, 64 // g + 1):
        new = [min(n, l) for l in LENS]
        q = tb(rows(rng, (sum(new), 2 * g, 128)), dev)
        for W in WINDOWS:
            same_bits(prefill(cache, q, new, max(LENS), W), prefill(twin, q, new, max(LENS), W), f"prefill g={g} P={P} n_b={n} W={W}")


@pytest.mark.parametrize("g", GS)
def test_twin_split_path(dev, g):
    """B * Hkv = 1 with max_seq_len 600: three chunks and the merge launch, in decode and in prefill"""
    assert mixedgemm.paged_decode_workspace_bytes(1, g, 1, 600) == 3 * g * (128 + 2) * 4
    for n_tok in (600, 300, 257):
        cache, rng = gauss_cache([n_tok], 1, 16, dev, 30 + g)
        twin = twin_of(cache)
        q = tb(rows(rng, (1, g, 128)), dev)
        for W in (None, 129, 599):
            same_bits(decode(cache, q, 600, W), decode(twin, q, 600, W), f"decode g={g} length {n_tok} W={W}")
        for n in (5, 64 // g + 1):
            assert mixedgemm.paged_prefill_workspace_bytes(n, 1, g, 1, 600) > 0, "must take the split path"
            qp = tb(rows(rng, (n, g, 128)), dev)
            for W in (None, 129, 599):
                same_bits(prefill(cache, qp, [n], 600, W), prefill(twin, qp, [n], 600, W), f"prefill g={g} length {n_tok} n_b={n} W={W}")


# ---- 3. fp64 oracle over the dequantized cache ----------------------------------------------------------------------------------------
# (Hq, Hkv, P, lens, W)
ORACLE_DECODE = [(8, 2, 16, [0, 1, 99, 100, 101, 700, 33], None), (5, 1, 24, [300, 64, 65, 600], 64), (16, 1, 1, [40, 17, 0], 33),
                 (32, 8, 16, [1, 257, 512], None)]


@pytest.mark.parametrize("case", range(len(ORACLE_DECODE)))
def test_decode_against_fp64(dev, case):
    Hq, Hkv, P, lens, W = ORACLE_DECODE[case]
    cache, rng = gauss_cache(lens, Hkv, P, dev, 40 + case)
    q = tb(rows(rng, (len(lens), Hq, 128), -1, 1), dev)
    o = decode(cache, q, max(lens), W)
    torch.cuda.synchronize()
    hd = dequantized_host(cache)
    want = kwo.decode_attention(bits(q), hd, None, *cache["tbl_h"], LAYER, W)
    for b, n in enumerate(lens):
        if n == 0:
            assert int(torch.count_nonzero(o[b].float())) == 0
    t_dec.check_attention(o, want, float(np.abs(ko.bf16_to_f32(hd[:, LAYER, 1])).max()))


# (Hq, Hkv, P, prior, new, W)
ORACLE_PREFILL = [(8, 2, 16, [0, 90, 5, 400, 100], [100, 10, 0, 70, 1], None), (5, 1, 24, [100, 0, 500], [65, 64, 13], 64),
                  (16, 1, 1, [3, 200], [17, 9], 33), (32, 8, 16, [0, 300], [130, 3], None)]


@pytest.mark.parametrize("case", range(len(ORACLE_PREFILL)))
def test_prefill_against_fp64(dev, case):
    Hq, Hkv, P, prior, new, W = ORACLE_PREFILL[case]
    lens = [a + n for a, n in zip(prior, new)]
    cache, rng = gauss_cache(lens, Hkv, P, dev, 50 + case)
    q = tb(rows(rng, (sum(new), Hq, 128), -1, 1), dev)
    o = prefill(cache, q, new, max(lens), W)
    torch.cuda.synchronize()
    hd, qo = dequantized_host(cache), kc.indptr_of(new)
    want = kwo.prefill_attention(bits(q), hd, None, *cache["tbl_h"], qo, LAYER, W)
    t_pre.check(o, want, kwo.prefill_vmax(tuple(q.shape), hd, None, *cache["tbl_h"], qo, LAYER, W), f"case {case}")


# ---- 4. needle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["decode", "prefill"])
@pytest.mark.parametrize("P, W", [(16, None), (24, None), (1, 129), (16, 129)])
def test_needle(dev, mode, P, W):
    """q = 4 in every dim, the needle's K row = +2 and every other K row = -2 (exact in e4m3 at the row scale 2^-7): the needle leads
    by 2 * 128 * 8 / sqrt(128) = 181 nats, so every other p underflows to 0 and o is the needle's V row, rounded once.  600 tokens,
    B = 1, twelve kv heads each with its own needle position: three chunks of 256 tokens in both kernels"""
    N, g, n_new = 600, 2, 5
    lo = 0 if W is None else N - W                                # the lowest position every query attends (the last one's window)
    top = N - 1 if mode == "decode" else N - n_new                # ... and the highest (the first query's own position)
    want_pos = [0, 31, 32, 63, 64, P - 1, P, 2 * P - 1, 255, 256, 511, 512]
    if W is not None:                                             # the same edges, those inside the window, and the window's own
        want_pos = [lo, lo + 1, top, lo + 31, lo + 32] + [p for p in (479, 480, 495, 496, 511, 512, 527, 528, 575, 576) if lo <= p <= top]
    pos = ([p for p in want_pos if lo <= p <= top] + [top] * 12)[:12]
    Hkv = len(pos)
    rng = np.random.default_rng(60 + P)
    kf = np.full((N, Hkv, 128), -2.0, dtype=np.float32)
    kf[pos, np.arange(Hkv)] = 2.0
    cache = make_cache(mo.f32_to_bf16(kf), rows(rng, (N, Hkv, 128)), [N], P, dev, poison=True, seed=P)
    if mode == "decode":
        assert mixedgemm.paged_decode_workspace_bytes(1, Hkv * g, Hkv, N, W) > 0 or W is not None
        q = tb(mo.f32_to_bf16(np.full((1, Hkv * g, 128), 4.0, dtype=np.float32)), dev)
        o = decode(cache, q, N, W)
    else:
        q = tb(mo.f32_to_bf16(np.full((n_new, Hkv * g, 128), 4.0, dtype=np.float32)), dev)
        o = prefill(cache, q, [n_new], N, W)
    torch.cuda.synchronize()
    hd = dequantized_host(cache)
    kd, vd = ko.dequantized(hd, None, *cache["tbl_h"], LAYER, 0)                       # [Hkv, N, 128]
    assert np.array_equal(kd, kf.transpose(1, 0, 2).astype(np.float64)), "the K rows must be exact in the cache"
    want = np.repeat(vd[np.arange(Hkv), pos], g, axis=0)[None]                         # [1, Hq, 128]
    got = o.float().cpu().numpy().astype(np.float64)
    err, ulp = np.abs(got - want), kc.bf16_ulp(want)
    assert (err <= ulp).all(), f"{int((err > ulp).sum())} outputs beyond 1 ulp of the needle's V row; heads {sorted(set(np.argwhere(err > ulp)[:, 1].tolist()))}, positions {pos}"


# ---- 5. poison ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PS)
def test_poison_outside_the_sequences_and_on_released_pages(dev, P):
    Hq, Hkv, W = 8, 2, 100
    prior, new = [0, 500, 140, 99, 300], [90, 1, 70, 3, 1]
    lens = [a + n for a, n in zip(prior, new)]
    clean, rng = gauss_cache(lens, Hkv, P, dev, 70 + P)
    dirty, _ = gauss_cache(lens, Hkv, P, dev, 70 + P, poison=True)
    hd = dirty["data"].cpu().numpy()
    assert (hd[0] == 0x7F).all() and (hd[:, 0] == 0x7F).all(), "page 0 and the other layer keep the poison"
    q = tb(rows(rng, (len(lens), Hq, 128)), dev)
    qp = tb(rows(rng, (sum(new), Hq, 128)), dev)
    for Wn in (None, W):
        for msl in (max(lens), 9000):
            o = decode(dirty, q, msl, Wn)
            assert torch.isfinite(o.float()).all()
            same_bits(o, decode(clean, q, msl, Wn), f"decode P={P} W={Wn} bound {msl}")
            o = prefill(dirty, qp, new, msl, Wn)
            assert torch.isfinite(o.float()).all()
            same_bits(o, prefill(clean, qp, new, msl, Wn), f"prefill P={P} W={Wn} bound {msl}")
    # released pages: their entries -1, their bytes poison
    indptr, indices, last = dirty["tbl_h"]
    for n_rel, run, base in (([1] * len(lens), lambda c, t: decode(c, q, max(lens), W, t), decode(clean, q, max(lens), W)),
                             (new, lambda c, t: prefill(c, qp, new, max(lens), W, t), prefill(clean, qp, new, max(lens), W))):
        gone = wc.released_entries(indptr, lens, n_rel, P, W)
        assert gone, "the case must release something"
        data, param = dirty["data"].clone(), dirty["param"].clone()
        pages = torch.from_numpy(indices[gone].astype(np.int64)).to(dev)
        data[pages] = 0x7F
        param.view(torch.int16)[pages] = NAN16
        idx = indices.copy()
        idx[gone] = -1
        o = run(dict(dirty, data=data, param=param), [dirty["tbl"][0], i32(idx, dev), dirty["tbl"][2]])
        assert torch.isfinite(o.float()).all()
        same_bits(o, base, f"released pages P={P}")


# ---- 6. the cache object under graph capture -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["attend", "attend_new"])
def test_graph_capture_across_page_releases(dev, mode):
    """append + attend (attend_new with 5 tokens per sequence) captured once, replayed over extend steps that release pages"""
    B, Hq, Hkv, P, W = 3, 8, 2, 16, 40
    n = 1 if mode == "attend" else 5
    cache = PagedKVCache(1, Hkv, P, 24, B, kind="fp8_e4m3", device=dev, window=W, max_seq_len=512)
    assert cache.kv_data.dtype is torch.uint8 and cache.kv_data.size(-1) == 128 and cache.kv_param.dtype is torch.float16
    rng = np.random.default_rng(88)
    first = [70, 5, 47]
    cache.extend(first)
    cache.append(0, tb(rows(rng, (sum(first), Hkv, 128)), dev), tb(rows(rng, (sum(first), Hkv, 128)), dev))
    bound = 512
    sk, sv, sq = (tb(rows(rng, (B * n, h, 128)), dev) for h in (Hkv, Hkv, Hq))
    run = (lambda: cache.attend(0, sq, max_seq_len=bound)) if mode == "attend" else (lambda: cache.attend_new(0, sq, max_seq_len=bound))
    cache.extend(n)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cache.append(0, sk, sv)
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cache.append(0, sk, sv)
        out = run()
    released = []
    for step in range(8):
        if step:
            cache.extend(n)
        released.append(sum(p.count(-1) for p in cache._pages))
        for t in (sk, sv, sq):
            t.copy_(tb(rows(rng, tuple(t.shape)), dev))
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        eager = run()
        torch.cuda.synchronize()
        same_bits(got, eager, f"replay {step} differs from eager")
        hd = fo.dequantize(cache.kv_data.cpu().numpy(), cache.kv_param.cpu().numpy())
        tbl = [t.cpu().numpy() for t in (cache.kv_indptr, cache.kv_indices, cache.last_page_len)]
        if mode == "attend":
            t_dec.check_attention(got, kwo.decode_attention(bits(sq), hd, None, *tbl, 0, W), float(np.abs(ko.bf16_to_f32(hd[:, 0, 1])).max()))
        else:
            qo = cache.append_indptr.cpu().numpy()
            t_pre.check(got, kwo.prefill_attention(bits(sq), hd, None, *tbl, qo, 0, W),
                        kwo.prefill_vmax(tuple(sq.shape), hd, None, *tbl, qo, 0, W), f"replay {step}")
    assert released[-1] > released[0], "the replays must cross a page release"


# ---- 7. the end of the allocation ------------------------------------------------------------------------------------------------------
def test_last_row_ends_at_the_end_of_its_allocation(dev):
    """kv_data and kv_param each copied to the END of a hipMalloc allocation of whole 2 MiB pages (tests/rope_bounds_probe.py): the
    appended token goes to the last slot of the last page, so the last rows of K and V of the last layer's last head are written and
    then read by decode and prefill.  The same bytes as with both in the middle of torch's pool."""
    lib = _lib.load()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    PAGE = 2 << 20
    Hq, Hkv, P, max_pages, n_tok = 8, 2, 16, 3, 2 * 16
    rng = np.random.default_rng(90)
    k, v, q = (tb(rows(rng, (n_tok, h, 128)), dev) for h in (Hkv, Hkv, Hq))
    tbl = [i32(a, dev) for a in ([0, 2], [0, max_pages - 1], [P])]
    app = i32([0, n_tok], dev)
    data, param = empty(max_pages, Hkv, P, dev, poison=False)
    mixedgemm.kv_append(data, param, *tbl, k, v, app, L - 1)
    want_dec = mixedgemm.paged_decode(q[-1:].contiguous(), data, param, *tbl, L - 1, n_tok)
    want_pre = mixedgemm.paged_prefill(q, data, param, *tbl, app, L - 1, n_tok)
    torch.cuda.synchronize()
    assert data[max_pages - 1, L - 1, 1, Hkv - 1, P - 1].any(), "the cache's last row must be written"
    allocs, ends = [], {}
    try:
        for name, t in (("data", data), ("param", param)):
            nbytes = t.numel() * t.element_size()
            size = (nbytes + PAGE - 1) // PAGE * PAGE
            p = ctypes.c_void_p()
            assert hip.hipMalloc(ctypes.byref(p), size) == 0
            allocs.append(p)
            ends[name] = p.value + size - nbytes
            z = torch.zeros_like(t)
            assert hip.hipMemcpy(ends[name], z.data_ptr(), nbytes, 3) == 0           # device to device
        st = torch.cuda.current_stream().cuda_stream
        geo = (3, max_pages, L, L - 1, Hkv, P, 128, *(t.data_ptr() for t in tbl), 1)
        assert lib.mm_kv_append(ends["data"], ends["param"], *geo, k.data_ptr(), v.data_ptr(), app.data_ptr(), n_tok, st) == 0
        o_dec, o_pre = torch.zeros_like(want_dec), torch.zeros_like(want_pre)
        q1 = q[-1:].contiguous()
        assert lib.mm_paged_decode(q1.data_ptr(), ends["data"], ends["param"], *geo, Hq, n_tok, 0.0, None, 0, o_dec.data_ptr(), st) == 0
        assert lib.mm_paged_prefill(q.data_ptr(), app.data_ptr(), n_tok, ends["data"], ends["param"], *geo, Hq, n_tok, 0.0, None, 0,
                                    o_pre.data_ptr(), st) == 0
        torch.cuda.synchronize()
        d2, p2 = torch.zeros_like(data), torch.zeros_like(param)
        for name, t in (("data", d2), ("param", p2)):
            assert hip.hipMemcpy(t.data_ptr(), ends[name], t.numel() * t.element_size(), 3) == 0
        torch.cuda.synchronize()
        assert torch.equal(d2, data) and torch.equal(p2.view(torch.int16), param.view(torch.int16))
        same_bits(o_dec, want_dec, "decode at the end of the allocation")
        same_bits(o_pre, want_pre, "prefill at the end of the allocation")
    finally:
        torch.cuda.synchronize()
        for p in allocs:
            hip.hipFree(p)
