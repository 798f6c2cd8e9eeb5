"""GPU tests of sliding-window attention over the paged KV cache (mixedgemm.paged_decode / paged_prefill with window=W,
PagedKVCache(window=W)); the preconditions of the exact families are proved on the CPU in tests/test_kv_window_cpu.py.

1 count     zero queries: the exact mean over the window, within 1 bf16 ulp of the fp64 value (one lost or extra token is >= 8 ulps)
2 twin      the needle planted twice: a plant at p - W is not seen (2^-20), a plant at p - W + 1 is (the exact mean of two rows, 1 ulp)
3 gaussian  against the fp64 window oracle with the bounds of test_kvcache_gpu.py / test_kvprefill_gpu.py
4 bits      no window, or one that covers max_seq_len: bit-equal to the un-windowed call; two launches; n_b = 1 against decode
5 released  table entries below the window set to -1 and their pages overwritten with NaN: bit-equal; PagedKVCache against release=False
6 capture   one hipGraph of append + attend / attend_new replayed across extend steps that release pages

No bound here comes from what a kernel produced."""
import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_exact_cases as kc
import kv_oracle as ko
import kv_window_cases as wc
import kv_window_oracle as kwo
import test_kv_exact_gpu as ex
import test_kvcache_gpu as t_dec
import test_kvprefill_gpu as t_pre

pytestmark = pytest.mark.gpu

KINDS = ["int4", "bf16"]
LAYER = ex.LAYER
SHAPES = [(hq, hkv, P) for hq, hkv in wc.HEADS for P in wc.PAGE_SIZES]
IDS = [f"{hq}x{hkv}-P{P}" for hq, hkv, P in SHAPES]


def decode(cache, q, tbl, msl, W, **kw):
    return mixedgemm.paged_decode(q, cache["data"], cache["param"], *tbl, LAYER, msl, window=W, **kw)


def prefill(cache, q, new, msl, W, tbl=None, **kw):
    return mixedgemm.paged_prefill(q, cache["data"], cache["param"], *(cache["tbl"] if tbl is None else tbl),
                                   ex.i32(kc.indptr_of(new), q.device), LAYER, msl, window=W, **kw)


def same_bits(a, b, what):
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), what


# ---- 1. count --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_count_decode(dev, kind, shape):
    """every window, the window start on both sides of every multiple of 32 / 64 / 256 and page edge, a tight and a loose bound"""
    Hq, Hkv, P = shape
    N = max(wc.WINDOWS) + wc.EDGE_MAX
    cache = ex.fill(kind, np.repeat(kc.ramp_k(np.arange(N))[:, None], Hkv, 1), np.repeat(kc.count_v(np.arange(N))[:, None], Hkv, 1), [N], P, dev)
    for W in wc.WINDOWS:
        c = wc.count_decode(Hq, Hkv, P, W)
        q, lens = ex.bf(c["q"], dev), c["lens"]
        tbl = [ex.i32(a, dev) for a in kc.prefix_table(cache["pages"], P, lens)]
        lab = lambda i: f"W={W} length {lens[i // Hq]} head {i % Hq}"
        ulp = kc.bf16_ulp(c["expect"]).reshape(-1, 128)
        for msl in (max(lens), max(lens) + 5000):
            ex.expect_rows(decode(cache, q, tbl, msl, W), c["expect"], lab, ulp, f"{kind} {shape} W={W} bound {msl}", grid=False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Hq, g", [(1, 1), (4, 4), (5, 5), (16, 16)])
def test_count_decode_split(dev, kind, Hq, g):
    """B * Hkv = 1 and W = 1024 (300): four (two) chunks of 256 tokens laid over the window, the window start on and beside every
    multiple of 256; also past the bound the split was planned for"""
    P, N = 16, 1024 + wc.EDGE_MAX + 300
    cache = ex.fill(kind, kc.ramp_k(np.arange(N))[:, None], kc.count_v(np.arange(N))[:, None], [N], P, dev)
    for W, nc in ((1024, 4), (300, 2)):
        msl = W + wc.EDGE_MAX
        assert mixedgemm.paged_decode_workspace_bytes(1, Hq, 1, msl, window=W) == nc * Hq * (128 + 2) * 4
        for e in (0, 1, 31, 32, 33, 255, 256, 257, 300, 511, 512, 513, wc.EDGE_MAX, wc.EDGE_MAX + 299):
            c = wc.count_decode(Hq, 1, P, W, lengths=[W + e])
            tbl = [ex.i32(a, dev) for a in kc.prefix_table(cache["pages"], P, c["lens"])]
            o = decode(cache, ex.bf(c["q"], dev), tbl, msl, W)
            ex.expect_rows(o, c["expect"], lambda i: f"W={W} length {W + e} head {i}", kc.bf16_ulp(c["expect"]).reshape(-1, 128),
                           f"{kind} g={g} W={W} window start {e}", grid=False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES[1::2] + SHAPES[:1], ids=IDS[1::2] + IDS[:1])
def test_count_prefill(dev, kind, shape):
    """n_b in {1, BQ - 1, BQ, BQ + 1, several tiles, 70}: the lower edge of consecutive rows crosses tile, page and chunk edges"""
    Hq, Hkv, P = shape
    for W in wc.WINDOWS:
        c = wc.count_prefill(Hq, Hkv, P, W)
        cache = ex.fill(kind, c["K"], c["V"], c["lens"], P, dev)
        q = ex.bf(c["q"], dev)
        ulp = kc.bf16_ulp(c["expect"]).reshape(-1, 128)
        for msl in (max(c["lens"]), max(c["lens"]) + 5000):
            ex.expect_rows(prefill(cache, q, c["new"], msl, W), c["expect"], ex.prefill_labels(c), ulp, f"{kind} {shape} W={W} bound {msl}",
                           grid=False)
    assert mixedgemm.paged_prefill_workspace_bytes(sum(c["new"]), len(c["new"]), Hq, Hkv, max(c["lens"]), window=1024) > 0, "W = 1024 must split"


# ---- 2. twin needle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["decode", "prefill"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[5], SHAPES[6], SHAPES[10], SHAPES[14]], ids=[IDS[i] for i in (1, 5, 6, 10, 14)])
def test_twin_needle(dev, kind, mode, shape):
    Hq, Hkv, P = shape
    for W in wc.TWIN_WINDOWS:
        c = wc.twin(Hq, Hkv, P, W, mode == "decode")
        cache = ex.fill(kind, c["K"], c["V"], c["lens"], P, dev)
        q, msl = ex.bf(c["q"], dev), max(c["lens"])
        o = decode(cache, q, cache["tbl"], msl, W) if mode == "decode" else prefill(cache, q, c["new"], msl, W)
        bound = np.broadcast_to(wc.twin_bound(c), c["expect"].shape).reshape(-1, 128)
        ex.expect_rows(o, c["expect"], ex.prefill_labels(c), bound, f"{kind} {mode} {shape} W={W}")
        assert torch.isfinite(o.float()).all()


# ---- 3. gaussian data against the fp64 window oracle -------------------------------------------------------------------------------
def gaussian(kind, lens, Hkv, P, dev, seed, poison=False):
    rng = np.random.default_rng(seed)
    K, V = ex.gauss((sum(lens), Hkv, 128), rng, 1.0), ex.gauss((sum(lens), Hkv, 128), rng, 0.5)
    return ex.fill(kind, K, V, lens, P, dev, poison, seed=seed), rng, float(np.abs(V).max())


GAUSS_DECODE = [(8, 2, 16, [0, 1, 99, 100, 101, 700, 33], 100), (5, 1, 24, [300, 64, 65, 2000], 64), (16, 1, 1, [40, 17, 0], 33),
                (1, 1, 16, [3000], 1024), (4, 1, 16, [1, 5, 130], 1)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", range(len(GAUSS_DECODE)))
def test_gaussian_decode(dev, kind, case):
    Hq, Hkv, P, lens, W = GAUSS_DECODE[case]
    cache, rng, vmax = gaussian(kind, lens, Hkv, P, dev, 900 + case)
    q = ex.bf(ex.gauss((len(lens), Hq, 128), rng, 2.0), dev)
    o = decode(cache, q, cache["tbl"], max(lens), W)
    o2 = decode(cache, q, cache["tbl"], max(lens), W)
    o_loose = decode(cache, q, cache["tbl"], max(lens) + 5000, W)
    torch.cuda.synchronize()
    same_bits(o, o2, "two launches differ")
    hd, hp = t_dec.host(cache["data"], cache["param"])
    want = kwo.decode_attention(t_dec.bits(q), hd, hp, *cache["tbl_h"], LAYER, W)
    if max(lens) > W + 50:
        assert np.abs(want - ko.attention(t_dec.bits(q), hd, hp, *cache["tbl_h"], LAYER)).max() > 1e-2, "the window must matter"
    for b, n in enumerate(lens):
        if n == 0:
            assert int(torch.count_nonzero(o[b].float())) == 0
    t_dec.check_attention(o, want, vmax)
    t_dec.check_attention(o_loose, want, vmax)


# (Hq, Hkv, P, prior, new, W): ragged, n_b = 0, lengths shorter than, equal to and longer than the window
GAUSS_PREFILL = [(8, 2, 16, [0, 90, 5, 400, 100], [100, 10, 0, 70, 1], 100), (5, 1, 24, [100, 0, 1000], [65, 64, 13], 64),
                 (16, 1, 1, [3, 200], [17, 9], 33), (4, 1, 16, [2500], [130], 1024), (1, 1, 16, [10, 0], [70, 3], 1)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", range(len(GAUSS_PREFILL)))
def test_gaussian_prefill(dev, kind, case):
    Hq, Hkv, P, prior, new, W = GAUSS_PREFILL[case]
    lens = [a + n for a, n in zip(prior, new)]
    cache, rng, _ = gaussian(kind, lens, Hkv, P, dev, 950 + case)
    q = ex.bf(ex.gauss((sum(new), Hq, 128), rng, 2.0), dev)
    o = prefill(cache, q, new, max(lens), W)
    o2 = prefill(cache, q, new, max(lens), W)
    o_loose = prefill(cache, q, new, max(lens) + 5000, W)
    torch.cuda.synchronize()
    same_bits(o, o2, "two launches differ")
    hd, hp = t_pre.host(cache["data"], cache["param"])
    qo = kc.indptr_of(new)
    want = kwo.prefill_attention(t_pre.bits(q), hd, hp, *cache["tbl_h"], qo, LAYER, W)
    vm = kwo.prefill_vmax(tuple(q.shape), hd, hp, *cache["tbl_h"], qo, LAYER, W)
    t_pre.check(o, want, vm, "tight bound")
    t_pre.check(o_loose, want, vm, "loose bound")


# ---- 4. bit equality -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_no_window_and_a_covering_window_are_the_unwindowed_bits(dev, kind):
    for Hq, Hkv, P, lens, msl in ((8, 2, 16, [0, 1, 100, 700, 33], 700), (16, 1, 24, [300, 31], 300), (1, 1, 16, [3000], 3000), (5, 1, 1, [64, 65], 9000)):
        cache, rng, _ = gaussian(kind, lens, Hkv, P, dev, 970 + Hq)
        q = ex.bf(ex.gauss((len(lens), Hq, 128), rng, 2.0), dev)
        base = mixedgemm.paged_decode(q, cache["data"], cache["param"], *cache["tbl"], LAYER, msl)
        for W in (None, 0, msl, msl + 1, 1 << 30, 2 ** 31 - 1):
            same_bits(decode(cache, q, cache["tbl"], msl, W), base, f"decode {kind} Hq={Hq} window {W}")
        new = [min(n, 70) for n in lens]
        qp = ex.bf(ex.gauss((sum(new), Hq, 128), rng, 2.0), dev)
        base = ex.prefill(cache, qp, new, msl)
        for W in (None, 0, msl, msl + 1, 1 << 30, 2 ** 31 - 1):
            same_bits(prefill(cache, qp, new, msl, W), base, f"prefill {kind} Hq={Hq} window {W}")


@pytest.mark.parametrize("kind", KINDS)
def test_single_token_prefill_matches_windowed_decode(dev, kind):
    """the comparison of test_kvprefill_gpu.test_single_token_matches_decode, with its bound, under a window"""
    for Hq, Hkv, lens, W in ((8, 2, [1, 17, 301, 2000], 300), (5, 1, [8, 1001], 64), (16, 1, [34, 33], 33)):
        cache, rng, _ = gaussian(kind, lens, Hkv, 16, dev, 990 + Hq)
        q = ex.bf(ex.gauss((len(lens), Hq, 128), rng, 2.0), dev)
        o = prefill(cache, q, [1] * len(lens), max(lens), W)
        d = decode(cache, q, cache["tbl"], max(lens), W)
        torch.cuda.synchronize()
        hd, hp = t_pre.host(cache["data"], cache["param"])
        qo = kc.indptr_of([1] * len(lens))
        vm = kwo.prefill_vmax(tuple(q.shape), hd, hp, *cache["tbl_h"], qo, LAYER, W)
        t_pre.check(o, kwo.prefill_attention(t_pre.bits(q), hd, hp, *cache["tbl_h"], qo, LAYER, W), vm, "prefill n_b = 1")
        t_pre.check(o, ex.f64(d), vm, "prefill against windowed decode")


# ---- 5. released pages -------------------------------------------------------------------------------------------------------------
def release(cache, lens, new, P, W):
    """a copy of the cache whose pages wholly below every window are overwritten with NaN / 0xFF and whose table entries are -1"""
    indptr, indices, last = cache["tbl_h"]
    gone = wc.released_entries(indptr, lens, new, P, W)
    assert gone, "the case must release something"
    data, param = cache["data"].clone(), None if cache["param"] is None else cache["param"].clone()
    pages = torch.from_numpy(indices[gone].astype(np.int64)).to(data.device)
    if param is None:
        data.view(torch.int16)[pages] = 0x7FC0
    else:
        data[pages] = 0xFF
        param.view(torch.int16)[pages] = 0x7E00
    idx = indices.copy()
    idx[gone] = -1
    return dict(data=data, param=param, tbl=[cache["tbl"][0], ex.i32(idx, data.device), cache["tbl"][2]])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", wc.PAGE_SIZES)
def test_released_pages_are_never_read(dev, kind, P):
    Hq, Hkv, W = 8, 2, 100
    prior, new = [0, 500, 140, 99, 1300], [90, 1, 70, 3, 1]
    lens = [a + n for a, n in zip(prior, new)]
    cache, rng, _ = gaussian(kind, lens, Hkv, P, dev, 1000 + P)
    q = ex.bf(ex.gauss((len(lens), Hq, 128), rng, 2.0), dev)
    qp = ex.bf(ex.gauss((sum(new), Hq, 128), rng, 2.0), dev)
    for msl in (max(lens), 9000):
        gone = release(cache, lens, [1] * len(lens), P, W)
        o = decode(gone, q, gone["tbl"], msl, W)
        assert torch.isfinite(o.float()).all()
        same_bits(o, decode(cache, q, cache["tbl"], msl, W), f"decode P={P} bound {msl}")
        gone = release(cache, lens, new, P, W)
        o = prefill(gone, qp, new, msl, W, tbl=gone["tbl"])
        assert torch.isfinite(o.float()).all()
        same_bits(o, prefill(cache, qp, new, msl, W), f"prefill P={P} bound {msl}")


@pytest.mark.parametrize("kind", KINDS)
def test_cache_with_release_equals_cache_without(dev, kind):
    """two caches fed the same tokens, one releasing pages into a pool so small that other sequences take them at once"""
    B, Hq, Hkv, P, W, most = 3, 8, 2, 16, 40, 20
    per_seq = -(-(W + most) // P) + 1
    a = PagedKVCache(1, Hkv, P, B * per_seq + 1, B, kind=kind, device=dev, window=W)
    b = PagedKVCache(1, Hkv, P, 256, B, kind=kind, device=dev, window=W, release=False)
    rng = np.random.default_rng(77)
    owner, reused = {}, False
    for step in range(40):
        new = [1] * B if step % 2 else [int(n) for n in rng.integers(0, most + 1, B)]
        a.extend(1 if step % 2 else new)
        b.extend(new)
        assert len(a._free) >= 1, "fewer free pages than ceil((W + n_b) / P) + 1 per sequence leaves"
        for s, pages in enumerate(a._pages):
            for p in pages:
                if p >= 0:
                    reused |= owner.setdefault(p, s) != s
                    owner[p] = s
        T = sum(new)
        k, v, q = (ex.bf(ex.gauss((T, h, 128), rng, s), dev) for h, s in ((Hkv, 1.0), (Hkv, 0.5), (Hq, 2.0)))
        for c in (a, b):
            c.append(0, k, v)
        same_bits(a.attend_new(0, q), b.attend_new(0, q), f"attend_new at step {step}")
        if step % 2:
            same_bits(a.attend(0, q), b.attend(0, q), f"attend at step {step}")
    assert min(a.seq_lens) > 3 * W and all(-1 in p for p in a._pages) and reused, "released pages must have gone to another sequence"
    torch.cuda.synchronize()
    hd, hp = t_pre.host(a.kv_data, a.kv_param)
    tbl = [t.cpu().numpy() for t in (a.kv_indptr, a.kv_indices, a.last_page_len)]
    o = a.attend(0, q)
    t_dec.check_attention(o, kwo.decode_attention(t_dec.bits(q), hd, hp, *tbl, 0, W), 4.0)


# ---- 6. capture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["attend", "attend_new"])
def test_graph_capture_across_page_releases(dev, kind, mode):
    """append + attend (attend_new with 5 tokens per sequence) captured once, replayed over extend steps that release pages"""
    B, Hq, Hkv, P, W = 3, 8, 2, 16, 40
    n = 1 if mode == "attend" else 5
    cache = PagedKVCache(1, Hkv, P, 24, B, kind=kind, device=dev, window=W, max_seq_len=512)
    rng = np.random.default_rng(88)
    first = [70, 5, 47]
    cache.extend(first)
    cache.append(0, t_dec.rand_bf16((sum(first), Hkv, 128), rng, dev), t_dec.rand_bf16((sum(first), Hkv, 128), rng, dev))
    bound = 512
    sk, sv, sq = (t_dec.rand_bf16((B * n, h, 128), rng, dev) for h in (Hkv, Hkv, Hq))
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
            t.copy_(t_dec.rand_bf16(tuple(t.shape), rng, dev))
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        eager = run()
        torch.cuda.synchronize()
        same_bits(got, eager, f"replay {step} differs from eager")
        hd, hp = t_pre.host(cache.kv_data, cache.kv_param)
        tbl = [t.cpu().numpy() for t in (cache.kv_indptr, cache.kv_indices, cache.last_page_len)]
        if mode == "attend":
            t_dec.check_attention(got, kwo.decode_attention(t_dec.bits(sq), hd, hp, *tbl, 0, W), 4.0)
        else:
            qo = cache.append_indptr.cpu().numpy()
            t_pre.check(got, kwo.prefill_attention(t_pre.bits(sq), hd, hp, *tbl, qo, 0, W),
                        kwo.prefill_vmax(tuple(sq.shape), hd, hp, *tbl, qo, 0, W), f"replay {step}")
    assert released[-1] > released[0], "the replays must cross a page release"
