"""CPU tests of sliding-window attention over the paged KV cache: the fp64 window oracle against the un-windowed oracles, the host side
of the four windowed entry points (workspace sizes, statuses), PagedKVCache's page release, and the preconditions of the exact families
tests/test_kv_window_gpu.py runs (tests/kv_window_cases.py).  No kernel is launched here."""
import inspect

import numpy as np
import pytest

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_exact_cases as kc
import kv_oracle as ko
import kv_prefill_oracle as kpo
import kv_window_cases as wc
import kv_window_oracle as kwo
from test_kv_exact_cpu import host_cache

KINDS = ["int4", "bf16"]
BIG = 1 << 30


def gauss(shape, rng, scale):
    return kc.to_bf16(rng.standard_normal(shape).astype(np.float32) * scale)


def gaussian_cache(kind, lens, Hkv, P, seed):
    rng = np.random.default_rng(seed)
    c = dict(K=gauss((sum(lens), Hkv, 128), rng, 1.0), V=gauss((sum(lens), Hkv, 128), rng, 0.5), lens=list(lens), P=P, Hkv=Hkv)
    return host_cache(kind, c), rng


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_with_a_window_that_covers_everything_is_the_unwindowed_oracle(kind):
    lens, new = [40, 0, 17, 1, 100], [7, 0, 17, 1, 33]
    (data, param, tbl), rng = gaussian_cache(kind, lens, 2, 16, 1)
    qd = kc.bf16_bits(gauss((len(lens), 8, 128), rng, 2.0))
    want = ko.attention(qd, data, param, *tbl, 1)
    for W in (100, 101, BIG, None, 0):
        assert np.array_equal(kwo.decode_attention(qd, data, param, *tbl, 1, W), want), W
    qo = kc.indptr_of(new)
    qp = kc.bf16_bits(gauss((sum(new), 8, 128), rng, 2.0))
    want = kpo.attention(qp, data, param, *tbl, qo, 1)
    vm = kpo.vmax(qp.shape, data, param, *tbl, qo, 1)
    for W in (100, BIG, None, 0):
        assert np.array_equal(kwo.prefill_attention(qp, data, param, *tbl, qo, 1, W), want), W
        assert np.array_equal(kwo.prefill_vmax(qp.shape, data, param, *tbl, qo, 1, W), vm), W


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_window_is_attention_over_the_last_w_tokens(kind):
    """the window oracle over a long sequence equals the un-windowed oracle over a cache that holds only the window's tokens, and a
    released (-1) entry below the window changes nothing"""
    L, W, Hkv, P = 75, 20, 2, 16
    (data, param, tbl), rng = gaussian_cache(kind, [L], Hkv, P, 2)
    q = kc.bf16_bits(gauss((1, 4, 128), rng, 2.0))
    K, V = ko.dequantized(data, param, *tbl, 1, 0)
    s = np.einsum("hd,htd->ht", ko.bf16_to_f32(q[0]).astype(np.float64), np.repeat(K[:, L - W:], 2, 0)) / np.sqrt(128)
    p = np.exp(s - s.max(-1, keepdims=True))
    want = np.einsum("ht,htd->hd", p / p.sum(-1, keepdims=True), np.repeat(V[:, L - W:], 2, 0))
    got = kwo.decode_attention(q, data, param, *tbl, 1, W)
    assert np.abs(got[0] - want).max() < 1e-13
    assert np.abs(got - ko.attention(q, data, param, *tbl, 1)).max() > 1e-3, "the window must matter"
    # prefill with one query per position is decode at that length
    n = 30
    qs = kc.bf16_bits(gauss((n, 4, 128), rng, 2.0))
    pre = kwo.prefill_attention(qs, data, param, *tbl, np.array([0, n]), 1, W)
    for j in (0, 1, n - 1):
        tbl_j = kc.prefix_table(tbl[1], P, [L - n + j + 1])
        assert np.abs(pre[j] - kwo.decode_attention(qs[j:j + 1], data, param, *tbl_j, 1, W)[0]).max() < 1e-13
    released = wc.released_entries(tbl[0], [L], [n], P, W)
    assert released == [0]                                           # positions 0 .. 15 lie below 75 - 30 - 20 + 1 = 26
    idx = tbl[1].copy()
    idx[released] = -1
    assert np.array_equal(kwo.prefill_attention(qs, data, param, tbl[0], idx, tbl[2], np.array([0, n]), 1, W), pre)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_window_entries_are_exported_and_the_version_stays():
    lib = _lib.load()
    header = open(inspect.getsourcefile(_lib).replace("micromix_amd/_lib.py", "include/micromix_hip.h")).read()
    for name in ("mm_paged_decode_window", "mm_paged_prefill_window", "mm_paged_decode_window_workspace_bytes",
                 "mm_paged_prefill_window_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"{name}(" in header
    assert lib.mm_version() == 660
    for fn in (mixedgemm.paged_decode, mixedgemm.paged_prefill):
        assert inspect.signature(fn).parameters["window"].kind is inspect.Parameter.KEYWORD_ONLY
        assert inspect.signature(fn).parameters["window"].default is None
    for fn in (mixedgemm.paged_decode_workspace_bytes, mixedgemm.paged_prefill_workspace_bytes):
        assert list(inspect.signature(fn).parameters)[-1] == "window" and inspect.signature(fn).parameters["window"].default is None


BOUNDS = sorted({1, 2, 31, 32, 33, 255, 256, 257, 1000, 4095, 4096, 4097, 32767, 32768} | {2 ** i for i in range(16)} | {3 * 2 ** i for i in range(13)})


def test_workspace_bytes_without_a_window_or_with_one_that_covers_the_bound():
    lib = _lib.load()
    assert BOUNDS[0] == 1 and BOUNDS[-1] == 32768
    for B in (1, 8, 64):
        for Hkv in (1, 8):
            for msl in BOUNDS:
                for Hq in (Hkv, 4 * Hkv):
                    d = lib.mm_paged_decode_workspace_bytes(B, Hq, Hkv, msl)
                    for W in (0, msl, msl + 1, 2 * msl, 2 ** 31 - 1):
                        assert lib.mm_paged_decode_window_workspace_bytes(B, Hq, Hkv, msl, W) == d, (B, Hq, Hkv, msl, W)
                    assert mixedgemm.paged_decode_workspace_bytes(B, Hq, Hkv, msl, window=None) == d
                    assert mixedgemm.paged_decode_workspace_bytes(B, Hq, Hkv, msl, window=msl) == d
                    for T in (B, 5 * B + 3):
                        p = lib.mm_paged_prefill_workspace_bytes(T, B, Hq, Hkv, msl)
                        for W in (0, msl, msl + 1, 2 ** 31 - 1):
                            assert lib.mm_paged_prefill_window_workspace_bytes(T, B, Hq, Hkv, msl, W) == p, (T, B, Hq, Hkv, msl, W)
                        assert mixedgemm.paged_prefill_workspace_bytes(T, B, Hq, Hkv, msl, 0) == p


def test_the_split_is_laid_over_the_window():
    """a 4096-token window under a 32768-token bound takes the workspace of an un-windowed call bounded by the window's span: W tokens
    in decode (the range starts at the window), W + 64 / g + 62 in prefill (a 64-token tile and the query tile's rows)"""
    lib = _lib.load()
    for B, Hq, Hkv in ((1, 32, 8), (8, 32, 8), (1, 1, 1), (3, 16, 1)):
        for W in (1, 300, 1024, 4096):
            for msl in (W, W + 1, 32768, 1 << 20):
                assert lib.mm_paged_decode_window_workspace_bytes(B, Hq, Hkv, msl, W) == lib.mm_paged_decode_workspace_bytes(B, Hq, Hkv, W)
            bq = 64 // (Hq // Hkv)
            for msl in (W + bq + 62, 32768):
                assert lib.mm_paged_prefill_window_workspace_bytes(512, B, Hq, Hkv, msl, W) == \
                    lib.mm_paged_prefill_workspace_bytes(512, B, Hq, Hkv, W + bq + 62)
    assert lib.mm_paged_decode_window_workspace_bytes(1, 1, 1, 5000, 1024) > 0, "W = 1024 with B * Hkv = 1 must split (the GPU tests rely on it)"
    assert lib.mm_paged_decode_window_workspace_bytes(1, 32, 8, 32768, 4096) < lib.mm_paged_decode_workspace_bytes(1, 32, 8, 32768)


def decode_args(window, q=1, data=1, B=2, Hq=8, Hkv=2, msl=100, ws=None, ws_bytes=0, o=1, L=1, layer=0, P=16, hd=128, tbl=(1, 1, 1), kind=0):
    return (q, data, 1, kind, 4, L, layer, Hkv, P, hd, *tbl, B, Hq, msl, 0.0, ws, ws_bytes, o, None, window)


def prefill_args(window, q=1, qo=1, T=4, data=1, B=2, Hq=8, Hkv=2, msl=100, ws=None, ws_bytes=0, o=1, hd=128, tbl=(1, 1, 1)):
    return (q, qo, T, data, 1, 0, 4, 1, 0, Hkv, 16, hd, *tbl, B, Hq, msl, 0.0, ws, ws_bytes, o, None, window)


def test_statuses_without_a_device():
    """every row returns before a launch: the addresses are fakes (1) or null"""
    lib = _lib.load()
    OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED
    dec, pre = lib.mm_paged_decode_window, lib.mm_paged_prefill_window
    for W in (-1, -4096, -2 ** 31):
        assert dec(*decode_args(W)) == BAD and pre(*prefill_args(W)) == BAD
        assert dec(*decode_args(W, B=0)) == BAD and pre(*prefill_args(W, T=0)) == BAD          # before "nothing to do"
        assert lib.mm_paged_decode_window_workspace_bytes(1, 8, 2, 100000, W) == 0
        assert lib.mm_paged_prefill_window_workspace_bytes(4, 1, 8, 2, 100000, W) == 0
    for W in (0, 1, 4096):
        assert dec(*decode_args(W, B=0, q=None, data=None, o=None, tbl=(None,) * 3)) == OK      # empty work, no pointer looked at
        assert pre(*prefill_args(W, T=0, q=None, qo=None, data=None, o=None, tbl=(None,) * 3)) == OK
        assert pre(*prefill_args(W, B=0, q=None, qo=None, data=None, o=None, tbl=(None,) * 3)) == OK
        for kw in ({"q": None}, {"data": None}, {"o": None}, {"tbl": (None, 1, 1)}, {"tbl": (1, None, 1)}, {"tbl": (1, 1, None)},
                   {"msl": -1}, {"Hq": 0}, {"Hq": 7}, {"Hkv": 0}, {"B": -1}):
            assert dec(*decode_args(W, **kw)) == BAD, kw
            assert pre(*prefill_args(W, **kw)) == BAD, kw
        assert pre(*prefill_args(W, qo=None)) == BAD and pre(*prefill_args(W, T=-1)) == BAD
        assert dec(*decode_args(W, Hq=34, Hkv=2)) == UNS and pre(*prefill_args(W, Hq=34, Hkv=2)) == UNS      # g = 17
        assert dec(*decode_args(W, hd=64)) == UNS and pre(*prefill_args(W, hd=64)) == UNS
        assert dec(*decode_args(W, P=0)) == BAD and dec(*decode_args(W, layer=1)) == BAD
    # a split launch without its workspace: null, too small, misaligned
    need = lib.mm_paged_decode_window_workspace_bytes(1, 8, 2, 100000, 4096)
    assert need > 0
    for ws, nb in ((None, 0), (0x10000, need - 1), (0x10008, need)):
        assert dec(*decode_args(4096, B=1, msl=100000, ws=ws, ws_bytes=nb)) == BAD
    need = lib.mm_paged_prefill_window_workspace_bytes(4, 1, 8, 2, 100000, 4096)
    assert need > 0
    for ws, nb in ((None, 0), (0x10000, need - 1), (0x10008, need)):
        assert pre(*prefill_args(4096, B=1, msl=100000, ws=ws, ws_bytes=nb)) == BAD
    # the Python layer refuses a negative window before it looks at a tensor
    for fn in (mixedgemm.paged_decode_workspace_bytes, ):
        with pytest.raises(ValueError):
            fn(1, 8, 2, 100, window=-1)
    with pytest.raises(ValueError):
        mixedgemm.paged_decode(None, None, None, None, None, None, 0, 10, window=-1)
    with pytest.raises(ValueError):
        mixedgemm.paged_prefill(None, None, None, None, None, None, None, 0, 10, window=-3)
    with pytest.raises(ValueError):
        PagedKVCache(1, 1, 16, 4, 1, device="cpu", window=-1)


# ---- PagedKVCache bookkeeping --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P, W", [(16, 40), (1, 7), (24, 100), (16, 1), (16, 16)])
def test_cache_releases_exactly_the_pages_below_the_window(P, W):
    B, rng = 4, np.random.default_rng(P * 1000 + W)
    most = 30
    per_seq = -(-(W + most) // P) + 1
    max_pages = B * per_seq + 2
    cache = PagedKVCache(1, 1, P, max_pages, B, kind="bf16", device="cpu", window=W)
    keep = PagedKVCache(1, 1, P, B * (300 * most // P + 2), B, kind="bf16", device="cpu", window=W, release=False)
    assert cache.window == W and cache.release and not keep.release
    lens, handed_back = [0] * B, 0
    for step in range(300):
        if step % 3 == 0:
            new = [1] * B
        elif step % 3 == 1:
            new = [int(n) for n in rng.integers(0, most + 1, B)]
        else:
            new = [0, 1, 0, int(rng.integers(1, most + 1))]
        if step in (120, 200):                                   # a sequence ends: every page it still holds comes back, once
            held = [p for p in cache._pages[1] if p >= 0]
            free_before = len(cache._free)
            cache.reset(1)
            keep.reset(1)
            assert len(cache._free) == free_before + len(held) and -1 not in cache._free
            lens[1] = 0
        cache.extend(new)
        keep.extend(new)
        lens = [a + n for a, n in zip(lens, new)]
        assert cache.seq_lens == lens == keep.seq_lens
        indptr, indices, last = (t.numpy() for t in (cache.kv_indptr, cache.kv_indices, cache.last_page_len))
        assert np.array_equal(ko.seq_lens(indptr, last, P), lens), "a released entry keeps its place: the lengths do not move"
        owned = []
        for b in range(B):
            ent = indices[indptr[b]:indptr[b + 1]]
            assert len(ent) == -(-lens[b] // P)
            bound = lens[b] - max(new[b], 1) - W + 1              # the lowest position the announced tokens attend
            below = [i for i in range(len(ent)) if (i + 1) * P <= bound]
            # (n_b = 0: what a decode query at the last position attends.)  The bound never moves down, so the released entries are
            # exactly the pages wholly below this step's
            assert [i for i in range(len(ent)) if ent[i] < 0] == below and (ent[below] == -1).all()
            held = ent[ent >= 0]
            assert len(held) <= -(-(W + new[b]) // P) + 1, "pages held beyond ceil((W + n_b) / P) + 1"
            owned += held.tolist()
            k_ent = keep.kv_indices.numpy()[keep.kv_indptr.numpy()[b]:keep.kv_indptr.numpy()[b + 1]]
            assert (k_ent >= 0).all() and len(k_ent) == len(ent)
        assert len(owned) == len(set(owned)), "a page is owned twice"
        assert not set(owned) & set(cache._free) and len(set(cache._free)) == len(cache._free)
        assert sorted(owned + cache._free) == list(range(max_pages)), "a page was lost"
        assert len(cache._free) >= max_pages - B * per_seq
    for b in range(B):
        cache.reset(b)
    assert sorted(cache._free) == list(range(max_pages)), "reset returns each page once"


def test_cache_without_a_window_releases_nothing():
    cache = PagedKVCache(1, 1, 16, 64, 2, kind="bf16", device="cpu")
    assert cache.window == 0 and not cache.release
    for _ in range(20):
        cache.extend([17, 30])
    assert (cache.kv_indices.numpy()[: int(cache.kv_indptr[-1])] >= 0).all() and len(cache._free) == 64 - 22 - 38
    with pytest.raises(RuntimeError, match="out of pages"):
        cache.extend(16 * 64)
    # a windowed cache goes on for ever in the same pool
    w = PagedKVCache(1, 1, 16, 16, 2, kind="bf16", device="cpu", window=32)
    for _ in range(500):
        w.extend([17, 30])
    assert w.seq_lens == [8500, 15000]


# ---- preconditions of the exact families -----------------------------------------------------------------------------------------
def test_count_expectation_is_the_mean_over_the_window():
    for W in wc.WINDOWS:
        for p in (0, 1, W - 1, W, W + 1, W + 127, W + 128, 3 * W + 300):
            lo = max(0, p - W + 1)
            want = kc.count_v(np.arange(lo, p + 1)).astype(np.float64).mean(0)
            assert np.abs(wc.count_window_expect(p, W) - want).max() <= 1e-15, (W, p)
    assert np.array_equal(wc.count_window_expect(np.arange(500), BIG), kc.count_expect(np.arange(500)))
    # one lost or one extra token is 8 ulps or more away for every W the tests use (29 at W = 1024; at W = 4096 it would be 7.4,
    # 1.875 / 4096 against an ulp of 2^-14: the margin DESIGN 7b argues from, which no window here comes near)
    assert max(wc.WINDOWS) <= 1024
    for W in wc.WINDOWS:
        p = W + 300
        want = wc.count_window_expect(p, W)
        ulp = kc.bf16_ulp(want)
        lost = kc.count_v(np.arange(p - W + 2, p + 1)).astype(np.float64).mean(0) if W > 1 else np.zeros(128)
        extra = kc.count_v(np.arange(p - W, p + 1)).astype(np.float64).mean(0)
        for other in (lost, extra):
            d = np.abs(other - want)
            assert (d / np.maximum(ulp, 2.0 ** -140)).max() >= 8, W          # in the dimension of that token


@pytest.mark.parametrize("P", wc.PAGE_SIZES)
def test_count_cases_put_the_window_start_on_both_sides_of_every_edge(P):
    starts = set(wc.window_starts(P))
    for step in (32, 64, 256) + ((P,) if P > 1 else ()):
        for m in range(step, wc.EDGE_MAX + 1, step):
            assert m in starts and m - 1 in starts, (step, m)
    for W in wc.WINDOWS:
        lens = wc.count_decode_lengths(W, P)
        assert {n - W for n in lens if n > W} >= starts - {0} and W in lens and min(lens) <= max(W - 1, 1)
        c = wc.count_prefill(5, 1, P, W)
        bq = 12
        assert c["new"][:5] == [1, bq - 1, bq, bq + 1, 3 * bq + 1]
        first = wc.window_begin(c["pos"], W)
        assert {31, 63, 64, 255, 256, 257} <= set(first.tolist()) and (np.array(c["lens"]) <= W).any() and (np.array(c["lens"]) > W).any()
    # the chunks of the split the library picks for W = 1024 at B * Hkv = 1 are 256 tokens long: 256 and 512 are chunk edges
    lib = _lib.load()
    assert lib.mm_paged_decode_window_workspace_bytes(1, 1, 1, 1024 + wc.EDGE_MAX, 1024) == 4 * (128 + 2) * 4


@pytest.mark.parametrize("kind", KINDS)
def test_count_oracle_returns_the_window_mean(kind):
    c = wc.count_prefill(4, 1, 16, 33)
    data, param, tbl = host_cache(kind, c)
    got = kwo.prefill_attention(kc.bf16_bits(c["q"]), data, param, *tbl, kc.indptr_of(c["new"]), 1, 33)
    assert np.abs(got - c["expect"]).max() <= 1e-13
    d = wc.count_decode(4, 1, 24, 65, lengths=[1, 64, 65, 66, 200])
    data, param, _ = host_cache(kind, d, [d["N"]])
    tbl = kc.prefix_table(kc.page_table([d["N"]], 24, 0)[1], 24, d["lens"])
    got = kwo.decode_attention(kc.bf16_bits(d["q"]), data, param, *tbl, 1, 65)
    assert np.abs(got - d["expect"]).max() <= 1e-13


def test_twin_margin_and_exactness():
    """40 nats between the needle and every other token a window can hold, the plants' mean is a bf16 value, and every family asks
    both questions: a plant at p - W (outside) with one inside, and a plant at p - W + 1 (the first inside) with another inside"""
    longest = 0
    for decode in (True, False):
        for W in wc.TWIN_WINDOWS:
            c = wc.twin(8, 2, 16, W, decode)
            longest = max(longest, c["N"] + 1)
            assert np.array_equal(kc.to_bf16(c["expect"].astype(np.float32)).astype(np.float64), c["expect"]), "the mean is not a bf16 value"
            assert np.array_equal(c["expect"] * 16, np.round(c["expect"] * 16))
            seen = c["plants_seen"]
            assert (seen == 1).any() and ((seen == 2).any() or W == 1)
            outside = inside_first = False
            pos = np.concatenate([a + np.arange(n) for a, n in zip(c["prior"], c["new"])])
            shape = wc.twin_shape(c["g"], W, decode)
            plants = np.concatenate([np.tile(np.array(s[2])[None], (s[1], 1)) for s in shape])
            for p, (a, b), k in zip(pos, plants, seen):
                outside |= bool(a == p - W and k == 1)
                inside_first |= bool(a == p - W + 1 and k == 2 and a != b)
            assert outside and (inside_first or W == 1), (W, decode)
    assert longest <= 4608
    for h in range(2):
        assert kc.worst_correlation(h, longest) <= 71                 # (128 - 71) * 8 * 0.9997 / sqrt(128) = 40.3 nats
    assert kc.needle_margin_nats(2, longest) >= kc.MARGIN_NATS and np.exp(-kc.MARGIN_NATS) * longest < 2.0 ** -40


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("decode", [True, False])
def test_twin_oracle_returns_the_plants(kind, decode):
    for W in (1, 33, 300):
        c = wc.twin(4, 1, 24, W, decode)
        data, param, tbl = host_cache(kind, c)
        q = kc.bf16_bits(c["q"])
        if decode:
            got = kwo.decode_attention(q, data, param, *tbl, 1, W)
        else:
            got = kwo.prefill_attention(q, data, param, *tbl, kc.indptr_of(c["new"]), 1, W)
        bad = np.abs(got - c["expect"]) > np.where(np.isfinite(wc.twin_bound(c)), 1e-12, np.inf)
        assert not bad.any(), (W, np.argwhere(bad)[:3])
