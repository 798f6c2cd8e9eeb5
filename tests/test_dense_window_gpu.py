"""GPU tests of sliding-window dense attention (mixedgemm.dense_attention_window, include/micromix_attention_window.h) and of
PagedKVCache.prefill_fresh(windowed=True): a plain fp64 band-causal reference, an exact count that walks the lower edge over every tile,
wave and block alignment, isolation, the bits where the window does not bind, views and graph replay, the cache route."""
import functools

import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
from micromix_amd.kvcache import PagedKVCache
from conftest import t_from_bits as from_bits
from test_dense_attention_gpu import bits, f64, indptr_of, rand_bf16
import rope_oracle as ro

pytestmark = pytest.mark.gpu
LENS = [64, 0, 323, 1, 129, 63, 128, 65, 127]
window = mixedgemm.dense_attention_window


def reference(q, k, v, lens, W, sm_scale=128 ** -0.5):
    """fp64 band-causal GQA attention over the bf16 values (row i attends i - W + 1 .. i); also max |V| over the tokens a row attends"""
    q, k, v = f64(q), f64(k).reshape(len(q), -1, 128), f64(v).reshape(len(q), -1, 128)
    g, o, vmax, t0 = q.shape[1] // k.shape[1], np.zeros(q.shape), np.zeros(q.shape[:2] + (1,)), 0
    for n in filter(None, lens):
        i = np.arange(n)
        band = (i[None] <= i[:, None]) & (i[None] > i[:, None] - W)
        for h in range(q.shape[1]):
            s = np.where(band, q[t0:t0 + n, h] @ k[t0:t0 + n, h // g].T * sm_scale, -np.inf)
            p = np.exp(s - s.max(axis=1, keepdims=True))
            o[t0:t0 + n, h] = p @ v[t0:t0 + n, h // g] / p.sum(axis=1, keepdims=True)
            vmax[t0:t0 + n, h, 0] = np.where(band, np.abs(v[t0:t0 + n, h // g]).max(axis=1)[None], 0).max(axis=1)
        t0 += n
    return o, vmax


def assert_within_7c(o, want, vmax, what):
    """|o - ref| <= 2 bf16 ulp(ref) + 2^-8 max|V| over the attended tokens"""
    err = np.abs(f64(o) - want)
    bound = 2 * 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-30))) - 7) + 2.0 ** -8 * vmax
    print(f"{what}: worst err {err.max():.3e}, worst err / bound {(err / bound).max():.3f}")
    assert np.isfinite(f64(o)).all() and (err <= bound).all(), f"{what}: {int((err > bound).sum())} outputs outside the bound"


@functools.lru_cache(maxsize=None)
def inputs(Hq, Hkv, dev, lens=tuple(LENS)):
    rng, T = np.random.default_rng(Hq * 100 + Hkv), sum(lens)
    return rand_bf16((T, Hq, 128), rng, dev, 2.0), rand_bf16((T, Hkv, 128), rng, dev), rand_bf16((T, Hkv, 128), rng, dev, 0.5)


@pytest.mark.parametrize("W", [1, 31, 64, 65, 100, 128, 200])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2), (5, 1)])
def test_against_fp64(dev, Hq, Hkv, W):
    q, k, v = inputs(Hq, Hkv, dev)
    o = window(q, k, v, W, indptr_of(LENS, dev))
    assert_within_7c(o, *reference(q, k, v, LENS, W), f"Hq {Hq} Hkv {Hkv} W {W}")


@pytest.mark.parametrize("m", [0, 1, 64, 65, 128, 200, 323])
@pytest.mark.parametrize("W", [1, 32, 63, 64, 65, 128, 129])
def test_exact_count(dev, W, m):
    """q = 0 makes the softmax uniform over the window; V is 1 below token m and 0 from there: o[i] is the share of the window below m"""
    n, i = 323, np.arange(323)
    q, k, _ = inputs(4, 2, dev, (n,))
    v = torch.from_numpy((i < m).astype(np.float32)).to(torch.bfloat16).to(dev)[:, None, None].expand(n, 2, 128).contiguous()
    o = f64(window(torch.zeros_like(q), k, v, W))
    want = (np.maximum(0, np.minimum(m, i + 1) - np.maximum(0, i - W + 1)) / np.minimum(i + 1, W))[:, None, None]
    bad = np.abs(o - want) > 2.0 ** (np.floor(np.log2(np.maximum(want, 1e-30))) - 7)
    assert not bad.any(), f"first wrong (token, head, dim): {np.argwhere(bad)[0]}, got {o[bad][0]}, want {np.broadcast_to(want, o.shape)[bad][0]}"


@pytest.mark.parametrize("W,t", [(100, 70), (31, 200), (64, 63), (1, 128)])
def test_isolation(dev, W, t):
    """1e3 planted in K and V at token t changes exactly the queries t .. t + W - 1 (q > 0, so t's score is the largest of every row that
    attends it); NaN in the neighbouring sequences changes nothing"""
    lens = (65, 323, 128)
    a, b, ip = lens[0], lens[0] + lens[1], indptr_of(lens, dev)
    q, k, v = (x.clone() for x in inputs(8, 2, dev, lens))
    o = window(q.abs_(), k, v, W, ip)
    k[a + t], v[a + t] = 1e3, 1e3
    for x in (q, k, v):
        x[:a], x[b:] = float("nan"), float("nan")
    o2 = window(q, k, v, W, ip)
    same, i = (bits(o)[a:b] == bits(o2)[a:b]).flatten(1).all(1).cpu().numpy(), np.arange(lens[1])
    attends = (i >= t) & (i - W + 1 <= t)
    assert torch.isfinite(o2[a:b].float()).all() and np.array_equal(~same, attends), f"wrong at rows {np.flatnonzero(same == attends)}"


def test_same_bits_views_and_graph_replay(dev):
    """where the window does not bind the bits are dense_attention's; views of one packed projection equal copies; a replay equals eager"""
    Hq, Hkv, lens, other, W = 8, 2, [64, 323, 100, 1], [387, 65, 36, 0], 100
    T, ip = sum(lens), indptr_of(lens, dev)
    packed = rand_bf16((T, (Hq + 2 * Hkv) * 128), np.random.default_rng(11), dev)
    q, k, v = packed[:, :Hq * 128], packed[:, Hq * 128:(Hq + Hkv) * 128], packed[:, (Hq + Hkv) * 128:]
    dense = bits(mixedgemm.dense_attention(q, k, v, ip))
    for big in (T, T + 1, 2 ** 40):
        assert torch.equal(bits(window(q, k, v, big, ip)), dense), f"window {big} >= T differs from dense_attention"
    o, want, short = window(q, k, v, W, ip), window(q, k, v, W, indptr_of(other, dev)), torch.ones(T, dtype=torch.bool)
    short[64 + W:64 + 323] = False                             # the rows of the long sequence past its first W
    assert torch.equal(bits(o)[short], dense[short]), "a row whose window holds its whole past differs from dense_attention"
    assert not torch.equal(bits(o)[~short], dense[~short]) and not torch.equal(bits(o), bits(want))
    assert torch.equal(bits(o), bits(window(q.contiguous(), k.contiguous(), v.contiguous(), W, ip))), "views differ from copies"
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        window(q, k, v, W, ip)
        with torch.cuda.graph(graph, stream=side):
            out = window(q, k, v, W, ip)
    ip.copy_(indptr_of(other, dev))                            # another split of the same T, read by the replays on the device
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(want)), "a replay after seq_indptr was rewritten differs from the eager call"


@pytest.mark.parametrize("kind", ["int4", "fp8_e4m3", "bf16"])
def test_prefill_fresh_windowed(dev, kind):
    rng, lens, Hq, Hkv, W, layer = np.random.default_rng(8), [0, 1, 63, 64, 65, 129], 8, 2, 64, 1
    split = lambda t: (t[:, : Hq * 128], t[:, Hq * 128: (Hq + Hkv) * 128], t[:, (Hq + Hkv) * 128:])       # noqa: E731
    qkv, step = split(rand_bf16((sum(lens), (Hq + 2 * Hkv) * 128), rng, dev)), split(rand_bf16((len(lens), (Hq + 2 * Hkv) * 128), rng, dev))
    tabs = [from_bits(t, dev) for t in ro.llama3_tables(np.concatenate([np.arange(n) for n in lens]))]
    a, b, c = (PagedKVCache(2, Hkv, 16, 32, len(lens), kind=kind, device=dev, window=W) for _ in range(3))
    a.extend(lens), b.extend(lens), c.extend(lens)
    with pytest.raises(ValueError, match="attend_new"):                        # the default call keeps refusing a windowed cache
        a.prefill_fresh(layer, *qkv, *tabs)
    o = a.prefill_fresh(layer, *qkv, *tabs, windowed=True)
    seen = b.append_rope(layer, *qkv, *tabs, dense=True)                       # q_rot, k_seen, v_seen (bf16: v itself, [T, Hkv * 128])
    c.append_rope(layer, *qkv, *tabs)
    assert torch.equal(a.kv_data.view(torch.uint8), c.kv_data.view(torch.uint8)), "cache bytes differ from append_rope()'s"
    assert_within_7c(o, *reference(*seen, lens, W), kind)
    a.extend(1), c.extend(1)                                                   # releases the pages below the window of the 65 and the 129
    tabs = [from_bits(t, dev) for t in ro.llama3_tables(lens)]
    res = [cache.attend(layer, cache.append_rope(layer, *step, *tabs)) for cache in (a, c)]
    assert torch.equal(bits(res[0]), bits(res[1]))
