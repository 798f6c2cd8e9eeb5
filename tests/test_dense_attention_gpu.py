"""GPU tests of dense causal GQA attention over contiguous bf16 q, k, v (mixedgemm.dense_attention, include/micromix_attention.h): a
plain fp64 reference, an exact count, causality and isolation, in-place views and graph replay.  The shapes stand on the edges of the
kernel's query tile BQ and kv tile BK."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm

pytestmark = pytest.mark.gpu

BQ, BK = _lib.ATTENTION["MM_DENSE_ATTN_BQ"], _lib.ATTENTION["MM_DENSE_ATTN_BK"]
LONG = 2 * BQ + BK + 3
LENS = [BK, 0, LONG, 1, BQ + 1, BK - 1, BQ, BK + 1, BQ - 1]           # {0, 1, BK -1 .. BK + 1, BQ - 1 .. BQ + 1, LONG}, shuffled


def indptr_of(lens, dev):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)


def rand_bf16(shape, rng, dev, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * scale).to(torch.bfloat16).to(dev)


def f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def bits(t):
    return t.contiguous().view(torch.int16)


def reference(q, k, v, lens, sm_scale):
    """fp64 causal GQA attention over the bf16 values; also max |V| over the tokens each output attends"""
    q, k, v = f64(q), f64(k), f64(v)
    g, o, vmax, t0 = q.shape[1] // k.shape[1], np.zeros(q.shape), np.zeros(q.shape[:2] + (1,)), 0
    for n in lens:
        for h in range(q.shape[1] if n else 0):
            s = q[t0:t0 + n, h] @ k[t0:t0 + n, h // g].T * sm_scale
            s[np.triu_indices(n, 1)] = -np.inf
            p = np.exp(s - s.max(axis=1, keepdims=True))
            o[t0:t0 + n, h] = p @ v[t0:t0 + n, h // g] / p.sum(axis=1, keepdims=True)
            vmax[t0:t0 + n, h, 0] = np.maximum.accumulate(np.abs(v[t0:t0 + n, h // g]).max(axis=1))
        t0 += n
    return o, vmax


@pytest.mark.parametrize("sm_scale", [0.02, 0.3], ids=["loose", "tight"])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2), (5, 1), (16, 1)])
def test_against_fp64(dev, Hq, Hkv, sm_scale):
    """|o - ref| <= 2 bf16 ulp(ref) + 2^-8 max|V| over the attended tokens, one ragged batch on every tile edge"""
    rng = np.random.default_rng(Hq * 100 + Hkv)
    T = sum(LENS)
    q, k, v = rand_bf16((T, Hq, 128), rng, dev, 2.0), rand_bf16((T, Hkv, 128), rng, dev), rand_bf16((T, Hkv, 128), rng, dev, 0.5)
    o = mixedgemm.dense_attention(q, k, v, indptr_of(LENS, dev), sm_scale)
    assert o.shape == (T, Hq, 128) and o.dtype is torch.bfloat16
    want, vmax = reference(q, k, v, LENS, sm_scale)
    got = f64(o)
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-30))) - 7)
    bad = err > 2 * ulp + 2.0 ** -8 * vmax
    print(f"Hq {Hq} Hkv {Hkv} sm_scale {sm_scale}: worst err {err.max():.3e}, worst err / bound {(err / (2 * ulp + 2.0 ** -8 * vmax)).max():.3f}")
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} outputs outside the bound; worst err {err.max():.3e}"


@pytest.mark.parametrize("m", [1, BK - 1, BK, BK + 1, BQ - 1, BQ, BQ + 1, 2 * BQ, 2 * BQ + BK, LONG])
def test_exact_count(dev, m):
    """q = 0 makes the softmax uniform; V is 1 below token m and 0 from there: o[i] = min(i + 1, m) / (i + 1) to 1 bf16 ulp, at every i"""
    Hq, Hkv, lens = 4, 2, [LONG, LONG]
    T = sum(lens)
    rng = np.random.default_rng(m)
    q, k = torch.zeros((T, Hq, 128), dtype=torch.bfloat16, device=dev), rand_bf16((T, Hkv, 128), rng, dev)
    i = torch.arange(LONG, device=dev).repeat(2)
    v = (i < m).to(torch.bfloat16)[:, None, None].expand(T, Hkv, 128).contiguous()
    o = f64(mixedgemm.dense_attention(q, k, v, indptr_of(lens, dev)))
    want = (torch.clamp(i + 1, max=m).double() / (i + 1).double()).cpu().numpy()[:, None, None]
    ulp = 2.0 ** (np.floor(np.log2(want)) - 7)
    bad = np.abs(o - want) > ulp
    assert not bad.any(), f"first wrong (token, head, dim): {np.argwhere(bad)[0]}, got {o[bad][0]}, want {np.broadcast_to(want, o.shape)[bad][0]}"


def test_causality_and_isolation(dev):
    """the last token's k, v set to 1e3 and the neighbouring sequences' tokens to NaN leave every other query's bits as they were"""
    Hq, Hkv, lens = 8, 2, [BK + 1, LONG, BQ]
    rng = np.random.default_rng(7)
    T, a, b = sum(lens), lens[0], lens[0] + lens[1]
    q, k, v = rand_bf16((T, Hq, 128), rng, dev, 2.0), rand_bf16((T, Hkv, 128), rng, dev), rand_bf16((T, Hkv, 128), rng, dev)
    ip = indptr_of(lens, dev)
    o = mixedgemm.dense_attention(q, k, v, ip)
    q2, k2, v2 = q.clone(), k.clone(), v.clone()
    k2[b - 1], v2[b - 1] = 1e3, 1e3
    for t in (q2, k2, v2):
        t[:a], t[b:] = float("nan"), float("nan")
    o2 = mixedgemm.dense_attention(q2, k2, v2, ip)
    assert torch.equal(bits(o)[a:b - 1], bits(o2)[a:b - 1])
    assert torch.isfinite(o2[b - 1].float()).all() and not torch.equal(bits(o)[b - 1], bits(o2)[b - 1])


def test_in_place_views_two_launches_and_graph_replay(dev):
    Hq, Hkv, lens, other = 8, 2, [BQ + 1, LONG], [LONG + BK, BQ + 1 - BK]
    rng = np.random.default_rng(11)
    T = sum(lens)
    packed = rand_bf16((T, (Hq + 2 * Hkv) * 128), rng, dev)
    q, k, v = packed[:, :Hq * 128], packed[:, Hq * 128:(Hq + Hkv) * 128], packed[:, (Hq + Hkv) * 128:]
    ip = indptr_of(lens, dev)
    o = mixedgemm.dense_attention(q, k, v, ip)
    assert torch.equal(bits(o), bits(mixedgemm.dense_attention(q.contiguous(), k.contiguous(), v.contiguous(), ip))), "views differ from copies"
    assert torch.equal(bits(o), bits(mixedgemm.dense_attention(q, k, v, ip))), "two launches differ"
    want = mixedgemm.dense_attention(q, k, v, indptr_of(other, dev))
    assert not torch.equal(bits(o), bits(want))
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        mixedgemm.dense_attention(q, k, v, ip)
        with torch.cuda.graph(graph, stream=side):
            out = mixedgemm.dense_attention(q, k, v, ip)
    ip.copy_(indptr_of(other, dev))                        # another split of the same T, read by the replay on the device
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(want)), "the replay after seq_indptr was rewritten differs from the eager call"
