"""GPU tests of the cache-less route for 64-wide heads (include/micromix_attention_hd64.h): mixedgemm.dense_attention(_window) and rope_qk
given [T, H, 64] tensors.  A plain fp64 reference (causal and band), an exact count, causality and isolation, in-place views, graph
replay, and RoPE against the header's element rule in torch bf16 arithmetic.  The shapes stand on the edges of the kernel's tiles."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm

pytestmark = pytest.mark.gpu

BQ, BK, TPW = (_lib.ATTENTION_HD64[n] for n in ("MM_DENSE_ATTN_HD64_BQ", "MM_DENSE_ATTN_HD64_BK", "MM_ROPE_HD64_TOKENS"))
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


def attend(q, k, v, ip, window, sm_scale=None):
    return mixedgemm.dense_attention_window(q, k, v, window, ip, sm_scale) if window else mixedgemm.dense_attention(q, k, v, ip, sm_scale)


def reference(q, k, v, lens, sm_scale, window):
    """fp64 causal (window 0) or band GQA attention over the bf16 values; also max |V| over the tokens each output attends"""
    q, k, v = f64(q), f64(k), f64(v)
    g, o, vmax, t0 = q.shape[1] // k.shape[1], np.zeros(q.shape), np.zeros(q.shape[:2] + (1,)), 0
    for n in lens:
        i = np.arange(n)
        keep = (i[None, :] <= i[:, None]) & ((i[None, :] > i[:, None] - window) | (window == 0))
        for h in range(q.shape[1] if n else 0):
            s = np.where(keep, q[t0:t0 + n, h] @ k[t0:t0 + n, h // g].T * sm_scale, -np.inf)
            p = np.exp(s - s.max(axis=1, keepdims=True))
            o[t0:t0 + n, h] = p @ v[t0:t0 + n, h // g] / p.sum(axis=1, keepdims=True)
            vmax[t0:t0 + n, h, 0] = np.where(keep, np.abs(v[t0:t0 + n, h // g]).max(axis=1)[None, :], 0.0).max(axis=1)
        t0 += n
    return o, vmax


@pytest.mark.parametrize("window", [0, 1, BK - 1, BK + 1, BQ + 1, 200])
@pytest.mark.parametrize("sm_scale", [0.03, 0.4], ids=["loose", "tight"])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2), (5, 1)])
def test_against_fp64(dev, Hq, Hkv, sm_scale, window):
    """|o - ref| <= 2 bf16 ulp(ref) + 2^-8 max|V| over the attended tokens, one ragged batch on every tile edge.
    Worst error / bound measured over the 36 cases: see DESIGN.md 7z"""
    rng = np.random.default_rng(Hq * 100 + Hkv)
    T = sum(LENS)
    q, k, v = rand_bf16((T, Hq, 64), rng, dev, 2.0), rand_bf16((T, Hkv, 64), rng, dev), rand_bf16((T, Hkv, 64), rng, dev, 0.5)
    o = attend(q, k, v, indptr_of(LENS, dev), window, sm_scale)
    assert o.shape == (T, Hq, 64) and o.dtype is torch.bfloat16
    want, vmax = reference(q, k, v, LENS, sm_scale, window)
    got = f64(o)
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    bound = 2 * 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-30))) - 7) + 2.0 ** -8 * vmax
    print(f"Hq {Hq} Hkv {Hkv} sm_scale {sm_scale} window {window}: worst err {err.max():.3e}, worst err / bound {(err / bound).max():.3f}")
    assert not (err > bound).any(), f"{int((err > bound).sum())} of {err.size} outputs outside the bound; worst err {err.max():.3e}"


def test_default_scale_is_that_of_64(dev):
    rng = np.random.default_rng(3)
    q, k, v = rand_bf16((BK + 1, 4, 64), rng, dev, 2.0), rand_bf16((BK + 1, 2, 64), rng, dev), rand_bf16((BK + 1, 2, 64), rng, dev)
    assert torch.equal(bits(mixedgemm.dense_attention(q, k, v)), bits(mixedgemm.dense_attention(q, k, v, sm_scale=0.125)))


@pytest.mark.parametrize("window", [0, BK + 5])
@pytest.mark.parametrize("m", [1, BK - 1, BK, BK + 1, BQ - 1, BQ, BQ + 1, 2 * BQ, 2 * BQ + BK, LONG])
def test_exact_count(dev, m, window):
    """q = 0 makes the softmax uniform; V is 1 below token m and 0 from there: o[i] = (attended tokens below m) / (attended tokens) to
    1 bf16 ulp at every i.  With the window the lower edge i - W + 1 walks over every alignment of a kv tile as i walks the sequence"""
    Hq, Hkv, lens = 4, 2, [LONG, LONG]
    T = sum(lens)
    q, k = torch.zeros((T, Hq, 64), dtype=torch.bfloat16, device=dev), rand_bf16((T, Hkv, 64), np.random.default_rng(m), dev)
    i = torch.arange(LONG, device=dev).repeat(2)
    v = (i < m).to(torch.bfloat16)[:, None, None].expand(T, Hkv, 64).contiguous()
    o = f64(attend(q, k, v, indptr_of(lens, dev), window))
    lo = torch.clamp(i - window + 1, min=0) if window else torch.zeros_like(i)
    want = (torch.clamp(torch.clamp(i + 1, max=m) - lo, min=0).double() / (i + 1 - lo).double()).cpu().numpy()[:, None, None]
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(want, 2.0 ** -126))) - 7)
    bad = np.abs(o - want) > ulp
    assert not bad.any(), f"first wrong (token, head, dim): {np.argwhere(bad)[0]}, got {o[bad][0]}, want {np.broadcast_to(want, o.shape)[bad][0]}"


@pytest.mark.parametrize("window", [0, BK + 1])
def test_causality_and_isolation(dev, window):
    """the last token's k, v set to 1e3 and the neighbouring sequences' tokens to NaN leave every other query's bits as they were"""
    Hq, Hkv, lens = 8, 2, [BK + 1, LONG, BQ]
    rng = np.random.default_rng(7)
    T, a, b = sum(lens), lens[0], lens[0] + lens[1]
    q, k, v = rand_bf16((T, Hq, 64), rng, dev, 2.0), rand_bf16((T, Hkv, 64), rng, dev), rand_bf16((T, Hkv, 64), rng, dev)
    ip = indptr_of(lens, dev)
    o = attend(q, k, v, ip, window)
    q2, k2, v2 = q.clone(), k.clone(), v.clone()
    k2[b - 1], v2[b - 1] = 1e3, 1e3
    for t in (q2, k2, v2):
        t[:a], t[b:] = float("nan"), float("nan")
    o2 = attend(q2, k2, v2, ip, window)
    assert torch.equal(bits(o)[a:b - 1], bits(o2)[a:b - 1])
    assert torch.isfinite(o2[b - 1].float()).all() and not torch.equal(bits(o)[b - 1], bits(o2)[b - 1])


def packed_views(T, Hq, Hkv, rng, dev):
    packed = rand_bf16((T, (Hq + 2 * Hkv) * 64), rng, dev)
    return (packed[:, :Hq * 64].unflatten(1, (Hq, 64)), packed[:, Hq * 64:(Hq + Hkv) * 64].unflatten(1, (Hkv, 64)),
            packed[:, (Hq + Hkv) * 64:].unflatten(1, (Hkv, 64)))


@pytest.mark.parametrize("window", [0, BQ + 1])
def test_in_place_views_and_graph_replay(dev, window):
    Hq, Hkv, lens, other = 8, 2, [BQ + 1, LONG], [LONG + BK, BQ + 1 - BK]
    q, k, v = packed_views(sum(lens), Hq, Hkv, np.random.default_rng(11), dev)
    assert not q.is_contiguous() and q.data_ptr() + 2 * Hq * 64 == k.data_ptr()
    ip = indptr_of(lens, dev)
    o = attend(q, k, v, ip, window)
    assert torch.equal(bits(o), bits(attend(q.contiguous(), k.contiguous(), v.contiguous(), ip, window))), "views differ from copies"
    want = attend(q, k, v, indptr_of(other, dev), window)
    assert not torch.equal(bits(o), bits(want))
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        attend(q, k, v, ip, window)
        with torch.cuda.graph(graph, stream=side):
            out = attend(q, k, v, ip, window)
    ip.copy_(indptr_of(other, dev))                        # another split of the same T, read by the replay on the device
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(want)), "the replay after seq_indptr was rewritten differs from the eager call"


@pytest.mark.parametrize("T", [1, TPW - 1, TPW + 1, 300])
@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (5, 5), (72, 8)])
def test_rope_qk_bits(dev, Hq, Hkv, T):
    """bit equality with the header's element rule -- bf16(bf16(x cos) + bf16(rotate_half(x) sin)), the partner at d +- 32 -- evaluated in
    torch bf16 arithmetic on the CPU; packed views of q, k and a row stride on cos / sin.  (72, 8): 80 rows, 16 waves, 5 rows each"""
    rng = np.random.default_rng(T)
    q, k, _ = packed_views(T, Hq, Hkv, rng, dev)
    table = rand_bf16((T, 2, 72), rng, dev)
    cos, sin = table[:, 0, :64], table[:, 1, :64]
    q_rot, k_rot = mixedgemm.rope_qk(q, k, cos, sin)
    assert q_rot.shape == (T, Hq, 64) and k_rot.shape == (T, Hkv, 64) and q_rot.is_contiguous() and k_rot.is_contiguous()
    for got, x in ((q_rot, q), (k_rot, k)):
        x, c, s = x.cpu(), cos.cpu()[:, None, :], sin.cpu()[:, None, :]
        want = x * c + torch.cat([-x[..., 32:], x[..., :32]], dim=-1) * s
        assert torch.equal(bits(got.cpu()), bits(want))
