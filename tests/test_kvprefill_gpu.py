"""GPU tests of causal multi-token attention over the paged KV cache (mixedgemm.paged_prefill, PagedKVCache.attend_new) against
tests/kv_prefill_oracle.py."""
import math

import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_oracle as ko
import kv_prefill_oracle as kpo

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def dev_i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def rand_bf16(shape, rng, dev, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * scale).to(torch.bfloat16).to(dev)


def host(data, param):
    d = data.cpu()
    d = d.numpy() if d.dtype == torch.uint8 else d.view(torch.int16).numpy().view(np.uint16)
    return d.copy(), (param.cpu().numpy().copy() if param is not None else None)


def indptr_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def build(kind, prior, new, Hq, Hkv, P, rng, dev, L=2, layer=1, scale_v=0.5):
    """a cache whose sequences hold prior[b] + new[b] tokens (all appended by kv_append), shuffled pages; returns the pieces a
    paged_prefill call over the new tokens needs"""
    lens = [a + n for a, n in zip(prior, new)]
    npg = [-(-n // P) for n in lens]
    max_pages = sum(npg) + 3
    perm = rng.permutation(max_pages)[: sum(npg)].astype(np.int32)
    indptr, last = indptr_of(npg), np.array([n - (k - 1) * P if k else 0 for n, k in zip(lens, npg)], dtype=np.int32)
    if kind == "int4":
        data = torch.zeros((max_pages, L, 2, Hkv, P, 64), dtype=torch.uint8, device=dev)
        param = torch.zeros((max_pages, L, 2, Hkv, P, 2), dtype=torch.float16, device=dev)
    else:
        data, param = torch.zeros((max_pages, L, 2, Hkv, P, 128), dtype=torch.bfloat16, device=dev), None
    tbl = [dev_i32(a, dev) for a in (indptr, perm, last)]
    T = sum(lens)
    k, v = rand_bf16((T, Hkv, 128), rng, dev), rand_bf16((T, Hkv, 128), rng, dev, scale_v)
    mixedgemm.kv_append(data, param, *tbl, k, v, dev_i32(indptr_of(lens), dev), layer)
    qo = indptr_of(new)
    q = rand_bf16((int(qo[-1]), Hq, 128), rng, dev, 2.0)
    return dict(data=data, param=param, tbl=tbl, tbl_h=(indptr, perm, last), qo=qo, qo_d=dev_i32(qo, dev), q=q, layer=layer,
                msl=max(lens) if lens else 0)


def run(c, msl=None, q=None):
    return mixedgemm.paged_prefill(c["q"] if q is None else q, c["data"], c["param"], *c["tbl"], c["qo_d"], c["layer"],
                                   c["msl"] if msl is None else msl)


def oracle(c, q=None):
    hd, hp = host(c["data"], c["param"])
    qb = bits(c["q"] if q is None else q)
    want = kpo.attention(qb, hd, hp, *c["tbl_h"], c["qo"], c["layer"])
    vm = kpo.vmax(qb.shape, hd, hp, *c["tbl_h"], c["qo"], c["layer"])
    return want, vm


def check(o, want, vmax, what=""):
    """|o - ref| <= 2 bf16 ulp(ref) + 2^-8 max|V| over the attended tokens"""
    got = o.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-30))) - 7)
    err = np.abs(got - want)
    bad = err > 2 * ulp + 2.0 ** -8 * vmax
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outputs outside the bound; worst err {err.max():.3e}"


# (Hq, Hkv, P, prior lengths, new tokens per sequence)
CASES = [
    (32, 8, 16, [0], [300]),                                          # square prefill
    (32, 8, 1, [0, 5, 40, 0], [15, 16, 17, 1]),
    (40, 8, 24, [100, 0, 7, 64, 1000], [65, 64, 0, 17, 16]),          # g = 5: 12 tokens x 5 heads per tile
    (32, 32, 64, [0, 33, 500], [65, 1, 64]),                          # g = 1: 64 tokens per tile
    (128, 8, 16, [3, 0, 200], [17, 15, 33]),                          # g = 16: 4 tokens per tile
    (32, 8, 16, [32768 - 17], [17]),                                  # chunk over 32k: the split path
    (40, 8, 64, [0, 2048, 0], [1, 300, 0]),
]


@pytest.mark.parametrize("kind", ["int4", "bf16"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_prefill_against_oracle(dev, kind, case):
    Hq, Hkv, P, prior, new = CASES[case]
    rng = np.random.default_rng(200 + case)
    c = build(kind, prior, new, Hq, Hkv, P, rng, dev)
    T, B = c["q"].size(0), len(new)
    if case == 5:
        assert mixedgemm.paged_prefill_workspace_bytes(T, B, Hq, Hkv, c["msl"]) > 0, "the 32k case must take the split path"
    o = run(c)
    o2 = run(c)
    o_loose = run(c, msl=c["msl"] + 5000)                             # a looser bound: another split, the same function
    torch.cuda.synchronize()
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16)), "two launches differ"
    want, vm = oracle(c)
    check(o, want, vm, "tight bound")
    check(o_loose, want, vm, "loose bound")


def test_page_sizes_and_empty_sequences(dev):
    """P in {1, 16, 24, 64}; a length-0 sequence and queries the table does not count give zeros"""
    rng = np.random.default_rng(9)
    for P in (1, 16, 24, 64):
        c = build("int4", [0, 70, 0], [5, 20, 0], 32, 8, P, rng, dev)
        o = run(c)
        torch.cuda.synchronize()
        want, vm = oracle(c)
        check(o, want, vm, f"P={P}")
    # a table that holds 2 of sequence 0's 5 tokens: its first 3 queries sit at negative positions
    c2 = build("bf16", [0], [5], 32, 8, 16, rng, dev)
    c2["tbl"][2].fill_(2)
    c2["tbl_h"] = (c2["tbl_h"][0], c2["tbl_h"][1], np.array([2], dtype=np.int32))
    o = run(c2)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(o[:3].float())) == 0
    want, vm = oracle(c2)
    check(o, want, vm, "uncounted tokens")


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_causality(dev, kind):
    """rewriting the last new token's K / V of each sequence (values of magnitude 1e3) leaves every earlier query's output bit-equal"""
    rng = np.random.default_rng(31)
    Hq, Hkv, P = 32, 8, 16
    prior, new = [0, 100, 31], [40, 17, 2]
    c = build(kind, prior, new, Hq, Hkv, P, rng, dev)
    before = run(c)
    one = np.ones(len(new), dtype=np.int32)                     # append one token per sequence: its last position
    big = torch.full((len(new), Hkv, 128), 1e3, device=dev) * torch.sign(torch.randn((len(new), Hkv, 128), device=dev))
    mixedgemm.kv_append(c["data"], c["param"], *c["tbl"], big.to(torch.bfloat16), (-big).to(torch.bfloat16), dev_i32(indptr_of(one), dev),
                        c["layer"])
    after = run(c)
    torch.cuda.synchronize()
    last = set((np.cumsum(new) - 1).tolist())
    for i in range(sum(new)):
        if i in last:
            assert not torch.equal(before[i].view(torch.int16), after[i].view(torch.int16)), f"token {i} should see the rewrite"
        else:
            assert torch.equal(before[i].view(torch.int16), after[i].view(torch.int16)), f"token {i} changed: it sees a later token"


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_single_token_matches_decode(dev, kind):
    rng = np.random.default_rng(41)
    for Hq, Hkv, prior in ((32, 8, [0, 16, 300, 4095]), (40, 8, [7, 1000]), (128, 8, [33])):
        B = len(prior)
        c = build(kind, prior, [1] * B, Hq, Hkv, 16, rng, dev)
        o = run(c)
        d = mixedgemm.paged_decode(c["q"], c["data"], c["param"], *c["tbl"], c["layer"], c["msl"])
        torch.cuda.synchronize()
        want, vm = oracle(c)
        check(o, want, vm, "prefill n_b = 1")
        check(o, d.float().cpu().numpy().astype(np.float64), vm, "prefill against paged_decode")


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_chunked_equals_whole(dev, kind):
    """a 1000-token prompt in one extend / append / attend_new, and in chunks of 256 / 256 / 256 / 232"""
    rng = np.random.default_rng(51)
    Hq, Hkv, N = 32, 8, 1000
    k, v = rand_bf16((N, Hkv, 128), rng, dev), rand_bf16((N, Hkv, 128), rng, dev, 0.5)
    q = rand_bf16((N, Hq, 128), rng, dev, 2.0)
    outs = []
    for chunks in ([N], [256, 256, 256, 232]):
        cache = PagedKVCache(1, Hkv, 16, 80, 1, kind=kind, device=dev)
        parts, t = [], 0
        for n in chunks:
            cache.extend(n)
            cache.append(0, k[t:t + n], v[t:t + n])
            parts.append(cache.attend_new(0, q[t:t + n]))
            t += n
        outs.append(torch.cat(parts))
    torch.cuda.synchronize()
    hd, hp = host(cache.kv_data, cache.kv_param)
    tbl = (cache.kv_indptr.cpu().numpy(), cache.kv_indices.cpu().numpy(), cache.last_page_len.cpu().numpy())
    qo = np.array([0, N])
    want = kpo.attention(bits(q), hd, hp, *tbl, qo, 0)
    vm = kpo.vmax(q.shape, hd, hp, *tbl, qo, 0)
    check(outs[0], want, vm, "whole")
    check(outs[1], want, vm, "chunked")
    check(outs[1], outs[0].float().cpu().numpy().astype(np.float64), vm, "chunked against whole")


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_graph_capture_over_extend_steps(dev, kind):
    """append + attend_new at B = 4, 5 tokens each, captured once; three replays over extend(5) steps, each bit-equal to eager"""
    B, Hq, Hkv, n = 4, 32, 8, 5
    cache = PagedKVCache(1, Hkv, 16, 256, B, kind=kind, device=dev)
    rng = np.random.default_rng(61)
    cache.extend([40, 5, 300, 0])
    cache.append(0, rand_bf16((345, Hkv, 128), rng, dev), rand_bf16((345, Hkv, 128), rng, dev))
    bound = 1024
    sk, sv, sq = (rand_bf16((B * n, h, 128), rng, dev) for h in (Hkv, Hkv, Hq))
    cache.extend(n)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cache.append(0, sk, sv)
        cache.attend_new(0, sq, max_seq_len=bound)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cache.append(0, sk, sv)
        out = cache.attend_new(0, sq, max_seq_len=bound)
    for step in range(3):
        if step:
            cache.extend(n)
        for t in (sk, sv, sq):
            t.copy_(rand_bf16(tuple(t.shape), rng, dev))
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        eager = cache.attend_new(0, sq, max_seq_len=bound)
        eager2 = cache.attend_new(0, sq, max_seq_len=bound)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), eager.view(torch.int16)), f"replay {step} differs from eager"
        assert torch.equal(eager.view(torch.int16), eager2.view(torch.int16)), "two launches differ"
        hd, hp = host(cache.kv_data, cache.kv_param)
        tbl = (cache.kv_indptr.cpu().numpy(), cache.kv_indices.cpu().numpy(), cache.last_page_len.cpu().numpy())
        qo = cache.append_indptr.cpu().numpy()
        check(got, kpo.attention(bits(sq), hd, hp, *tbl, qo, 0), kpo.vmax(sq.shape, hd, hp, *tbl, qo, 0), f"replay {step}")


def fake_quant(x):
    """quantize_int_group(x, 4, 128) of the reference (model/qLlamaLayer.py:13-23), in fp32"""
    shape = x.shape
    w = x.reshape(-1, 128).float()
    mx, mn = w.amax(-1, keepdim=True), w.amin(-1, keepdim=True)
    s = (mx - mn).clamp(min=1e-5) / 15
    base = torch.round(-mn / s).clamp_(0, 15)
    return ((torch.clamp(torch.round(w / s) + base, 0, 15) - base) * s).reshape(shape)


def causal_sdpa(q, k, v, g):
    """fp32 causal attention of a square prefill: q [N, Hq, 128], k / v [N, Hkv, 128] -> [N, Hq, 128]"""
    qq = q.float().transpose(0, 1)
    kk = k.float().transpose(0, 1).repeat_interleave(g, 0)
    vv = v.float().transpose(0, 1).repeat_interleave(g, 0)
    return torch.nn.functional.scaled_dot_product_attention(qq, kk, vv, is_causal=True).transpose(0, 1)


def test_quality_parity_with_reference_fake_quant(dev):
    """a square int4 prefill is within 5 % (mean abs error) of causal SDPA over quantize_int_group-fake-quantized K/V"""
    Hq, Hkv, N = 32, 8, 1024
    rng = np.random.default_rng(71)
    k, v = rand_bf16((N, Hkv, 128), rng, dev), rand_bf16((N, Hkv, 128), rng, dev)
    q = rand_bf16((N, Hq, 128), rng, dev, 2.0)
    cache = PagedKVCache(1, Hkv, 16, N // 16 + 1, 1, kind="int4", device=dev)
    cache.extend(N)
    cache.append(0, k, v)
    o = cache.attend_new(0, q).float()
    exact = causal_sdpa(q, k, v, Hq // Hkv)
    ref = causal_sdpa(q, fake_quant(k), fake_quant(v), Hq // Hkv)
    err_ours = (o - exact).abs().mean().item()
    err_ref = (ref - exact).abs().mean().item()
    assert err_ours <= 1.05 * err_ref, (err_ours, err_ref)


def test_llama3_prefill_step(dev):
    """q/k/v projection (FusedQLinear) -> RoPE -> append -> attend_new -> o_proj at M = 128 over 200 cached tokens, against the same
    chain with causal SDPA over fake-quantized K/V"""
    from micromix_amd.qlinear import FusedQLinear, QLinearLayer
    H, Hq, Hkv, T0, M = 4096, 32, 8, 200, 128
    g = torch.Generator().manual_seed(0)
    idx = torch.randperm(H, generator=g).to(torch.int16).to(dev)
    lin = lambda n, k: torch.nn.Linear(k, n, bias=False, dtype=torch.bfloat16).to(dev)
    qp, kp, vp, op = lin(Hq * 128, H), lin(Hkv * 128, H), lin(Hkv * 128, H), lin(H, Hq * 128)
    for m in (qp, kp, vp, op):
        m.weight.data = (torch.randn(m.weight.shape, generator=g) * 0.02).to(torch.bfloat16).to(dev)
    fused = FusedQLinear([QLinearLayer(m, p8_num=1024, p6_num=1024, reorder_index=idx) for m in (qp, kp, vp)])
    oproj = QLinearLayer(op, p8_num=1024, p6_num=1024, reorder_index=torch.arange(Hq * 128, dtype=torch.int16, device=dev))
    norm_w = (1 + 0.1 * torch.randn((H,), generator=g)).to(torch.bfloat16).to(dev)
    x = torch.randn((M, H), generator=g).to(torch.bfloat16).to(dev)
    q, k, v = fused.forward_norm(x, norm_w, 1e-5)
    inv = 1.0 / (500000.0 ** (torch.arange(0, 128, 2, device=dev).float() / 128))
    pos = (T0 + torch.arange(M, device=dev).float())[:, None, None]

    def rope(t, nh):
        t = t.reshape(M, nh, 128).float()
        ang = pos * inv
        cos, sin = torch.cat([ang.cos(), ang.cos()], -1), torch.cat([ang.sin(), ang.sin()], -1)
        return (t * cos + torch.cat([-t[..., 64:], t[..., :64]], -1) * sin).to(torch.bfloat16).contiguous()

    q, k = rope(q, Hq), rope(k, Hkv)
    v = v.reshape(M, Hkv, 128).contiguous()
    rng = np.random.default_rng(4)
    past_k, past_v = rand_bf16((T0, Hkv, 128), rng, dev), rand_bf16((T0, Hkv, 128), rng, dev)
    cache = PagedKVCache(1, Hkv, 16, 64, 1, kind="int4", device=dev)
    cache.extend(T0)
    cache.append(0, past_k, past_v)
    cache.extend(M)
    cache.append(0, k, v)
    attn = cache.attend_new(0, q)
    y = oproj(attn.reshape(1, M, Hq * 128)).reshape(M, H).float()
    allk, allv = fake_quant(torch.cat([past_k, k])), fake_quant(torch.cat([past_v, v]))
    # bottom-right causal mask: query i sees positions 0 .. T0 + i
    mask = torch.arange(T0 + M, device=dev)[None, :] <= (T0 + torch.arange(M, device=dev))[:, None]
    qq = q.float().transpose(0, 1)
    kk, vv = allk.transpose(0, 1).repeat_interleave(Hq // Hkv, 0), allv.transpose(0, 1).repeat_interleave(Hq // Hkv, 0)
    ref_attn = torch.nn.functional.scaled_dot_product_attention(qq, kk, vv, attn_mask=mask).transpose(0, 1).to(torch.bfloat16)
    y_ref = oproj(ref_attn.reshape(1, M, Hq * 128)).reshape(M, H).float()
    rel_attn = ((attn.float() - ref_attn.float()).norm() / ref_attn.float().norm()).item()
    assert math.isfinite(rel_attn) and rel_attn < 0.03, rel_attn
    rel = ((y - y_ref).norm() / y_ref.norm()).item()
    assert math.isfinite(rel) and rel < 0.1, rel
