"""GPU tests of the paged KV cache (mixedgemm.kv_append / paged_decode, micromix_amd.kvcache.PagedKVCache) against tests/kv_oracle.py."""
import math

import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_oracle as ko

pytestmark = pytest.mark.gpu

BF16_ULP_TOL = 2


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def empty_cache(kind, max_pages, L, Hkv, P, dev, poison=0xA5):
    if kind == "int4":
        data = torch.full((max_pages, L, 2, Hkv, P, 64), poison, dtype=torch.uint8, device=dev)
        param = torch.full((max_pages, L, 2, Hkv, P, 2), -7.0, dtype=torch.float16, device=dev)
    else:
        data = torch.full((max_pages, L, 2, Hkv, P, 128), 0x5A5A, dtype=torch.int16, device=dev).view(torch.bfloat16)
        param = None
    return data, param


def host(data, param):
    d = data.cpu()
    d = d.numpy() if d.dtype == torch.uint8 else d.view(torch.int16).numpy().view(np.uint16)
    return d.copy(), (param.cpu().numpy().copy() if param is not None else None)


def page_table(lens, P, max_pages, rng):
    """shuffled, non-contiguous pages for sequences of the given lengths"""
    npg = [-(-n // P) for n in lens]
    perm = rng.permutation(max_pages)[: sum(npg)]
    indptr = np.concatenate([[0], np.cumsum(npg)]).astype(np.int32)
    last = np.array([n - (k - 1) * P if k else 0 for n, k in zip(lens, npg)], dtype=np.int32)
    return indptr, perm.astype(np.int32), last


def dev_i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def rand_bf16(shape, rng, dev, scale=1.0):
    x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * scale)
    return x.to(torch.bfloat16).to(dev)


def run_append(kind, P, lens_before, new, L, layer, Hkv, max_pages, rng, dev, data=None, param=None):
    """append `new[b]` tokens to sequences already holding lens_before[b]; compare with the oracle byte for byte"""
    lens = [a + n for a, n in zip(lens_before, new)]
    indptr, indices, last = page_table(lens, P, max_pages, rng)
    if data is None:
        data, param = empty_cache(kind, max_pages, L, Hkv, P, dev)
    want_d, want_p = host(data, param)
    T = sum(new)
    k = rand_bf16((T, Hkv, 128), rng, dev, 2.0)
    v = rand_bf16((T, Hkv, 128), rng, dev, 0.5)
    app = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
    mixedgemm.kv_append(data, param, dev_i32(indptr, dev), dev_i32(indices, dev), dev_i32(last, dev), k, v, dev_i32(app, dev), layer)
    torch.cuda.synchronize()
    ko.append(want_d, want_p, indptr, indices, last, bits(k), bits(v), app, layer)
    got_d, got_p = host(data, param)
    assert np.array_equal(got_d, want_d), f"{int((got_d != want_d).sum())} cache bytes differ"
    if param is not None:
        assert np.array_equal(got_p.view(np.uint16), want_p.view(np.uint16)), "params differ"
    return indptr, indices, last


@pytest.mark.parametrize("kind", ["int4", "bf16"])
@pytest.mark.parametrize("P", [1, 16, 24, 64])
def test_append_byte_exact(dev, kind, P):
    rng = np.random.default_rng(P)
    Hkv, L, layer = 4, 3, 1
    before = [0, 5, P - 1 if P > 1 else 0, 3 * P + 2, 40]
    new = [17, 1, 2, 0, 3]
    max_pages = sum(-(-(a + n) // P) for a, n in zip(before, new)) + 7
    run_append(kind, P, before, new, L, layer, Hkv, max_pages, rng, dev)


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_append_prefill_then_decode_steps(dev, kind):
    rng = np.random.default_rng(7)
    Hkv, L, P, layer, max_pages = 8, 3, 16, 1, 64
    data, param = empty_cache(kind, max_pages, L, Hkv, P, dev)
    lens = [0, 0, 0]
    prefill = [37, 16, 1]
    perm = rng.permutation(max_pages)
    pages = [[], [], []]
    want_d, want_p = host(data, param)
    for step, new in enumerate([prefill, [1, 1, 1], [1, 1, 1], [1, 0, 1], [1, 1, 1]]):
        for b in range(3):
            lens[b] += new[b]
            while len(pages[b]) * P < lens[b]:
                pages[b].append(int(perm[sum(map(len, pages))]))
        indptr = np.concatenate([[0], np.cumsum([len(p) for p in pages])]).astype(np.int32)
        indices = np.array(sum(pages, []), dtype=np.int32)
        last = np.array([n - (len(p) - 1) * P if n else 0 for n, p in zip(lens, pages)], dtype=np.int32)
        T = sum(new)
        k, v = rand_bf16((T, Hkv, 128), rng, dev), rand_bf16((T, Hkv, 128), rng, dev)
        app = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
        mixedgemm.kv_append(data, param, dev_i32(indptr, dev), dev_i32(indices, dev), dev_i32(last, dev), k, v, dev_i32(app, dev), layer)
        ko.append(want_d, want_p, indptr, indices, last, bits(k), bits(v), app, layer)
    torch.cuda.synchronize()
    got_d, got_p = host(data, param)
    assert np.array_equal(got_d, want_d)
    if param is not None:
        assert np.array_equal(got_p.view(np.uint16), want_p.view(np.uint16))


def test_append_page_past_2gib(dev):
    """one bf16 page whose rows lie beyond byte offset 2^31 (64-bit addressing); only the target rows change"""
    P, L, Hkv = 16, 2, 8
    page_bytes = L * 2 * Hkv * P * 128 * 2
    max_pages = (2 ** 31) // page_bytes + 2
    data = torch.zeros((max_pages, L, 2, Hkv, P, 128), dtype=torch.bfloat16, device=dev)
    far = max_pages - 1
    assert far * page_bytes > 2 ** 31
    rng = np.random.default_rng(3)
    k, v = rand_bf16((3, Hkv, 128), rng, dev), rand_bf16((3, Hkv, 128), rng, dev)
    i32 = lambda a: dev_i32(np.array(a), dev)
    mixedgemm.kv_append(data, None, i32([0, 1]), i32([far]), i32([3]), k, v, i32([0, 3]), 1)
    torch.cuda.synchronize()
    assert torch.equal(data[far, 1, 0, :, :3].transpose(0, 1), k) and torch.equal(data[far, 1, 1, :, :3].transpose(0, 1), v)
    assert int(torch.count_nonzero(data[far].view(torch.int16))) == int(torch.count_nonzero(k.view(torch.int16))) + \
        int(torch.count_nonzero(v.view(torch.int16)))
    assert int(torch.count_nonzero(data[: far].view(torch.int16))) == 0
    # int4 codes of the same page position, against the oracle
    data4 = torch.zeros((max_pages * 4, L, 2, Hkv, P, 64), dtype=torch.uint8, device=dev)
    del data
    param4 = torch.zeros((max_pages * 4, L, 2, Hkv, P, 2), dtype=torch.float16, device=dev)
    far4 = max_pages * 4 - 1
    mixedgemm.kv_append(data4, param4, i32([0, 1]), i32([far4]), i32([3]), k, v, i32([0, 3]), 1)
    torch.cuda.synchronize()
    codes, s, z = ko.quantize_row(ko.bf16_to_f32(bits(k)))
    assert np.array_equal(data4[far4, 1, 0, :, :3].transpose(0, 1).cpu().numpy(), ko.pack_codes(codes))
    assert np.array_equal(param4[far4, 1, 0, :, :3, 0].transpose(0, 1).cpu().numpy().view(np.uint16), s.view(np.uint16))


def fill_cache(kind, lens, P, L, layer, Hkv, rng, dev, scale_k=1.0, scale_v=1.0):
    max_pages = sum(-(-n // P) for n in lens) + 3
    data, param = empty_cache(kind, max_pages, L, Hkv, P, dev, poison=0)
    if param is not None:
        param.zero_()
    indptr, indices, last = page_table(lens, P, max_pages, rng)
    T = sum(lens)
    k = rand_bf16((T, Hkv, 128), rng, dev, scale_k)
    v = rand_bf16((T, Hkv, 128), rng, dev, scale_v)
    tbl = [dev_i32(a, dev) for a in (indptr, indices, last)]
    mixedgemm.kv_append(data, param, *tbl, k, v, dev_i32(np.concatenate([[0], np.cumsum(lens)]), dev), layer)
    return data, param, (indptr, indices, last), tbl, k, v


def check_attention(o, want, vmax):
    got = o.float().cpu().numpy().astype(np.float64)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-30))) - 7)      # bf16 ulp of the oracle value
    err = np.abs(got - want)
    bad = (err > BF16_ULP_TOL * ulp) & (err > 1e-3 * vmax)
    assert not bad.any(), f"{int(bad.sum())} outputs outside 2 bf16 ulps / 1e-3 max|V|; worst err {err.max():.3e}"
    assert np.isfinite(got).all()


CASES = [
    # (Hq, Hkv, lens)
    (32, 8, [17]),
    (32, 8, [0, 1, 4096]),
    (40, 8, [15, 16, 17]),
    (40, 8, [4096, 0, 1, 15, 16, 17, 33, 4095]),
    (32, 32, [1, 16, 17]),
    (32, 8, [(i * 131) % 600 for i in range(33)]),
    (32, 8, [32768]),
]


@pytest.mark.parametrize("kind", ["int4", "bf16"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_decode_attention(dev, kind, case):
    Hq, Hkv, lens = CASES[case]
    rng = np.random.default_rng(100 + case)
    P, L, layer = 16, 2, 1
    data, param, tbl_h, tbl, k, v = fill_cache(kind, lens, P, L, layer, Hkv, rng, dev, scale_v=0.5)
    q = rand_bf16((len(lens), Hq, 128), rng, dev, 2.0)
    o = mixedgemm.paged_decode(q, data, param, *tbl, layer, max(lens))
    o2 = mixedgemm.paged_decode(q, data, param, *tbl, layer, max(lens))
    torch.cuda.synchronize()
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16)), "two launches differ"
    hd, hp = host(data, param)
    want = ko.attention(bits(q), hd, hp, *tbl_h, layer)
    for b, n in enumerate(lens):
        if n == 0:
            assert int(torch.count_nonzero(o[b].float())) == 0
    vmax = float(v.float().abs().max())
    check_attention(o, want, vmax)


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_decode_bound_larger_than_lengths_and_page_sizes(dev, kind):
    """the split follows max_seq_len, not the lengths: a loose bound and odd page sizes give the same answer"""
    rng = np.random.default_rng(5)
    for P in (1, 24, 64):
        lens = [3, 300, 77]
        data, param, tbl_h, tbl, k, v = fill_cache(kind, lens, P, 1, 0, 8, rng, dev)
        q = rand_bf16((3, 32, 128), rng, dev)
        o_tight = mixedgemm.paged_decode(q, data, param, *tbl, 0, 300)
        o_loose = mixedgemm.paged_decode(q, data, param, *tbl, 0, 20000)
        o_short = mixedgemm.paged_decode(q, data, param, *tbl, 0, 100)      # a bound too small still attends every token
        torch.cuda.synchronize()
        hd, hp = host(data, param)
        want = ko.attention(bits(q), hd, hp, *tbl_h, 0)
        vmax = float(v.float().abs().max())
        for o in (o_tight, o_loose, o_short):
            check_attention(o, want, vmax)


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_graph_capture_over_extend_steps(dev, kind):
    B, Hq, Hkv, L = 3, 32, 8, 2
    cache = PagedKVCache(L, Hkv, 16, 256, B, kind=kind, device=dev)
    rng = np.random.default_rng(11)
    cache.extend([40, 5, 70])
    for layer in range(L):
        cache.append(layer, rand_bf16((115, Hkv, 128), rng, dev), rand_bf16((115, Hkv, 128), rng, dev))
    bound = 512
    sk, sv, sq = (rand_bf16((B, h, 128), rng, dev) for h in (Hkv, Hkv, Hq))
    cache.extend(1)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cache.append(1, sk, sv)
        cache.attend(1, sq, max_seq_len=bound)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cache.append(1, sk, sv)
        out = cache.attend(1, sq, max_seq_len=bound)
    for step in range(4):
        if step:
            cache.extend(1)
        for t in (sk, sv, sq):
            t.copy_(rand_bf16(tuple(t.shape), rng, dev))
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        eager = cache.attend(1, sq, max_seq_len=bound)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), eager.view(torch.int16)), f"replay {step} differs from eager"
        hd, hp = host(cache.kv_data, cache.kv_param)
        want = ko.attention(bits(sq), hd, hp, cache.kv_indptr.cpu().numpy(), cache.kv_indices.cpu().numpy(),
                            cache.last_page_len.cpu().numpy(), 1)
        check_attention(got, want, 4.0)


def fake_quant(x):
    """quantize_int_group(x, 4, 128) of the reference (model/qLlamaLayer.py:13-23), in fp32"""
    shape = x.shape
    w = x.reshape(-1, 128).float()
    mx, mn = w.amax(-1, keepdim=True), w.amin(-1, keepdim=True)
    s = (mx - mn).clamp(min=1e-5) / 15
    base = torch.round(-mn / s).clamp_(0, 15)
    return ((torch.clamp(torch.round(w / s) + base, 0, 15) - base) * s).reshape(shape)


def sdpa(q, k, v, g):
    """fp32 attention of one token: q [B, Hq, 128], k / v [B, Hkv, T, 128]"""
    k, v = k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    return torch.nn.functional.scaled_dot_product_attention(q.float().unsqueeze(2), k.float(), v.float()).squeeze(2)


def test_quality_parity_with_reference_fake_quant(dev):
    """int4-cache attention is within 5 % (mean abs error) of SDPA over quantize_int_group-fake-quantized K/V"""
    B, Hq, Hkv, T = 4, 32, 8, 1024
    rng = np.random.default_rng(21)
    data, param, tbl_h, tbl, k, v = fill_cache("int4", [T] * B, 16, 1, 0, Hkv, rng, dev)
    q = rand_bf16((B, Hq, 128), rng, dev, 2.0)
    o = mixedgemm.paged_decode(q, data, param, *tbl, 0, T).float()
    kk = k.view(B, T, Hkv, 128).transpose(1, 2)
    vv = v.view(B, T, Hkv, 128).transpose(1, 2)
    exact = sdpa(q, kk, vv, Hq // Hkv)
    ref = sdpa(q, fake_quant(kk), fake_quant(vv), Hq // Hkv)
    err_ours = (o - exact).abs().mean().item()
    err_ref = (ref - exact).abs().mean().item()
    assert err_ours <= 1.05 * err_ref, (err_ours, err_ref)


def test_llama3_attention_step(dev):
    """q/k/v projection (FusedQLinear.forward_norm) -> RoPE -> append -> attend -> o_proj at M = 1, against the same chain with SDPA over
    fake-quantized K/V"""
    from micromix_amd.qlinear import FusedQLinear, QLinearLayer
    H, Hq, Hkv, T0 = 4096, 32, 8, 300
    g = torch.Generator().manual_seed(0)
    idx = torch.randperm(H, generator=g).to(torch.int16).to(dev)
    lin = lambda n, k: torch.nn.Linear(k, n, bias=False, dtype=torch.bfloat16).to(dev)
    qp, kp, vp, op = lin(Hq * 128, H), lin(Hkv * 128, H), lin(Hkv * 128, H), lin(H, Hq * 128)
    for m in (qp, kp, vp, op):
        m.weight.data = (torch.randn(m.weight.shape, generator=g) * 0.02).to(torch.bfloat16).to(dev)
    split = (2048, 1024, 1024)
    fused = FusedQLinear([QLinearLayer(m, p8_num=split[2], p6_num=split[1], reorder_index=idx) for m in (qp, kp, vp)])
    oidx = torch.arange(Hq * 128, dtype=torch.int16, device=dev)
    oproj = QLinearLayer(op, p8_num=1024, p6_num=1024, reorder_index=oidx)
    norm_w = (1 + 0.1 * torch.randn((H,), generator=g)).to(torch.bfloat16).to(dev)
    x = torch.randn((1, H), generator=g).to(torch.bfloat16).to(dev)
    q, k, v = fused.forward_norm(x, norm_w, 1e-5)

    def rope(t, pos, nh):
        t = t.view(1, nh, 128).float()
        inv = 1.0 / (500000.0 ** (torch.arange(0, 128, 2, device=dev).float() / 128))
        ang = pos * inv
        cos, sin = torch.cat([ang.cos(), ang.cos()]), torch.cat([ang.sin(), ang.sin()])
        rot = torch.cat([-t[..., 64:], t[..., :64]], -1)
        return (t * cos + rot * sin).to(torch.bfloat16)

    q, k = rope(q, T0, Hq), rope(k, T0, Hkv)
    v = v.view(1, Hkv, 128)
    rng = np.random.default_rng(4)
    past_k, past_v = rand_bf16((T0, Hkv, 128), rng, dev), rand_bf16((T0, Hkv, 128), rng, dev)
    cache = PagedKVCache(1, Hkv, 16, 64, 1, kind="int4", device=dev)
    cache.extend(T0)
    cache.append(0, past_k, past_v)
    cache.extend(1)
    cache.append(0, k.contiguous(), v.contiguous())
    attn = cache.attend(0, q.contiguous())
    y = oproj(attn.reshape(1, 1, Hq * 128)).reshape(1, H).float()
    allk = torch.cat([past_k, k.view(1, Hkv, 128)]).transpose(0, 1).unsqueeze(0)
    allv = torch.cat([past_v, v.view(1, Hkv, 128)]).transpose(0, 1).unsqueeze(0)
    ref_attn = sdpa(q, fake_quant(allk), fake_quant(allv), Hq // Hkv).to(torch.bfloat16)
    y_ref = oproj(ref_attn.reshape(1, 1, Hq * 128)).reshape(1, H).float()
    # the attention outputs differ only where the two rules' scales round differently (fp16 against fp32 parameters)
    rel_attn = ((attn.float() - ref_attn.float()).norm() / ref_attn.float().norm()).item()
    assert math.isfinite(rel_attn) and rel_attn < 0.03, rel_attn
    # o_proj re-quantizes its input to MX formats, so bf16-level input differences flip element codes: a looser bound on y
    rel = ((y - y_ref).norm() / y_ref.norm()).item()
    assert math.isfinite(rel) and rel < 0.1, rel
