"""GPU tests of the prefill-shaped RoPE + KV append (include/micromix_rope.h: mm_rope_prefill; mixedgemm.rope_qk, rope_kv_append_dense,
PagedKVCache.append_rope(dense=True), prefill_fresh) against tests/rope_oracle.py, kv_oracle.py and kv_fp8_oracle.py.  Every comparison
is bit equality except the attention of prefill_fresh, which is held to DESIGN 7c's bound."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd._args import _stream_ptr
from micromix_amd.kvcache import PagedKVCache
from conftest import bits_from_t as bits, t_from_bits as from_bits
import kv_fp8_oracle as fo
import kv_oracle as ko
import rope_oracle as ro

pytestmark = pytest.mark.gpu
TPW = _lib.ROPE["MM_ROPE_PREFILL_TOKENS"]
L, LAYER, SENTINEL = 2, 1, 0x5A5A
KINDS = ["int4", "fp8_e4m3", "bf16"]
ARGS = "kv_data kv_param kv_dtype max_pages L layer Hkv P hd kv_indptr kv_indices last B q k v sq Hq cos sin sc app T q_out k_out v_out".split()
POINTERS = set("kv_data kv_param kv_indptr kv_indices last q k v cos sin app q_out k_out v_out".split())


def host(data, param):
    d = data.cpu()
    d = d.view(torch.uint8).numpy() if d.element_size() == 1 else d.view(torch.int16).numpy().view(np.uint16)
    return d.copy(), (param.cpu().numpy().copy() if param is not None else None)


def poisoned(kind, max_pages, Hkv, P, dev):
    if kind == "bf16":
        return torch.full((max_pages, L, 2, Hkv, P, 128), SENTINEL, dtype=torch.int16, device=dev).view(torch.bfloat16), None
    data = torch.full((max_pages, L, 2, Hkv, P, 64 if kind == "int4" else 128), 0xA5, dtype=torch.uint8, device=dev)
    return data, torch.full((max_pages, L, 2, Hkv, P, 2), -7.0, dtype=torch.float16, device=dev)


def seen(kind, data, param, pages, sl, which):
    """the bf16 bits a reader of the slots gets back, [n, Hkv, 128] (include/micromix_rope.h, k_out / v_out), from host copies"""
    rows = data[pages, LAYER, which, :, sl]
    if kind == "bf16":
        return rows
    prm = param[pages, LAYER, which, :, sl]
    if kind == "fp8_e4m3":
        return fo.dequantize(rows, prm)
    return ro.f32_to_bf16(ko.unpack_codes(rows).astype(np.float32) * prm[..., 0:1].astype(np.float32) - prm[..., 1:2].astype(np.float32))


def case(kind, Hq, Hkv, P, prior, new, rng, dev, tables=None):
    """inputs (views of one packed projection), a poisoned cache with shuffled pages, and what the oracles say of q, the cache, K and V"""
    lens = [a + n for a, n in zip(prior, new)]
    npg = [-(-n // P) for n in lens]
    max_pages = sum(npg) + 3
    indptr, indices = np.concatenate([[0], np.cumsum(npg)]).astype(np.int32), rng.permutation(max_pages)[: sum(npg)].astype(np.int32)
    last = np.array([n - (k - 1) * P if k else 0 for n, k in zip(lens, npg)], dtype=np.int32)
    app = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
    T = int(app[-1])
    x = rng.standard_normal((T, (Hq + 2 * Hkv) * 128)).astype(np.float32)
    x[0, (Hq + Hkv) * 128: (Hq + Hkv) * 128 + 128] = 1.5                         # V, token 0, head 0: a constant row
    x[T - 1, -128:] = np.linspace(-2.5, 12.5, 128).round()                      # V, last token, last head: s = 1 and -min / s = 2.5, a tie
    x[T - 1, -128], x[T - 1, -1] = -2.5, 12.5
    buf = torch.from_numpy(x).to(torch.bfloat16).to(dev)
    q, k, v = buf[:, : Hq * 128], buf[:, Hq * 128: (Hq + Hkv) * 128], buf[:, (Hq + Hkv) * 128:]
    cos_b, sin_b = ro.llama3_tables(rng.integers(0, 131072, T)) if tables is None else tables
    data, param = poisoned(kind, max_pages, Hkv, P, dev)
    want_d, want_p = host(data, param)
    qb, kb, vb = (bits(t).reshape(T, -1, 128) for t in (q, k, v))
    want_q, rk = ro.rope(qb, cos_b, sin_b), ro.rope(kb, cos_b, sin_b)
    (fo if kind == "fp8_e4m3" else ko).append(want_d, want_p, indptr, indices, last, rk, vb, app, LAYER)
    where = [ko.slots(indptr, indices, P, b, np.arange(lens[b] - n, lens[b])) for b, n in enumerate(new) if n]
    pages, sl = (np.concatenate(c) for c in zip(*where))
    return dict(q=q, k=k, v=v, buf=buf, cos=from_bits(cos_b, dev), sin=from_bits(sin_b, dev), data=data, param=param, T=T,
                tbl=[torch.from_numpy(a).to(dev) for a in (indptr, indices, last)], app=torch.from_numpy(app).to(dev), want_q=want_q, want_cache=(want_d, want_p),
                want_k=seen(kind, want_d, want_p, pages, sl, 0), want_v=seen(kind, want_d, want_p, pages, sl, 1))


def check(c, q_rot, k_seen, v_seen, what):
    torch.cuda.synchronize()
    got_d, got_p = host(c["data"], c["param"])
    assert np.array_equal(bits(q_rot), c["want_q"]), f"{what}: q differs from the oracle"
    assert np.array_equal(got_d, c["want_cache"][0]), f"{what}: {int((got_d != c['want_cache'][0]).sum())} cache bytes differ from the oracle"
    assert got_p is None or np.array_equal(got_p.view(np.uint16), c["want_cache"][1].view(np.uint16)), f"{what}: params differ"
    assert np.array_equal(bits(k_seen), c["want_k"]), f"{what}: k_seen is not what the slot reads back"
    assert np.array_equal(bits(v_seen).reshape(c["want_v"].shape), c["want_v"]), f"{what}: v_seen is not what the slot reads back"


def split(T):
    """T new tokens over four sequences holding 3, 0, 15 and 20: one appends nothing, the third crosses a page edge from 2 tokens on"""
    return [3, 0, 15, 20], [T // 3, 0, T - T // 3 - T // 4, T // 4]


def tables_of(table, T):
    one, zero = np.full((T, 128), 0x3F80, np.uint16), np.zeros((T, 128), np.uint16)
    half = np.concatenate([zero[:, :64], one[:, :64]], axis=1)                 # cos = (0, 1), sin = (1, 0): a table that repeats nothing
    return {"identity": (one, zero), "halves differ": (half, half ^ np.uint16(0x3F80)), "strided": ro.llama3_tables(np.arange(T)[::-1] * 997)}.get(table)


@pytest.mark.parametrize("P,table", [(1, "llama3"), (16, "llama3"), (24, "llama3"), (16, "identity"), (16, "halves differ"), (16, "strided")])
@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (5, 1)])
@pytest.mark.parametrize("kind", KINDS)
def test_outputs_against_the_oracles(dev, kind, heads, P, table):
    rng = np.random.default_rng(heads[0] * 100 + P)
    for T in (1, TPW - 1, TPW, TPW + 1, 2 * TPW + 3):
        c = case(kind, *heads, P, *split(T), rng, dev, tables=tables_of(table, T))
        if table == "strided":
            both = torch.cat([c["cos"], c["sin"]], dim=1)                      # rows of one [T, 256] tensor, in HF's [1, T, 128] shape
            c["cos"], c["sin"] = both[:, :128].unsqueeze(0), both[:, 128:].unsqueeze(0)
        out = mixedgemm.rope_kv_append_dense(c["data"], c["param"], *c["tbl"], c["q"], c["k"], c["v"], c["cos"], c["sin"], c["app"], LAYER)
        check(c, *out, f"T = {T}")
        assert (out[2] is c["v"]) == (kind == "bf16")
        assert table != "identity" or np.array_equal(bits(out[0]).reshape(T, -1), bits(c["q"])), "q did not pass through"


@pytest.mark.parametrize("kind", KINDS)
def test_against_the_old_kernel(dev, kind):
    c = case(kind, 8, 2, 16, *split(2 * TPW + 3), np.random.default_rng(6), dev)
    old_d, old_p = poisoned(kind, c["data"].size(0), 2, 16, dev)
    q_old = mixedgemm.rope_kv_append(old_d, old_p, *c["tbl"], c["q"], c["k"], c["v"], c["cos"], c["sin"], c["app"], LAYER)
    q_new = mixedgemm.rope_kv_append_dense(c["data"], c["param"], *c["tbl"], c["q"], c["k"], c["v"], c["cos"], c["sin"], c["app"], LAYER)[0]
    assert torch.equal(q_old.view(torch.int16), q_new.view(torch.int16))
    assert torch.equal(old_d.view(torch.uint8), c["data"].view(torch.uint8)) and (old_p is None or torch.equal(old_p.view(torch.int16), c["param"].view(torch.int16)))


def raw(dev, c, heads, kv_heads, outs, cache=False, **change):
    """mm_rope_prefill itself on the tensors of a case, with the outputs given (None: NULL); returns the status"""
    a = dict.fromkeys(ARGS, 0)
    if cache:
        kind, max_pages, _, _, P, data = mixedgemm._kv_geometry(c["data"], c["param"], dev.index)
        a.update(kv_data=data.data_ptr(), kv_param=c["param"].data_ptr() if c["param"] is not None else None, kv_dtype=kind, max_pages=max_pages,
                 L=L, layer=LAYER, P=P, kv_indptr=c["tbl"][0].data_ptr(), kv_indices=c["tbl"][1].data_ptr(), last=c["tbl"][2].data_ptr(),
                 B=c["tbl"][2].numel(), app=c["app"].data_ptr())
    a.update(Hkv=kv_heads, hd=128, q=c["q"].data_ptr(), k=c["k"].data_ptr(), v=c["v"].data_ptr(), sq=c["buf"].stride(0), Hq=heads, cos=c["cos"].data_ptr(),
             sin=c["sin"].data_ptr(), sc=128, T=c["T"], **{n: (t.data_ptr() if t is not None else None) for n, t in zip(ARGS[-3:], outs)})
    a.update(change)
    st = _lib.load().mm_rope_prefill(*[(a[n] or None) if n in POINTERS else a[n] for n in ARGS], _stream_ptr(dev))
    torch.cuda.synchronize()
    return st


def guarded(T, heads, dev):
    """three outputs inside one sentinel-filled buffer, 64 elements of guard around each"""
    n = [T * h * 128 for h in heads]
    whole = torch.full((sum(n) + 64 * 4,), SENTINEL, dtype=torch.int16, device=dev)
    starts = [64, 128 + n[0], 192 + n[0] + n[1]]
    return whole, [whole[s: s + m].view(torch.bfloat16).view(T, h, 128) for s, m, h in zip(starts, n, heads)]


def test_no_cache_form(dev):
    Hq, Hkv, T = 8, 2, 2 * TPW + 3
    c = case("bf16", Hq, Hkv, 16, *split(T), np.random.default_rng(7), dev)
    want_k = ro.rope(bits(c["k"]).reshape(T, Hkv, 128), bits(c["cos"]), bits(c["sin"]))
    for q, k in ((c["q"], c["k"]), (c["q"].reshape(T, Hq, 128).contiguous(), c["k"].contiguous())):     # views of the projection, then copies
        q_rot, k_rot = mixedgemm.rope_qk(q, k, c["cos"], c["sin"])
        assert np.array_equal(bits(q_rot), c["want_q"]) and np.array_equal(bits(k_rot), want_k)
    for nulls in ((), (2,), (1, 2)):
        whole, outs = guarded(T, (Hq, Hkv, Hkv), dev)
        assert raw(dev, c, Hq, Hkv, [None if i in nulls else o for i, o in enumerate(outs)]) == _lib.MM_OK
        want = [c["want_q"], want_k, bits(c["v"]).reshape(T, Hkv, 128)]
        for i, o in enumerate(outs):
            assert np.array_equal(bits(o), np.full_like(want[i], SENTINEL) if i in nulls else want[i]), (nulls, i)
        assert int((whole == SENTINEL).sum()) == 256 + sum(outs[i].numel() for i in nulls), "memory next to an output was written"
    assert torch.equal(c["data"].view(torch.int16), torch.full_like(c["data"].view(torch.int16), SENTINEL)), "no cache was given"


def attention_fp64(q_bits, k_bits, v_bits, lens):
    """plain causal GQA attention per sequence in fp64, and max|V| over the attended tokens"""
    q, k, v = (ko.bf16_to_f32(x).astype(np.float64) for x in (q_bits, k_bits, v_bits))
    g, o, vm, a0 = q.shape[1] // k.shape[1], np.zeros(q.shape), np.zeros(q.shape[:2] + (1,)), 0
    for n in filter(None, lens):
        for h in range(q.shape[1]):
            s = np.where(np.tri(n, dtype=bool), q[a0:a0 + n, h] @ k[a0:a0 + n, h // g].T * 128 ** -0.5, -np.inf)
            p = np.exp(s - s.max(-1, keepdims=True))
            o[a0:a0 + n, h] = p @ v[a0:a0 + n, h // g] / p.sum(-1, keepdims=True)
            vm[a0:a0 + n, h, 0] = np.maximum.accumulate(np.abs(v[a0:a0 + n, h // g]).max(-1))
        a0 += n
    return o, vm


@pytest.mark.parametrize("kind", KINDS)
def test_prefill_fresh(dev, kind):
    rng = np.random.default_rng(8)
    lens, Hq, Hkv = [0, 1, 63, 64, 65, 129], 8, 2
    T = sum(lens)
    buf = torch.from_numpy(rng.standard_normal((T, (Hq + 2 * Hkv) * 128)).astype(np.float32)).to(torch.bfloat16).to(dev)
    q, k, v = buf[:, : Hq * 128], buf[:, Hq * 128: (Hq + Hkv) * 128], buf[:, (Hq + Hkv) * 128:]
    cos, sin = (from_bits(t, dev) for t in ro.llama3_tables(np.concatenate([np.arange(n) for n in lens])))
    a, b, c = (PagedKVCache(L, Hkv, 16, 32, len(lens), kind=kind, device=dev) for _ in range(3))
    a.extend(lens), b.extend(lens), c.extend(lens)
    o = a.prefill_fresh(LAYER, q, k, v, cos, sin)
    q_rot, k_seen, v_seen = b.append_rope(LAYER, q, k, v, cos, sin, dense=True)
    torch.cuda.synchronize()
    assert torch.equal(a.kv_data.view(torch.uint8), b.kv_data.view(torch.uint8))
    if kind != "int4":                                                         # the oracle reads the cache itself: exactly bf16 numbers
        data, param = host(b.kv_data, b.kv_param)
        tbl = [t.cpu().numpy() for t in (b.kv_indptr, b.kv_indices)]
        pages, sl = (np.concatenate(c) for c in zip(*[ko.slots(*tbl, 16, s, np.arange(n)) for s, n in enumerate(lens) if n]))
        k_ref, v_ref = (seen(kind, data, param, pages, sl, w) for w in (0, 1))
    else:                                                                      # the returned tensors, checked bit for bit above
        k_ref, v_ref = bits(k_seen), bits(v_seen)
    want, vmax = attention_fp64(bits(q_rot), k_ref, v_ref.reshape(T, Hkv, 128), lens)
    err = np.abs(o.float().cpu().numpy().astype(np.float64) - want)
    bound = 2 * 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-30))) - 7) + 2.0 ** -8 * vmax
    print(f"{kind}: worst err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), f"{int((err > bound).sum())} outputs outside 2 ulp + 2^-8 max|V|; worst err / bound {(err / bound).max():.3f}"
    c.append_rope(LAYER, q, k, v, cos, sin)                                    # one decode step afterwards: the cache is append_rope()'s
    step = torch.from_numpy(rng.standard_normal((len(lens), (Hq + 2 * Hkv) * 128)).astype(np.float32)).to(torch.bfloat16).to(dev)
    parts = step[:, : Hq * 128], step[:, Hq * 128: (Hq + Hkv) * 128], step[:, (Hq + Hkv) * 128:]
    tabs = [from_bits(t, dev) for t in ro.llama3_tables(lens)]
    a.extend(1), c.extend(1)
    res = [cache.attend(LAYER, cache.append_rope(LAYER, *parts, *tabs)) for cache in (a, c)]
    assert torch.equal(res[0].view(torch.int16), res[1].view(torch.int16))
    with pytest.raises(ValueError, match="attend_new"):                        # every sequence holds tokens now
        a.prefill_fresh(LAYER, *parts, *tabs)
    w = PagedKVCache(L, Hkv, 16, 32, len(lens), kind=kind, device=dev, window=64)
    w.extend(lens)
    with pytest.raises(ValueError, match="attend_new"):
        w.prefill_fresh(LAYER, q, k, v, cos, sin)


def test_graph_replay_with_another_split(dev):
    rng = np.random.default_rng(9)
    Hq, Hkv, T = 8, 2, 40
    buf = torch.zeros((T, (Hq + 2 * Hkv) * 128), dtype=torch.bfloat16, device=dev)
    q, k, v = buf[:, : Hq * 128], buf[:, Hq * 128: (Hq + Hkv) * 128], buf[:, (Hq + Hkv) * 128:]
    cos, sin = (from_bits(t, dev) for t in ro.llama3_tables(np.arange(T)))
    cache = PagedKVCache(L, Hkv, 16, 16, 3, kind="int4", device=dev)
    cache.extend([10, 0, 30])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cache.prefill_fresh(LAYER, q, k, v, cos, sin)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = cache.prefill_fresh(LAYER, q, k, v, cos, sin)
    for counts in ([10, 0, 30], [25, 15, 0], [1, 38, 1]):
        for b in range(3):
            cache.reset(b)
        cache.extend(counts)
        buf.copy_(torch.from_numpy(rng.standard_normal(tuple(buf.shape)).astype(np.float32)).to(torch.bfloat16))
        graph.replay()
        torch.cuda.synchronize()
        got, got_cache = out.clone(), host(cache.kv_data, cache.kv_param)
        eager = cache.prefill_fresh(LAYER, q, k, v, cos, sin)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), eager.view(torch.int16)), f"{counts}: the replay differs from the eager call"
        assert all(np.array_equal(x, y) for x, y in zip(got_cache, host(cache.kv_data, cache.kv_param))), f"{counts}: the caches differ"


BAD, UNSUP = "MM_ERR_BAD_ARG", "MM_ERR_UNSUPPORTED"
REFUSED = [(dict(T=-1), BAD), (dict(Hq=0), BAD), (dict(Hq=7), BAD), (dict(sq=8 * 128 - 8), BAD), (dict(sq=12 * 128 + 4), BAD), (dict(sc=120), BAD),
           (dict(sc=132), BAD), (dict(hd=64), UNSUP), (dict(q=0), BAD), (dict(cos=0), BAD), (dict(q_out=0), BAD), (dict(k="+8"), BAD),
           (dict(k_out="+8"), BAD), (dict(kv_dtype=2), BAD), (dict(layer=L), BAD), (dict(B=0), BAD), (dict(app=0), BAD), (dict(kv_param=0), BAD),
           (dict(kv_data="+8"), BAD), (dict(last=0), BAD)]


@pytest.mark.parametrize("change,status", REFUSED, ids=[str(c) for c, _ in REFUSED])
def test_statuses(dev, change, status):
    Hq, Hkv, T = 8, 2, TPW + 1
    c = case("int4", Hq, Hkv, 16, *split(T), np.random.default_rng(10), dev)
    whole, outs = guarded(T, (Hq, Hkv, Hkv), dev)
    base = dict(k=c["k"].data_ptr(), k_out=outs[1].data_ptr(), kv_data=c["data"].data_ptr())
    change = {n: base[n] + int(x) if isinstance(x, str) else x for n, x in change.items()}
    clean = host(c["data"], c["param"])
    assert raw(dev, c, Hq, Hkv, outs, cache=True, **change) == getattr(_lib, status)
    assert bool((whole == SENTINEL).all()) and all(np.array_equal(x, y) for x, y in zip(clean, host(c["data"], c["param"]))), "a refused call wrote"
    assert raw(dev, c, Hq, Hkv, outs, cache=True, T=0) == _lib.MM_OK and bool((whole == SENTINEL).all())
