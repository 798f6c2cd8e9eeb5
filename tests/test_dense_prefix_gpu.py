"""GPU tests of dense attention over a cached prefix: mixedgemm.kv_gather_dense (include/micromix_kvgather.h), dense_attention_prefix
(include/micromix_attention_prefix.h) and PagedKVCache.attend_new_dense, against a plain fp64 reference over the bf16 inputs and the
cache oracles.  The shapes stand on the edges of the query tile, the kv tile and the chunks the plan reports."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd._args import _stream_ptr
from micromix_amd.kvcache import PagedKVCache
from conftest import bits_from_t as nbits, t_from_bits as from_bits
from test_dense_attention_gpu import bits, f64, indptr_of, rand_bf16
from test_rope_prefill_gpu import KINDS, LAYER, L, host, poisoned, seen
import kv_fp8_oracle as fo
import kv_oracle as ko
import rope_oracle as ro

pytestmark = pytest.mark.gpu
prefix, plan = mixedgemm.dense_attention_prefix, mixedgemm.dense_attention_prefix_plan
PAIRS = [(0, 0), (0, 50), (1, 1), (1, 200), (5, 64), (64, 65), (65, 129), (127, 128), (128, 323), (129, 129), (130, 700), (3, 2)]
SENTINEL = 0x5A5A


def nan_workspace(Tq, B, Hq, bound, dev):
    need = mixedgemm.dense_attention_prefix_workspace_bytes(Tq, B, Hq, bound)
    return torch.full((need // 4,), float("nan"), dtype=torch.float32, device=dev) if need else None


def reference(q, k, v, pairs, sm_scale=128 ** -0.5):
    """fp64 bottom-right causal GQA attention over the bf16 values (an empty range gives zeros); max |V| over the tokens each output attends"""
    q, k, v = f64(q), f64(k), f64(v)
    g, o, vmax, q0, k0 = q.shape[1] // k.shape[1], np.zeros(q.shape), np.zeros(q.shape[:2] + (1,)), 0, 0
    for nq, nk in pairs:
        last = nk - nq + np.arange(nq)                                     # the last key each query attends
        live = last >= 0
        for h in range(q.shape[1] if live.any() else 0):
            s = q[q0:q0 + nq, h] @ k[k0:k0 + nk, h // g].T * sm_scale
            s[np.arange(nk)[None, :] > last[:, None]] = -np.inf
            p = np.exp(s[live] - s[live].max(axis=1, keepdims=True))
            o[q0:q0 + nq, h][live] = p @ v[k0:k0 + nk, h // g] / p.sum(axis=1, keepdims=True)
            vmax[q0:q0 + nq, h, 0][live] = np.maximum.accumulate(np.abs(v[k0:k0 + nk, h // g]).max(axis=1))[last[live]]
        q0, k0 = q0 + nq, k0 + nk
    return o, vmax


def within_bound(o, want, vmax, what):
    """the project's bound: |o - ref| <= 2 bf16 ulp(ref) + 2^-8 max|V| over the attended tokens"""
    got = f64(o)
    err, ulp = np.abs(got - want), 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-30))) - 7)
    bound = 2 * ulp + 2.0 ** -8 * vmax
    print(f"{what}: worst err {err.max():.3e}, worst err / bound {(err / np.maximum(bound, 1e-30))[bound > 0].max():.3f}")
    assert np.isfinite(got).all() and not (err > bound).any(), f"{what}: {int((err > bound).sum())} outputs outside the bound"


@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2), (5, 1), (32, 8)])
def test_against_fp64(dev, Hq, Hkv):
    """the issue's three head counts split the kv tokens; (32, 8) fills the device without, so it runs the shifted diagonal and the
    empty rows through the kernel's own epilogue (nc == 1)"""
    rng = np.random.default_rng(Hq * 100 + Hkv)
    Tq, Tk, longest = sum(a for a, _ in PAIRS), sum(b for _, b in PAIRS), max(b for _, b in PAIRS)
    q, k, v = rand_bf16((Tq, Hq, 128), rng, dev, 2.0), rand_bf16((Tk, Hkv, 128), rng, dev), rand_bf16((Tk, Hkv, 128), rng, dev, 0.5)
    qo, kvp = indptr_of([a for a, _ in PAIRS], dev), indptr_of([b for _, b in PAIRS], dev)
    want, vmax = reference(q, k, v, PAIRS)
    assert (max(plan(Tq, len(PAIRS), Hq, bound)[0] for bound in (longest, 5 * longest)) > 1) == (Hq < 32), "the split is not the one this case is for"
    for bound in (longest, 5 * longest):
        o = prefix(q, k, v, qo, kvp, bound, workspace=nan_workspace(Tq, len(PAIRS), Hq, bound, dev))
        within_bound(o, want, vmax, f"Hq {Hq} Hkv {Hkv} bound {bound} plan {plan(Tq, len(PAIRS), Hq, bound)}")
        assert not o[Tq - 3].float().any(), "a query that attends nothing must give zeros"


def test_square_has_dense_attention_bits(dev):
    Hq, Hkv, lens = 8, 2, [129, 64, 1, 200]
    T = sum(lens)
    assert plan(T, len(lens), Hq, max(lens))[0] == 1
    packed = rand_bf16((T, (Hq + 2 * Hkv) * 128), np.random.default_rng(3), dev)
    q, k, v = packed[:, :Hq * 128], packed[:, Hq * 128:(Hq + Hkv) * 128], packed[:, (Hq + Hkv) * 128:]
    ip = indptr_of(lens, dev)
    want = mixedgemm.dense_attention(q, k, v, ip)
    assert torch.equal(bits(prefix(q, k, v, ip, ip, max(lens))), bits(want)), "views"
    assert torch.equal(bits(prefix(q.contiguous(), k.contiguous(), v.contiguous(), ip, ip, max(lens))), bits(want)), "copies"


NQ, NK = 130, 700
CHUNK = 256          # what the plan gives for this shape; the test asserts it


@pytest.mark.parametrize("m", [0, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 569, 570, 700])
def test_exact_count_across_chunks(dev, m):
    """q = 0 makes the softmax uniform; V is 1 below token m and 0 from there: o[i] = min(off + i + 1, m) / (off + i + 1) to 1 bf16 ulp"""
    Hq, Hkv = 4, 2
    assert plan(NQ, 1, Hq, NK) == (3, CHUNK)
    q, k = torch.zeros((NQ, Hq, 128), dtype=torch.bfloat16, device=dev), rand_bf16((NK, Hkv, 128), np.random.default_rng(m), dev)
    v = (torch.arange(NK, device=dev) < m).to(torch.bfloat16)[:, None, None].expand(NK, Hkv, 128).contiguous()
    o = f64(prefix(q, k, v, None, None, NK, workspace=nan_workspace(NQ, 1, Hq, NK, dev)))
    seen_keys = NK - NQ + 1 + np.arange(NQ, dtype=np.float64)
    want = (np.minimum(seen_keys, m) / seen_keys)[:, None, None]
    bad = np.abs(o - want) > 2.0 ** (np.floor(np.log2(np.maximum(want, 1e-30))) - 7)
    assert not bad.any(), f"first wrong (token, head, dim): {np.argwhere(bad)[0]}, got {o[bad][0]}"


def test_isolation(dev):
    """NaN in the neighbours' K / V and in kv rows no sequence owns changes no bit; output rows no sequence owns keep a sentinel"""
    Hq, Hkv, pairs, pad = 8, 2, [(70, 300), (130, 700), (64, 64)], 5
    rng = np.random.default_rng(5)
    qo = torch.tensor(np.cumsum([pad] + [a for a, _ in pairs]), dtype=torch.int32, device=dev)
    kvp = torch.tensor(np.cumsum([pad] + [b for _, b in pairs]), dtype=torch.int32, device=dev)
    Tq, Tk = int(qo[-1]) + pad, int(kvp[-1]) + pad
    q, k, v = rand_bf16((Tq, Hq, 128), rng, dev, 2.0), rand_bf16((Tk, Hkv, 128), rng, dev), rand_bf16((Tk, Hkv, 128), rng, dev)
    assert plan(Tq, 3, Hq, 700)[0] > 1
    ws, lib = nan_workspace(Tq, 3, Hq, 700, dev), _lib.load()

    def run(k, v):
        o = torch.full((Tq, Hq, 128), SENTINEL, dtype=torch.int16, device=dev).view(torch.bfloat16)
        assert lib.mm_dense_attention_prefix(q.data_ptr(), k.data_ptr(), v.data_ptr(), Hq * 128, Hkv * 128, Hkv * 128, qo.data_ptr(),
                                             kvp.data_ptr(), 3, Tq, Tk, Hq, Hkv, 128, 700, 0.1, ws.data_ptr(), ws.numel() * 4, o.data_ptr(),
                                             _stream_ptr(dev)) == _lib.MM_OK
        return bits(o)

    a, b = int(kvp[1]), int(kvp[2])
    k2, v2 = k.clone(), v.clone()
    for t in (k2, v2):
        t[:a], t[b:] = float("nan"), float("nan")
    o, o2 = run(k, v), run(k2, v2)
    lo, hi = int(qo[1]), int(qo[2])
    assert torch.equal(o[lo:hi], o2[lo:hi]) and (o[:pad] == SENTINEL).all() and (o[-pad:] == SENTINEL).all()
    assert torch.isfinite(o[pad:-pad].view(torch.bfloat16).float()).all()


@pytest.mark.parametrize("P", [1, 16, 24])
@pytest.mark.parametrize("kind", KINDS)
def test_gather_against_the_oracles(dev, kind, P):
    """every row of k_out / v_out is what the oracle's cache reads back at that slot, or the sentinel it held"""
    Hkv, rng = 2, np.random.default_rng(P)
    lens = [0, 1, P - 1, P, P + 1, 3 * P + 5]
    npg = [-(-n // P) for n in lens]
    indptr, indices = np.concatenate([[0], np.cumsum(npg)]).astype(np.int32), rng.permutation(sum(npg) + 3)[: sum(npg)].astype(np.int32)
    last = np.array([n - (c - 1) * P if c else 0 for n, c in zip(lens, npg)], dtype=np.int32)
    app = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    kb, vb = (nbits(rand_bf16((sum(lens), Hkv, 128), rng, "cpu", s)) for s in (1.0, 3.0))
    data, param = poisoned(kind, sum(npg) + 3, Hkv, P, dev)
    hd, hp = host(data, param)
    (fo if kind == "fp8_e4m3" else ko).append(hd, hp, indptr, indices, last, kb, vb, app, LAYER)
    data.copy_(torch.from_numpy(hd.view(np.int16) if kind == "bf16" else hd).view(data.dtype).to(dev))
    if param is not None:
        param.copy_(torch.from_numpy(hp).to(dev))
    gone = int(indptr[5]) + 1                                              # the second page of the longest sequence is released
    room = [n + 3 for n in lens]
    room[4] = lens[4] - 1                                                  # ... and the sequence before it has a row less than it holds
    out = np.concatenate([[2], 2 + np.cumsum(room)]).astype(np.int32)
    total = int(out[-1]) + 4                                               # a capacity larger than the sum
    want = np.full((2, total, Hkv, 128), SENTINEL, dtype=np.uint16)
    for b, n in enumerate(lens):
        pos = np.array([p for p in range(min(n, room[b])) if indptr[b] + p // P != gone], dtype=np.int64)
        if len(pos):
            pages, sl = ko.slots(indptr, indices, P, b, pos)
            for which in (0, 1):
                want[which, out[b] + pos] = seen(kind, hd, hp, pages, sl, which)
    indices[gone] = -1
    tbl = [torch.from_numpy(a).to(dev) for a in (indptr, indices, last, out)]
    k_out, v_out = (torch.full((total, Hkv, 128), SENTINEL, dtype=torch.int16, device=dev).view(torch.bfloat16) for _ in "kv")
    got = mixedgemm.kv_gather_dense(data, param, *tbl[:3], tbl[3], LAYER, total, k_out, v_out)
    assert got[0] is k_out and got[1] is v_out
    assert np.array_equal(nbits(k_out), want[0]) and np.array_equal(nbits(v_out), want[1])


@pytest.mark.parametrize("kind", KINDS)
def test_route_through_the_cache(dev, kind):
    """a 300-token prompt in chunks of 128 + 128 + 44 next to a sequence that holds 70 tokens; the third chunk also by graph replay"""
    Hq, Hkv, P, held, bound = 8, 2, 16, 70, 300
    rng = np.random.default_rng(17)
    assert plan(128, 2, Hq, bound) == plan(44, 2, Hq, bound) and plan(128, 2, Hq, bound)[0] > 1     # the replay runs the eager call's split
    cache, twin = (PagedKVCache(L, Hkv, P, 40, 2, kind=kind, device=dev) for _ in range(2))
    first = [rand_bf16((held, Hkv, 128), rng, dev) for _ in "kv"]
    for c in (cache, twin):
        c.extend([0, held])
        c.append(LAYER, *first)
    q_static, graph, done = torch.zeros((128, Hq, 128), dtype=torch.bfloat16, device=dev), torch.cuda.CUDAGraph(), 0
    for step, n in enumerate([128, 128, 44]):
        buf = rand_bf16((n, (Hq + 2 * Hkv) * 128), rng, dev)
        q, k, v = buf[:, :Hq * 128], buf[:, Hq * 128:(Hq + Hkv) * 128], buf[:, (Hq + Hkv) * 128:]
        cos, sin = (from_bits(t, dev) for t in ro.llama3_tables(np.arange(done, done + n)))
        for c in (cache, twin):
            c.extend([n, 0])
        q_rot, k_seen, v_seen = cache.append_rope(LAYER, q, k, v, cos, sin, dense=True)
        twin.attend_new(LAYER, twin.append_rope(LAYER, q, k, v, cos, sin))
        o = cache.attend_new_dense(LAYER, q_rot, max_seq_len=bound)
        done += n
        K, V = mixedgemm.kv_gather_dense(cache.kv_data, cache.kv_param, cache.kv_indptr, cache.kv_indices, cache.last_page_len,
                                         cache.gather_indptr, LAYER, done + held)
        assert torch.equal(bits(K[done - n:done]), bits(k_seen))
        assert torch.equal(bits(V[done - n:done]), bits(v_seen).reshape(n, Hkv, 128))       # bf16: v_seen is the [n, Hkv * 128] view given
        within_bound(o, *reference(q_rot, K, V, [(n, done), (0, held)]), f"{kind} chunk {step}")
        assert torch.equal(cache.kv_data.view(torch.uint8), twin.kv_data.view(torch.uint8))
        if step == 1:
            q_static.copy_(q_rot)
            with torch.cuda.graph(graph):
                o_static = cache.attend_new_dense(LAYER, q_static, max_seq_len=bound)
        if step == 2:
            q_static[:n].copy_(q_rot)
            for _ in range(3):
                graph.replay()
                assert torch.equal(bits(o_static[:n]), bits(o)), "a replay differs from the eager call"
    with pytest.raises(ValueError):
        cache.attend_new_dense(LAYER, q_rot, max_seq_len=done - 1)        # a bound below the longest sequence
    cache.step_launch(None, [3, 2], max_seq_len=done + 20)                # a device step announces tokens: gather_indptr is the host's
    q5, k5, v5 = rand_bf16((5, Hq, 128), rng, dev), rand_bf16((5, Hkv, 128), rng, dev), rand_bf16((5, Hkv, 128), rng, dev)
    cache.append(LAYER, k5, v5)
    with pytest.raises(ValueError):
        cache.attend_new_dense(LAYER, q5)
    cache.sync()                                                          # ... and is written again here, from the device's lengths
    o = cache.attend_new_dense(LAYER, q5)
    K, V = mixedgemm.kv_gather_dense(cache.kv_data, cache.kv_param, cache.kv_indptr, cache.kv_indices, cache.last_page_len,
                                     indptr_of([done + 3, held + 2], dev), LAYER, done + held + 5)
    within_bound(o, *reference(q5, K, V, [(3, done + 3), (2, held + 2)]), f"{kind} after a device step and sync()")
    with pytest.raises(ValueError):
        PagedKVCache(L, Hkv, P, 8, 1, kind=kind, device=dev, window=64).attend_new_dense(LAYER, q_rot)
