"""GPU tests of causal multi-token attention over the paged cache for 64-wide heads (include/micromix_kv_prefill_hd64.h) through
mixedgemm.paged_prefill and PagedKVCache(head_dim=64).attend_new, against an fp64 reference of a few lines."""
import functools

import numpy as np
import pytest
import torch

import kv_fp8_oracle as kf
import kv_oracle as ko
from micromix_amd import mixedgemm
from micromix_amd.kvcache import PagedKVCache
from test_kv_hd64_gpu import DEV, KINDS, bf16_ulp, bits, from_bits, gather, gauss_bits, make_cache, step_inputs, table

pytestmark = pytest.mark.gpu
HEADS = ((4, 4), (8, 2), (14, 2), (16, 1))            # g = 1, 4, 7, 16


def causal_fp64(q, k, v, pos, scale):
    """o [n, Hq, 64] and, per query, max |V| over what it attends: query i at position pos[i] attends tokens 0 .. pos[i] (none below 0)"""
    g = q.shape[1] // k.shape[1]
    s = np.einsum("ihd,thd->hit", q, np.repeat(k, g, axis=1)) * scale
    s = np.where(np.arange(k.shape[0])[None, :] <= pos[:, None], s, -np.inf)
    p = np.exp(s - np.maximum(s.max(-1, keepdims=True), -1e300))
    o = np.einsum("hit,thd->ihd", p / np.maximum(p.sum(-1, keepdims=True), 1e-300), np.repeat(v, g, axis=1))
    vmax = np.maximum.accumulate(np.abs(v).max(axis=(1, 2)))[np.maximum(pos, 0)] * (pos >= 0)
    return o, vmax


def reference(q_bits, seen, tbl, P, layer, qo, scale=0.125):
    q = ko.bf16_to_f32(q_bits).astype(np.float64)
    o, vmax = np.zeros(q.shape), np.zeros(q.shape[0])
    for b, n in enumerate(ko.seq_lens(tbl[0], tbl[2], P)):
        new = qo[b + 1] - qo[b]
        if n and new:
            k, v = gather(seen, tbl[0], tbl[1], P, layer, b, n)
            o[qo[b]: qo[b + 1]], vmax[qo[b]: qo[b + 1]] = causal_fp64(q[qo[b]: qo[b + 1]], k, v, n - new + np.arange(new), scale)
    return o, vmax


def fraction(o, ref, vmax):           # the largest |o - ref| as a fraction of DESIGN 7c's bound: 2 bf16 ulps + 2^-8 max|V| over the attended tokens
    err = np.abs(ko.bf16_to_f32(bits(o)).astype(np.float64) - ref)
    return float((err / (2 * bf16_ulp(ref) + 2.0 ** -8 * vmax[:, None, None] + 1e-300)).max())


def prefill(q, data, param, tbl, qo, layer, bound):
    return mixedgemm.paged_prefill(q, data, param, *(torch.from_numpy(a).to(DEV) for a in tbl[:3]), torch.from_numpy(qo).to(DEV), layer, bound)


@functools.lru_cache(maxsize=None)
def case(kind, Hq, Hkv, P, rows):
    """one call whose (prior, new) pairs sit on both sides of every edge of the plan's tile of `rows` rows; made once, left unchanged"""
    bq = rows // (Hq // Hkv)
    news = [0, 1, bq - 1, bq, bq + 1, 2 * bq + 1]
    pairs = list(zip([0, 1, 63, 64, 65, 200], news)) + list(zip([200, 65, 64, 63, 1, 0], news))
    lens, qo = [p + n for p, n in pairs], np.concatenate([[0], np.cumsum([n for _, n in pairs])]).astype(np.int32)
    rng = np.random.default_rng(Hq + P)
    tbl = table(lens, P, rng)
    data, param, seen = make_cache(kind, gauss_bits(rng, (tbl[3], 2, 2, Hkv, P, 64)))
    q_bits = gauss_bits(rng, (int(qo[-1]), Hq, 64), 2.0)
    tight, loose = max(lens), 4096
    plans = [mixedgemm.paged_prefill_hd64_plan(int(qo[-1]), len(lens), Hq, Hkv, bound) for bound in (tight, loose)]
    assert all(p.rows == rows and p.tile_tokens == bq for p in plans) and plans[1].chunks > 1
    return tbl, qo, data, param, seen, q_bits, (tight, loose), reference(q_bits, seen, tbl, P, 1, qo)


SHAPES = [(Hq, Hkv, P, rows) for Hq, Hkv in HEADS for P in (1, 16) for rows in (128, 64)]


@pytest.mark.parametrize("Hq,Hkv,P,rows", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_against_fp64(kind, Hq, Hkv, P, rows):
    """worst fraction of the bound observed: see DESIGN 7ab"""
    tbl, qo, data, param, _, q_bits, bounds, (ref, vmax) = case(kind, Hq, Hkv, P, rows)
    for bound in bounds:
        o = prefill(from_bits(q_bits), data, param, tbl, qo, 1, bound)
        frac = fraction(o, ref, vmax)
        print(f"kv_prefill_hd64 {kind} Hq={Hq} Hkv={Hkv} P={P} rows={rows} bound={bound}: worst fraction of the bound {frac:.3f}")
        assert frac <= 1.0


@pytest.mark.parametrize("Hq,Hkv,P,rows", SHAPES)
def test_fp8_is_bf16_on_the_dequantized_values(Hq, Hkv, P, rows):
    tbl, qo, data, param, seen, q_bits, bounds, _ = case("fp8_e4m3", Hq, Hkv, P, rows)
    for bound in bounds:
        assert torch.equal(prefill(from_bits(q_bits), data, param, tbl, qo, 1, bound), prefill(from_bits(q_bits), from_bits(seen), None, tbl, qo, 1, bound))


def counting_cache(kind, lens, tbl, Hkv, P):
    """V[t] = e_(t mod 64) on the slots the sequences hold, K Gaussian there, NaN in every other slot of every page"""
    rng = np.random.default_rng(3)
    vals, held = gauss_bits(rng, (tbl[3], 1, 2, Hkv, P, 64)), np.zeros((tbl[3], 1, 2, Hkv, P), dtype=bool)
    one = bits(torch.tensor([1.0], dtype=torch.bfloat16))[0]
    for b, n in enumerate(lens):
        pages, sl = ko.slots(tbl[0], tbl[1], P, b, np.arange(n))
        rows = np.zeros((n, Hkv, 64), dtype=np.uint16)
        rows[np.arange(n), :, np.arange(n) % 64] = one
        vals[pages, 0, 1, :, sl], held[pages, :, :, :, sl] = rows, True
    data, param, _ = make_cache(kind, vals)
    free = torch.from_numpy(~held).to(DEV)
    if param is None:
        data[free] = float("nan")
    else:
        data.view(torch.uint8)[free], param[free] = 0x7F, float("nan")
    return data, param


@pytest.mark.parametrize("few", [False, True], ids=["rows128", "rows64"])
@pytest.mark.parametrize("kind", KINDS)
def test_exact_counts(kind, few):
    """q = 0: round(o[d] * (p + 1)) is the number of positions <= p congruent to d mod 64, at every p of one 2048-token prompt (every
    tile edge, both sides of every chunk edge), or -- the 64-row kernel -- at one new token behind each edge; no NaN gets in"""
    Hq, Hkv, P = 8, 2, 16
    edges = sorted({e + s for e in range(64, 2048, 64) for s in (-1, 0, 1)} | {1, 2047, 2048})
    lens, news = ([2048], [2048]) if not few else (edges, [1] * len(edges))
    qo = np.concatenate([[0], np.cumsum(news)]).astype(np.int32)
    tbl = table(lens, P, np.random.default_rng(9), spare=4)
    data, param = counting_cache(kind, lens, tbl, Hkv, P)
    pos = np.concatenate([n - new + np.arange(new) for n, new in zip(lens, news)])
    want = np.stack([np.bincount(np.arange(p + 1) % 64, minlength=64) for p in pos])
    q = torch.zeros((int(qo[-1]), Hq, 64), dtype=torch.bfloat16, device=DEV)
    for bound in (256, 2048):
        plan = mixedgemm.paged_prefill_hd64_plan(int(qo[-1]), len(lens), Hq, Hkv, bound)
        assert plan.rows == (64 if few else 128) and (plan.chunks > 1) == (bound == 2048) and plan.chunk_len % 64 == 0   # chunk edges are tile edges
        o = ko.bf16_to_f32(bits(prefill(q, data, param, tbl, qo, 0, bound))).astype(np.float64)
        assert not np.isnan(o).any()
        assert np.array_equal(np.rint(o * (pos + 1)[:, None, None]), np.broadcast_to(want[:, None, :], o.shape)), bound


@pytest.mark.parametrize("kind", KINDS)
def test_one_token_agrees_with_decode(kind):
    """n_b = 1 everywhere: paged_decode's function, within the sum of the two kernels' bounds (decode never rounds p: not the same bits)"""
    Hq, Hkv, P, lens = 8, 2, 16, [1, 63, 64, 65, 255, 256, 257, 1300]
    rng = np.random.default_rng(17)
    tbl = table(lens, P, rng)
    data, param, seen = make_cache(kind, gauss_bits(rng, (tbl[3], 1, 2, Hkv, P, 64)))
    q = from_bits(gauss_bits(rng, (len(lens), Hq, 64), 2.0))
    qo = np.arange(len(lens) + 1, dtype=np.int32)
    vmax = np.array([np.abs(gather(seen, tbl[0], tbl[1], P, 0, b, n)[1]).max() for b, n in enumerate(lens)])[:, None, None]
    for bound in (256, 1300):
        a = ko.bf16_to_f32(bits(prefill(q, data, param, tbl, qo, 0, bound))).astype(np.float64)
        d = ko.bf16_to_f32(bits(mixedgemm.paged_decode(q, data, param, *(torch.from_numpy(x).to(DEV) for x in tbl[:3]), 0, bound))).astype(np.float64)
        assert (np.abs(a - d) <= 2 * bf16_ulp(d) + 2.0 ** -8 * vmax + np.maximum(2 * bf16_ulp(d), 1e-3 * vmax)).all()


@pytest.mark.parametrize("kind", KINDS)
def test_cache_chunked_prompt_and_graph_replay(kind):
    """a 256-token prompt as 100 / 100 / 56 through extend -> append_rope -> attend_new against fp64 over the whole prompt; then one hipGraph
    of append_rope + attend_new under a bound, replayed over three extend(5) steps, each bit-equal to eager"""
    rng, Hq, Hkv, P, bound = np.random.default_rng(23), 8, 2, 16, 1024
    cache = PagedKVCache(num_layers=1, num_kv_heads=Hkv, page_size=P, max_pages=40, batch=1, kind=kind, device=DEV, head_dim=64)
    q_rot, o = [], []
    for n in (100, 100, 56):
        cache.extend([n])
        q_rot.append(cache.append_rope(0, *step_inputs(rng, n, Hq, Hkv)))
        o.append(cache.attend_new(0, q_rot[-1]))
    raw = cache.kv_data.view(torch.uint8).cpu().numpy() if kind != "bf16" else bits(cache.kv_data)
    seen = raw if kind == "bf16" else kf.dequantize(raw, cache.kv_param.cpu().numpy())
    k, v = gather(seen, cache.kv_indptr.cpu().numpy(), cache.kv_indices.cpu().numpy(), P, 0, 0, 256)
    ref, vmax = causal_fp64(ko.bf16_to_f32(bits(torch.cat(q_rot))).astype(np.float64), k, v, np.arange(256), 0.125)
    assert fraction(torch.cat(o), ref, vmax) <= 1.0
    cache.extend([5])
    static = step_inputs(rng, 5, Hq, Hkv)
    cache.attend_new(0, cache.append_rope(0, *static), max_seq_len=bound)             # warm: the workspace exists before the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = cache.attend_new(0, cache.append_rope(0, *static), max_seq_len=bound)
    assert mixedgemm.paged_prefill_hd64_workspace_bytes(5, 1, Hq, Hkv, bound) > 0    # the replayed graph holds the merge launch too
    for _ in range(3):
        cache.extend([5])
        for dst, src in zip(static, step_inputs(rng, 5, Hq, Hkv)):
            dst.copy_(src)
        graph.replay()
        assert torch.equal(out.clone(), cache.attend_new(0, cache.append_rope(0, *static), max_seq_len=bound))
