"""GPU tests of the paged KV cache for 64-wide heads (include/micromix_kv_hd64.h) through mixedgemm and PagedKVCache(head_dim=64)."""
import numpy as np
import pytest
import torch

import kv_fp8_oracle as kf
import kv_oracle as ko
from micromix_amd import mixedgemm
from micromix_amd.kvcache import PagedKVCache

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("bf16", "fp8_e4m3")
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1300)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(b, dev=DEV):
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16)).view(torch.bfloat16).to(dev)


def gauss_bits(rng, shape, scale=1.0):
    return bits(torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * scale).to(torch.bfloat16))


def table(lens, P, rng, spare=3):     # a page table over shuffled pages: (kv_indptr, kv_indices, last_page_len, max_pages)
    need = [-(-n // P) for n in lens]
    max_pages = sum(need) + spare
    indptr = np.concatenate([[0], np.cumsum(need)]).astype(np.int32)
    indices = rng.permutation(max_pages)[: sum(need)].astype(np.int32)
    last = np.array([n - (c - 1) * P if n else 0 for n, c in zip(lens, need)], dtype=np.int32)
    return indptr, indices, last, max_pages


def make_cache(kind, vals_bits):      # (kv_data, kv_param) holding bf16 bits [max_pages, L, 2, Hkv, P, 64], and what a reader gets back
    if kind == "bf16":
        return from_bits(vals_bits), None, vals_bits
    codes, e = kf.quantize_row(vals_bits)
    param = kf.param_pair(e)
    data = torch.from_numpy(codes.astype(np.uint8)).to(DEV).view(torch.float8_e4m3fn)
    return data, torch.from_numpy(param).to(DEV), kf.dequantize(codes.astype(np.uint8), param)


def gather(seen_bits, indptr, indices, P, layer, b, n):                     # K, V of sequence b as float64 [n, Hkv, 64]
    pages, sl = ko.slots(indptr, indices, P, b, np.arange(n))
    rows = ko.bf16_to_f32(seen_bits[pages, layer, :, :, sl]).astype(np.float64)        # [n, 2, Hkv, 64]
    return rows[:, 0], rows[:, 1]


def reference(q_bits, seen_bits, indptr, indices, last, P, layer, scale):   # fp64 decode attention: gather, repeat_kv, softmax
    q = ko.bf16_to_f32(q_bits).astype(np.float64)
    B, Hq, _ = q.shape
    o, vmax = np.zeros((B, Hq, 64)), np.zeros(B)
    for b, n in enumerate(ko.seq_lens(indptr, last, P)):
        if n:
            k, v = gather(seen_bits, indptr, indices, P, layer, b, n)
            g = Hq // k.shape[1]
            s = np.einsum("hd,thd->ht", q[b], np.repeat(k, g, axis=1)) * scale
            p = np.exp(s - s.max(-1, keepdims=True))
            o[b] = np.einsum("ht,thd->hd", p / p.sum(-1, keepdims=True), np.repeat(v, g, axis=1))
            vmax[b] = np.abs(v).max()
    return o, vmax


def bf16_ulp(x):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126))) - 7)


def worst(o, ref, vmax):              # the largest |o - ref| as a fraction of DESIGN 7b's bound: 2 bf16 ulps, or 1e-3 max|V|
    err = np.abs(ko.bf16_to_f32(bits(o)).astype(np.float64) - ref)
    return float((err / np.maximum(2 * bf16_ulp(ref), 1e-3 * vmax[:, None, None] + 1e-300)).max())


def decode(q, data, param, tbl, layer, bound, scale=None):
    return mixedgemm.paged_decode(q, data, param, *(torch.from_numpy(a).to(DEV) for a in tbl[:3]), layer, bound, sm_scale=scale)


def rope_cpu(x, cos, sin):                            # the header's element rule in torch-CPU bf16 arithmetic
    x, c, s = x.cpu(), cos.cpu()[:, None, :], sin.cpu()[:, None, :]
    return x * c + torch.cat([-x[..., 32:], x[..., :32]], dim=-1) * s


EDGE_ROWS = [np.zeros(64), np.full(64, -0.0), *(np.r_[448.0 * 2.0 ** k, np.zeros(63)] for k in (-14, 0, 15)),
             *(np.r_[450.0 * 2.0 ** k, np.ones(63)] for k in (-14, 0, 14)),          # the next bf16 above 448 * 2^k is 450 * 2^k
             np.full(64, 3.3895313892515355e38), np.full(64, 2.0 ** -130)]            # bf16 max, a bf16 subnormal


@pytest.mark.parametrize("P", [1, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_append_byte_for_byte(kind, P):
    rng = np.random.default_rng(P)
    held, counts, Hq, Hkv, L, layer = [0, 15, 16, 31], [0, 1, 17, 40], 4, 2, 2, 1
    lens, T = [h + c for h, c in zip(held, counts)], sum(counts)
    indptr, indices, last, max_pages = table(lens, P, rng)
    app = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    qkv = from_bits(gauss_bits(rng, (T, (Hq + 2 * Hkv) * 64)))
    q, k, v = (qkv[:, a * 64: b * 64].view(T, -1, 64) for a, b in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv)))
    edge = torch.tensor(np.stack(EDGE_ROWS), dtype=torch.float32).to(torch.bfloat16).to(DEV)
    k[: len(EDGE_ROWS), 0], v[T - len(EDGE_ROWS):, 1] = edge, edge
    ang = torch.from_numpy(rng.uniform(0, 6.28, (T, 64)).astype(np.float32))
    cos, sin = ang.cos().to(torch.bfloat16).to(DEV), ang.sin().to(torch.bfloat16).to(DEV)
    cos[: len(EDGE_ROWS)], sin[: len(EDGE_ROWS)] = 1.0, 0.0                            # the planted K rows reach the cache as they are
    dev_tbl = [torch.from_numpy(a).to(DEV) for a in (indptr, indices, last)]
    shape = (max_pages, L, 2, Hkv, P, 64)

    def fresh():
        if kind == "bf16":
            return torch.full(shape, -7.0, dtype=torch.bfloat16, device=DEV), None
        return torch.full(shape, 0x5A, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn), torch.full(shape[:5] + (2,), -3.0, dtype=torch.float16, device=DEV)

    data, param = fresh()
    want_data, want_param = data.view(torch.uint8 if param is not None else torch.int16).cpu().numpy().copy(), None if param is None else param.cpu().numpy().copy()
    q_rot, k_seen, v_seen = mixedgemm.rope_kv_append_dense(data, param, *dev_tbl, q, k, v, cos, sin, torch.from_numpy(app).to(DEV), layer)
    want_q, _ = mixedgemm.rope_qk(q, k, cos, sin)
    assert torch.equal(q_rot, want_q) and np.array_equal(bits(q_rot), bits(rope_cpu(q, cos, sin)))
    kr, vb = bits(rope_cpu(k, cos, sin)), bits(v)
    seen = {0: kr.copy(), 1: vb.copy()}
    for b, n in enumerate(counts):
        pages, sl = ko.slots(indptr, indices, P, b, np.arange(held[b], lens[b]))
        for which, src in ((0, kr), (1, vb)):
            rows = src[app[b]: app[b + 1]]
            if kind == "bf16":
                want_data[pages, layer, which, :, sl] = rows.view(np.int16)
            elif n:
                codes, e = kf.quantize_row(rows)
                want_data[pages, layer, which, :, sl], want_param[pages, layer, which, :, sl] = codes, kf.param_pair(e)
                seen[which][app[b]: app[b + 1]] = kf.dequantize(codes.astype(np.uint8), kf.param_pair(e))
    got = data.view(torch.uint8 if param is not None else torch.int16).cpu().numpy()
    assert np.array_equal(got, want_data)                                               # the slots, and the sentinel everywhere else
    assert param is None or np.array_equal(param.cpu().numpy().view(np.uint16), want_param.view(np.uint16))
    assert np.array_equal(bits(k_seen), seen[0]) and np.array_equal(bits(v_seen), seen[1])
    # rope_kv_append gives the same bytes and q; the copy form equals the rotate form at cos = 1, sin = 0
    d2, p2 = fresh()
    assert torch.equal(mixedgemm.rope_kv_append(d2, p2, *dev_tbl, q, k, v, cos, sin, torch.from_numpy(app).to(DEV), layer), q_rot)
    assert torch.equal(d2.view(torch.uint8), data.view(torch.uint8)) and (param is None or torch.equal(p2.view(torch.int16), param.view(torch.int16)))
    (d3, p3), (d4, p4) = fresh(), fresh()
    k[1, 0] = 0.0              # the planted -0.0 row of K: x * 1 + r * 0 is +0.0 there by IEEE (and by HF), a copy keeps the sign
    mixedgemm.kv_append(d3, p3, *dev_tbl, k.contiguous(), v.contiguous(), torch.from_numpy(app).to(DEV), layer)
    mixedgemm.rope_kv_append(d4, p4, *dev_tbl, q, k, v, torch.ones_like(cos), torch.zeros_like(sin), torch.from_numpy(app).to(DEV), layer)
    assert torch.equal(d3.view(torch.uint8), d4.view(torch.uint8)) and (param is None or torch.equal(p3.view(torch.int16), p4.view(torch.int16)))


@pytest.fixture(scope="module", params=[(kind, P, Hkv) for kind in KINDS for P in (1, 16) for Hkv in (1, 2, 4)], ids=str)
def filled(request):
    """one ragged batch per (kind, P, Hkv): Gaussian K and V on shuffled pages, layer 1 of 2; made once and left unchanged"""
    kind, P, Hkv = request.param
    rng = np.random.default_rng(7 * P + Hkv)
    tbl = table(LENGTHS, P, rng)
    data, param, seen = make_cache(kind, gauss_bits(rng, (tbl[3], 2, 2, Hkv, P, 64)))
    return kind, P, Hkv, tbl, data, param, seen


HEADS = {1: (16,), 2: (8, 14), 4: (4,)}              # Hkv -> Hq: g = 16; 4 and 7; 1
BOUNDS = (256, max(LENGTHS), 8192)                    # below the lengths (one chunk, attended in full all the same), tight, loose


@pytest.mark.parametrize("scale", [None, 0.4])
@pytest.mark.parametrize("bound", BOUNDS)
def test_decode_against_fp64(filled, bound, scale):
    kind, P, Hkv, tbl, data, param, seen = filled
    split = {b: mixedgemm.paged_decode_hd64_workspace_bytes(len(LENGTHS), HEADS[Hkv][0], Hkv, b) > 0 for b in BOUNDS}
    assert not split[256] and split[max(LENGTHS)] and split[8192]                      # a one-chunk case and split cases are both here
    for Hq in HEADS[Hkv]:
        q_bits = gauss_bits(np.random.default_rng(Hq), (len(LENGTHS), Hq, 64), 2.0)    # scale 2: one lost token shows
        o = decode(from_bits(q_bits), data, param, tbl, 1, bound, scale)
        ref, vmax = reference(q_bits, seen, *tbl[:3], P, 1, scale or 0.125)
        frac = worst(o, ref, vmax)
        print(f"kv_hd64 decode {kind} P={P} Hq={Hq} Hkv={Hkv} bound={bound} scale={scale}: worst fraction of the bound {frac:.3f}")
        assert frac <= 1.0 and not bits(o)[0].any()                                     # and the length-0 sequence gives zeros


@pytest.mark.parametrize("kind", KINDS)
def test_exact_count(kind):
    """q = 0 and V[t, d] = 1.875 [d == t % 64]: o[d] = 1.875 count_d / len to 1 bf16 ulp, on both sides of every chunk edge of the plan"""
    Hq, Hkv, P, bound = 8, 2, 16, 2048
    lens = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    B = len(lens)
    for _ in range(4):                                                                  # the plan depends on the batch the edges add to
        nc, cl = mixedgemm.paged_decode_hd64_plan(B, Hkv, bound)
        B = len(lens) + 2 * (nc - 1)
    assert nc > 1 and mixedgemm.paged_decode_hd64_plan(B, Hkv, bound) == (nc, cl)
    lens += [c * cl + side for c in range(1, nc) for side in (0, 1)]
    rng = np.random.default_rng(3)
    tbl = table(lens, P, rng)
    vals = gauss_bits(rng, (tbl[3], 1, 2, Hkv, P, 64))                                  # K: anything finite
    one = bits(torch.tensor([1.875], dtype=torch.bfloat16))[0]
    for b, n in enumerate(lens):
        pages, sl = ko.slots(tbl[0], tbl[1], P, b, np.arange(n))
        rows = np.zeros((n, Hkv, 64), dtype=np.uint16)
        rows[np.arange(n), :, np.arange(n) % 64] = one
        vals[pages, 0, 1, :, sl] = rows
    data, param, _ = make_cache(kind, vals)
    for bd in (256, max(lens), bound):                                                  # one chunk, tight, loose
        o = ko.bf16_to_f32(bits(decode(torch.zeros((B, Hq, 64), dtype=torch.bfloat16, device=DEV), data, param, tbl, 0, bd))).astype(np.float64)
        for b, n in enumerate(lens):
            want = 1.875 * np.bincount(np.arange(n) % 64, minlength=64) / n
            assert (np.abs(o[b] - want) <= bf16_ulp(want)).all(), (bd, n)


@pytest.mark.parametrize("bound", BOUNDS[:2])
def test_fp8_is_bf16_on_the_dequantized_values(filled, bound):
    _, P, Hkv, tbl, _, _, values = filled
    data, param, seen = make_cache("fp8_e4m3", values)       # the fixture's values, quantized (again: a fixed point for its fp8 half)
    for Hq in HEADS[Hkv]:
        q = from_bits(gauss_bits(np.random.default_rng(Hq), (len(LENGTHS), Hq, 64), 2.0))
        assert torch.equal(decode(q, data, param, tbl, 1, bound), decode(q, from_bits(seen), None, tbl, 1, bound))


@pytest.mark.parametrize("kind", KINDS)
def test_poison(kind):
    """NaN in every slot no sequence holds and on unreferenced pages: decode and the k_out / v_out of append are bit-equal to the clean run"""
    rng, P, Hq, Hkv, lens = np.random.default_rng(11), 16, 8, 2, [0, 5, 16, 300, 1300]
    tbl = table(lens, P, rng, spare=5)
    held = np.zeros((tbl[3], 1, 2, Hkv, P), dtype=bool)
    for b, n in enumerate(lens):
        pages, sl = ko.slots(tbl[0], tbl[1], P, b, np.arange(n))
        held[pages, :, :, :, sl] = True
    data, param, _ = make_cache(kind, gauss_bits(rng, held.shape + (64,)))
    dirty = data.clone().view(torch.uint8 if param is not None else torch.bfloat16)
    free = torch.from_numpy(~held).to(DEV)
    dirty[free] = 0x7F if param is not None else float("nan")
    dirty_param = None if param is None else param.clone()
    if param is not None:
        dirty, dirty_param[free] = dirty.view(torch.float8_e4m3fn), float("nan")
    q = from_bits(gauss_bits(rng, (len(lens), Hq, 64), 2.0))
    for bound in (256, max(lens)):
        assert torch.equal(decode(q, data, param, tbl, 0, bound), decode(q, dirty, dirty_param, tbl, 0, bound))
    # append: the table as it is counts one new token, the last, for every sequence that holds any
    qkv = [from_bits(gauss_bits(rng, (4, h, 64))) for h in (Hq, Hkv, Hkv)]
    cs = [from_bits(gauss_bits(rng, (4, 64))) for _ in range(2)]
    app = torch.tensor([0, 0, 1, 2, 3, 4], dtype=torch.int32, device=DEV)
    outs = [mixedgemm.rope_kv_append_dense(d, p, *(torch.from_numpy(a).to(DEV) for a in tbl[:3]), *qkv, *cs, app, 0)
            for d, p in ((data.clone(), None if param is None else param.clone()), (dirty, dirty_param))]
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def step_inputs(rng, T, Hq, Hkv):
    ang = torch.from_numpy(rng.uniform(0, 6.28, (T, 64)).astype(np.float32))
    return [from_bits(gauss_bits(rng, (T, h, 64))) for h in (Hq, Hkv, Hkv)] + [ang.cos().to(torch.bfloat16).to(DEV), ang.sin().to(torch.bfloat16).to(DEV)]


def test_graph_replay():
    """one hipGraph of append_rope + attend under a bound, replayed after each of three extend(1) steps with rewritten inputs"""
    rng, B, Hq, Hkv, bound = np.random.default_rng(5), 3, 8, 2, 600
    cache = PagedKVCache(num_layers=1, num_kv_heads=Hkv, page_size=16, max_pages=64, batch=B, kind="fp8_e4m3", device=DEV, head_dim=64)
    cache.extend([300, 31, 0])
    cache.append(0, *step_inputs(rng, 331, Hq, Hkv)[1:3])
    cache.extend(1)
    static = step_inputs(rng, B, Hq, Hkv)
    cache.attend(0, cache.append_rope(0, *static), max_seq_len=bound)                   # warm: the workspace exists before the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = cache.attend(0, cache.append_rope(0, *static), max_seq_len=bound)
    assert mixedgemm.paged_decode_hd64_workspace_bytes(B, Hq, Hkv, bound) > 0   # the replayed graph holds the merge launch too
    for _ in range(3):
        cache.extend(1)
        for dst, src in zip(static, step_inputs(rng, B, Hq, Hkv)):
            dst.copy_(src)
        graph.replay()
        assert torch.equal(out.clone(), cache.attend(0, cache.append_rope(0, *static), max_seq_len=bound))


@pytest.mark.parametrize("kind", KINDS)
def test_cache_class_end_to_end(kind):
    """extend(prompt) -> prefill_fresh, then three extend(1) -> append_rope -> attend, against fp64 on the values the cache holds"""
    rng, Hq, Hkv, P, prompt = np.random.default_rng(13), 8, 2, 16, [37, 5, 130]
    cache = PagedKVCache(num_layers=2, num_kv_heads=Hkv, page_size=P, max_pages=40, batch=3, kind=kind, device=DEV, head_dim=64)

    def held():
        raw = cache.kv_data.view(torch.uint8).cpu().numpy() if kind != "bf16" else bits(cache.kv_data)
        seen = raw if kind == "bf16" else kf.dequantize(raw, cache.kv_param.cpu().numpy())
        return seen, cache.kv_indptr.cpu().numpy(), cache.kv_indices.cpu().numpy(), cache.last_page_len.cpu().numpy()

    cache.extend(prompt)
    x = step_inputs(rng, sum(prompt), Hq, Hkv)
    o = ko.bf16_to_f32(bits(cache.prefill_fresh(1, *x))).astype(np.float64)
    q = ko.bf16_to_f32(bits(mixedgemm.rope_qk(x[0], x[1], x[3], x[4])[0])).astype(np.float64)
    seen, indptr, indices, last = held()
    t0 = 0
    for b, n in enumerate(prompt):
        k, v = gather(seen, indptr, indices, P, 1, b, n)
        s = np.einsum("ihd,thd->hit", q[t0: t0 + n], np.repeat(k, Hq // Hkv, axis=1)) * 0.125
        s = np.where(np.tril(np.ones((n, n), dtype=bool))[None], s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        ref = np.einsum("hit,thd->ihd", p / p.sum(-1, keepdims=True), np.repeat(v, Hq // Hkv, axis=1))
        assert (np.abs(o[t0: t0 + n] - ref) <= 2 * bf16_ulp(ref) + 2.0 ** -8 * np.abs(v).max()).all()      # DESIGN 7c's bound
        t0 += n
    for step in range(3):
        cache.extend(1)
        q_rot = cache.append_rope(1, *step_inputs(rng, 3, Hq, Hkv))
        o = cache.attend(1, q_rot)
        seen, indptr, indices, last = held()
        ref, vmax = reference(bits(q_rot), seen, indptr, indices, last, P, 1, 0.125)
        assert worst(o, ref, vmax) <= 1.0 and cache.seq_lens == [n + step + 1 for n in prompt]
