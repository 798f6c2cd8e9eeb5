"""GPU tests of the edges include/micromix_kv_hd64.h and micromix_kv_prefill_hd64.h promise for the 64-wide paged cache and no other test
reaches: page-table entries outside [0, max_pages) (-1, max_pages, 2^31 - 1) in attention and in append, a last_page_len outside [0, P],
an append_indptr that brings more tokens than the table counts, and NaN in page 0 (masked lanes form their addresses from row 0).

The expectations are exact: the count construction of tests/kv_exact_cases_hd64.py over the tokens that remain (1 bf16 ulp), the needle
construction (2^-20), zeros -- not NaN -- for a sequence without a valid page, and caches compared byte for byte with a twin that
received the equivalent valid call.  Sequences own their pages here and every cache is poisoned before the library appends to it."""
import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
import kv_exact_cases_hd64 as k6
from kv_hd64_gpu_util import KINDS, LAYER, bf, device_cache, expect_rows, f64, fill, i32

pytestmark = pytest.mark.gpu

BAD = (-1, None, 2 ** 31 - 1)              # None: max_pages
G, HKV, N = 4, 2, 1300
HQ = G * HKV
PLACES = ("first tile of chunk 0", "first tile of a later chunk", "a page in the middle", "the last page", "every page", "none")


def raw(t):
    return t.view(torch.uint8).cpu().numpy() if t.dtype is not torch.float16 else t.view(torch.int16).cpu().numpy()


def off_tokens(place, P, chunk_starts):
    """bool [N]: the tokens whose page the placement takes off the cache (whole pages: a page that holds one such token goes)"""
    off = np.zeros(N, dtype=bool)
    spans = {"first tile of chunk 0": [(0, 64)], "first tile of a later chunk": [(s, s + 64) for s in chunk_starts],
             "a page in the middle": [(700, 701)], "the last page": [(N - 1, N)], "every page": [(0, N)], "none": []}[place]
    for a, b in spans:
        off[(a // P) * P: min(-(-b // P) * P, N)] = True
    return off


def with_bad_pages(cache, off, P):
    """the cache's page table with the entry of every page that holds an off token replaced by -1, max_pages, 2^31 - 1 in turn"""
    indptr, indices, last = (a.copy() for a in cache["tbl_h"])
    k = 0
    for b in range(len(last)):
        for pg in np.flatnonzero(np.add.reduceat(off[b].astype(np.int64), np.arange(0, N, P)) > 0):
            v = BAD[k % 3]
            indices[indptr[b] + pg] = cache["max_pages"] if v is None else v
            k += 1
    return indptr, indices, last


@pytest.mark.parametrize("P", [3, 16, 100])
def test_pages_outside_the_cache_are_not_attended(dev, P):
    """count and needle, decode and prefill (both workgroup shapes): the exact answer of the sequence without the tokens whose page
    entry lies outside the cache; a sequence with no valid page gives zeros.  The first tile of chunk 0 off reaches consume_tile's
    `base = mn == -inf ? 0 : mn`; masked tokens of the prefill fetch its row of zeros while page 0 holds NaN"""
    B = len(PLACES)
    nc, cl = mixedgemm.paged_decode_hd64_plan(B, HKV, N)
    plans = {new: mixedgemm.paged_prefill_hd64_plan(B * new, B, HQ, HKV, N) for new in (70, 1)}
    assert nc > 1 and plans[70].rows == 128 and plans[1].rows == 64 and plans[70].chunks > 1 and plans[1].chunks > 1
    starts = sorted({cl} | {p.chunk_len for p in plans.values()})
    off = np.stack([off_tokens(place, P, starts) for place in PLACES])
    assert off[4].all() and not off[5].any() and all(off[i].any() and not off[i].all() for i in range(4))
    present = ~off
    # needle targets: per (sequence, query position, head) a present token <= the position, the ones next to the hole first
    def targets(b, p):
        ok = np.flatnonzero(present[b, : p + 1])
        if ok.size == 0:
            return np.full(HQ, -1)
        hole = np.flatnonzero(off[b, : p + 1])
        near = [ok[ok < hole[0]][-1:], ok[ok > hole[-1]][:1]] if hole.size else []
        first = np.concatenate([ok[:1], ok[-1:], *near]).astype(np.int64)
        return np.concatenate([first, np.random.default_rng(1000 * b + p).choice(ok, HQ - len(first))])[:HQ]   # the same for both kinds
    lens = [N] * B
    kvh = np.arange(HQ) // G
    cases = {"count": (np.concatenate([np.repeat(k6.ramp_k(np.arange(N))[:, None], HKV, 1)] * B),
                       np.concatenate([np.repeat(k6.count_v(np.arange(N))[:, None], HKV, 1)] * B)),
             "needle": (np.concatenate([np.stack([k6.code(h, N) for h in range(HKV)], 1).astype(np.float32)] * B),
                        np.concatenate([k6.v_grid(b, np.arange(N)[:, None], np.arange(HKV)[None, :]) for b in range(B)]))}
    k6.needle_margin_nats(HKV)
    for what, (K, V) in cases.items():
        outs = {}
        for kind in KINDS:
            cache = fill(kind, K, V, lens, P, dev, seed=P)
            tbl = [i32(a, dev) for a in with_bad_pages(cache, off, P)]
            for new in (1, 70):                              # new = 1 runs as decode too
                pos = np.stack([N - new + np.arange(new)] * B)                                   # [B, new]
                if what == "count":
                    q = np.zeros((B * new, HQ, 64), dtype=np.float32)
                    want = np.stack([k6.count_expect(p, present[b]) for b in range(B) for p in pos[b]])[:, None].repeat(HQ, 1)
                    bound, grid = k6.bf16_ulp(want).reshape(-1, 64), False
                else:
                    tg = np.stack([targets(b, p) for b in range(B) for p in pos[b]])             # [B * new, HQ]
                    q = np.stack([16.0 * k6.codebook(h)[np.maximum(tg[:, hq], 0), :64] for hq, h in enumerate(kvh)], 1).astype(np.float32)
                    seq = np.repeat(np.arange(B), new)[:, None]
                    want = np.where((tg >= 0)[..., None], k6.v_grid(seq, np.maximum(tg, 0), kvh[None, :]), 0.0).astype(np.float64)
                    bound, grid = k6.EXACT_BOUND, True
                label = lambda i: f"{PLACES[i // (new * HQ)]} off, position {pos[0][(i // HQ) % new]}, head {i % HQ}"
                qo = i32(np.arange(B + 1) * new, dev)
                for msl in (256, N):
                    o = mixedgemm.paged_prefill(bf(q, dev), cache["data"], cache["param"], *tbl, qo, LAYER, msl)
                    expect_rows(o, want, label, bound, f"{what} prefill {kind} P={P} new={new} bound {msl}", grid)
                    outs[kind, "prefill", new, msl] = o
                    if new == 1:
                        o = mixedgemm.paged_decode(bf(q, dev), cache["data"], cache["param"], *tbl, LAYER, msl)
                        expect_rows(o, want, label, bound, f"{what} decode {kind} P={P} bound {msl}", grid)
                        outs[kind, "decode", new, msl] = o
                        assert not f64(o)[4].any(), "a sequence whose pages all lie off the cache must give zeros"
        for key in [k for k in outs if k[0] == "fp8"]:
            assert torch.equal(outs[key].view(torch.int16), outs[("bf16",) + key[1:]].view(torch.int16)), f"{what} {key}: fp8 differs from bf16"


def append_inputs(rng, T, dev):
    g = lambda h: bf(k6.kc.to_bf16(rng.standard_normal((T, h, 64)).astype(np.float32)), dev)
    ang = torch.from_numpy(rng.uniform(0, 6.28, (T, 64)).astype(np.float32))
    return g(HQ), g(HKV), g(HKV), ang.cos().to(torch.bfloat16).to(dev), ang.sin().to(torch.bfloat16).to(dev)


def append_both(kind, P, dev, lens, counts, table, twin_table, twin_counts=None, twin_rows=None, seed=0):
    """rope_kv_append_dense of `counts` tokens under `table` on one poisoned cache, and of twin_counts tokens (rows twin_rows of the
    same inputs) under the valid `twin_table` on another: returns (cache, twin, outputs, twin outputs, inputs)"""
    max_pages = k6.page_table(lens, P, seed)[3]
    x = append_inputs(np.random.default_rng(seed + P), sum(counts), dev)
    res = []
    for tbl, cnt, rows in ((table, counts, None), (twin_table, twin_counts or counts, twin_rows)):
        data, param = device_cache(kind, max_pages, HKV, P, dev)
        xs = x if rows is None else [t[torch.tensor(rows, device=dev)].contiguous() for t in x]
        out = mixedgemm.rope_kv_append_dense(data, param, *(i32(a, dev) for a in tbl), *xs, i32(k6.indptr_of(cnt), dev), LAYER)
        res.append((data, param, out))
    return res[0], res[1], x


def assert_same_cache(a, b, what):
    for name, x, y in (("data", a[0], b[0]), ("param", a[1], b[1])):
        if x is not None:
            assert np.array_equal(raw(x), raw(y)), f"{what}: {name} differs from the twin's"


@pytest.mark.parametrize("P", [3, 16, 100])
@pytest.mark.parametrize("kind", KINDS)
def test_append_to_a_page_outside_the_cache_writes_nothing(dev, kind, P):
    """entries -1, max_pages and 2^31 - 1 under appended tokens: the cache afterwards equals, byte for byte in data and params, a twin
    appended to under the valid table whose refused pages were then put back to what they held -- every slot of a refused page keeps
    its poison, every other slot is written as usual --; k_out / v_out are written for every token and q_out is the rotation"""
    lens, counts = [2 * P + 1, 5 * P, 7, 3 * P + 2], [2 * P + 1, 2 * P + 3, 7, P + 2]
    indptr, indices, last, max_pages = k6.page_table(lens, P, seed=1)
    bad = indices.copy()
    refused = [indptr[0] + 1, indptr[1] + 4, indptr[2], indptr[3] + 2]       # a middle page, a last page, an only page, and one more
    for k, e in enumerate(refused):
        bad[e] = max_pages if BAD[k % 3] is None else BAD[k % 3]
    # the twin: the same call under the valid table, after which the refused pages are put back to what an untouched cache holds
    app = k6.indptr_of(counts)
    x = append_inputs(np.random.default_rng(P), sum(counts), dev)
    data, param = device_cache(kind, max_pages, HKV, P, dev)
    q_out, k_out, v_out = mixedgemm.rope_kv_append_dense(data, param, *(i32(a, dev) for a in (indptr, bad, last)), *x, i32(app, dev), LAYER)
    twin, twin_p = device_cache(kind, max_pages, HKV, P, dev)
    tq, tk, tv = mixedgemm.rope_kv_append_dense(twin, twin_p, *(i32(a, dev) for a in (indptr, indices, last)), *x, i32(app, dev), LAYER)
    assert torch.equal(q_out, tq) and torch.equal(q_out, mixedgemm.rope_qk(x[0], x[1], x[3], x[4])[0]), "q_out is the rotation whatever the table says"
    assert torch.equal(k_out, tk) and torch.equal(v_out, tv), "k_out / v_out are written for every token, whether or not its slot was"
    blank, blank_p = device_cache(kind, max_pages, HKV, P, dev)
    pages = torch.tensor([int(indices[e]) for e in refused], device=dev)
    twin[pages] = blank[pages]                               # the refused pages keep what they held
    if twin_p is not None:
        twin_p[pages] = blank_p[pages]
    assert_same_cache((data, param), (twin, twin_p), f"{kind} P={P}")


@pytest.mark.parametrize("P", [3, 16, 100])
def test_last_page_len_is_clamped(dev, P):
    """last_page_len of -5, 0 and P + 7 answers as clamp(.., 0, P): decode and prefill by the count construction, and append writes
    exactly the slots the clamped length names"""
    pages = [3, 2, 4, 1]
    given = np.array([-5, 0, P + 7, -5], dtype=np.int32)
    clamped = np.clip(given, 0, P)
    lens = [(n - 1) * P + int(c) for n, c in zip(pages, clamped)]
    full = [n * P for n in pages]
    B = len(pages)
    K = np.concatenate([np.repeat(k6.ramp_k(np.arange(n))[:, None], HKV, 1) for n in full])
    V = np.concatenate([np.repeat(k6.count_v(np.arange(n))[:, None], HKV, 1) for n in full])
    outs = {}
    for kind in KINDS:
        cache = fill(kind, K, V, full, P, dev, seed=2)
        tbl = [cache["tbl"][0], cache["tbl"][1], i32(given, dev)]
        new = [min(2, n) for n in lens]
        pos = np.concatenate([n - m + np.arange(m) for n, m in zip(lens, new)]).astype(np.int64)
        want = np.repeat(k6.count_expect(pos)[:, None], HQ, 1)
        o = mixedgemm.paged_prefill(torch.zeros((sum(new), HQ, 64), dtype=torch.bfloat16, device=dev), cache["data"], cache["param"], *tbl,
                                    i32(k6.indptr_of(new), dev), LAYER, max(full))
        expect_rows(o, want, lambda i: f"query {i // HQ}", k6.bf16_ulp(want).reshape(-1, 64), f"prefill {kind} P={P}", grid=False)
        want = np.repeat(k6.count_expect(np.array(lens) - 1)[:, None], HQ, 1)
        d = mixedgemm.paged_decode(torch.zeros((B, HQ, 64), dtype=torch.bfloat16, device=dev), cache["data"], cache["param"], *tbl, LAYER, max(full))
        expect_rows(d, want, lambda i: f"sequence {i // HQ} of length {lens[i // HQ]}", k6.bf16_ulp(want).reshape(-1, 64), f"decode {kind} P={P}", grid=False)
        outs[kind] = (o, d)
        # append: two tokens per sequence under the given lengths and under the clamped ones
        indptr, indices = cache["tbl_h"][0], cache["tbl_h"][1]
        counts = [2] * B
        a, b, _ = append_both(kind, P, dev, full, counts, (indptr, indices, given), (indptr, indices, clamped), seed=2)
        assert_same_cache(a, b, f"append {kind} P={P}")
        assert all(torch.equal(s, t) for s, t in zip(a[2], b[2]))
    assert all(torch.equal(s.view(torch.int16), t.view(torch.int16)) for s, t in zip(outs["fp8"], outs["bf16"]))


@pytest.mark.parametrize("P", [3, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_tokens_the_table_does_not_count_are_not_written(dev, kind, P):
    """an append_indptr that gives sequences more tokens than they hold: the surplus (the first of each) is dropped, the rest lands on
    the sequence's positions from 0, and no other slot changes -- the twin receives exactly the kept rows"""
    lens, counts = [5, 2 * P + 1, 0, P], [9, 2 * P + 4, 3, P]
    tbl = k6.page_table(lens, P, seed=3)[:3]
    app = k6.indptr_of(counts)
    kept = [min(c, n) for c, n in zip(counts, lens)]
    rows = [int(app[b + 1]) - m + j for b, m in enumerate(kept) for j in range(m)]
    a, b, x = append_both(kind, P, dev, lens, counts, tbl, tbl, kept, rows, seed=3)
    assert_same_cache(a, b, f"{kind} P={P}")
    sel = torch.tensor(rows, device=dev)
    assert all(torch.equal(s[sel], t) for s, t in zip(a[2], b[2])), "the outputs of the kept tokens"
    assert torch.equal(a[2][0], mixedgemm.rope_qk(x[0], x[1], x[3], x[4])[0]), "q_out is the rotation for every token"


@pytest.mark.parametrize("P", [16, 24])
@pytest.mark.parametrize("kind", KINDS)
def test_poison_with_page_0_poisoned(dev, kind, P):
    """test_kv_hd64_gpu.py::test_poison with a page table that leaves page 0 free, so that row 0 -- which every masked lane addresses --
    holds NaN: decode and prefill are bit-equal to the run over a cache that held zeros, and finite"""
    rng, lens = np.random.default_rng(11), [0, 5, 16, 300, 1300]
    gauss = lambda shape, s: k6.kc.to_bf16(rng.standard_normal(shape).astype(np.float32) * s)
    K, V = gauss((sum(lens), HKV, 64), 1.0), gauss((sum(lens), HKV, 64), 0.5)
    clean, dirty = (fill(kind, K, V, lens, P, dev, seed=4, poison=p) for p in (False, True))
    assert 0 not in clean["pages"] and np.array_equal(clean["pages"], dirty["pages"])
    q = bf(gauss((len(lens), HQ, 64), 2.0), dev)
    new = [0, 3, 16, 70, 1]
    qn, qo = bf(gauss((sum(new), HQ, 64), 2.0), dev), i32(k6.indptr_of(new), dev)
    for bound in (256, max(lens)):
        a, b = (mixedgemm.paged_decode(q, c["data"], c["param"], *c["tbl"], LAYER, bound) for c in (clean, dirty))
        assert torch.isfinite(b.float()).all() and torch.equal(a.view(torch.int16), b.view(torch.int16)), f"decode, bound {bound}"
        a, b = (mixedgemm.paged_prefill(qn, c["data"], c["param"], *c["tbl"], qo, LAYER, bound) for c in (clean, dirty))
        assert torch.isfinite(b.float()).all() and torch.equal(a.view(torch.int16), b.view(torch.int16)), f"prefill, bound {bound}"
