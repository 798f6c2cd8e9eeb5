"""GPU tests of the paged KV cache kernels on inputs whose answer is known exactly (tests/kv_exact_cases.py; the preconditions are
proved on the CPU in tests/test_kv_exact_cpu.py).

A needle   every query names the one token it must return: |o - V[target]| <= 2^-20 (p = 1, l = 1, V on the 1/8 grid)
B ramp     the score rises (falls) 45 nats per token: a query returns V of its own position (of position 0), <= 2^-20
C count    zero queries: the exact mean 1.875 count_d(p) / (p + 1), within 1 bf16 ulp of the fp64 value
D poison   the same answers, bit for bit, over a cache that held NaN everywhere before the append
E edge     the clamps, ties, floor and saturation of the int4 rule, byte for byte against tests/kv_oracle.py
F sm_scale 0.05 and 0.25 against the oracles, with the bounds of test_kvcache_gpu.py / test_kvprefill_gpu.py

No bound here comes from what a kernel produced.  Left out (of 9 g x 3 priors x 2 kinds needle prefill cases): the prior of
32768 - n runs at g = 4 only, and the 32768-token decode context at P = 16 only -- one 32k case per kernel and cache kind, the long
contexts being the slow ones; every g and every page size runs at priors 0 .. 300 and lengths up to 4096.

The decode cases of A, B and C query prefixes of ONE physical sequence, so the slots after a prefix's last token hold later, valid
tokens, not poison; the tail of the last page is poisoned only for the full length where that is no page multiple (4096 at P = 24 in
test_poison_needle_decode[2]) and in test_poison_gaussian_decode, whose sequences own their pages.  `fill` asserts that page 0 is
referenced by no sequence.  Pages are shuffled; test_append_edge_rows_byte_exact and the older files do use page 0.
"""
import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
import kv_exact_cases as kc
import kv_oracle as ko
import kv_prefill_oracle as kpo
import test_kvcache_gpu as t_dec
import test_kvprefill_gpu as t_pre

pytestmark = pytest.mark.gpu

KINDS = ["int4", "bf16"]
L, LAYER = 2, 1


def i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def bf(x, dev):
    """float32 numpy holding bf16 values -> bf16 tensor (exact)"""
    kc.bf16_bits(x)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(dev)


def f64(o):
    return o.float().cpu().numpy().astype(np.float64)


def fill(kind, K, V, lens, P, dev, poison=False, seed=0):
    """a cache of L layers whose layer LAYER holds the sequences' K / V (kv_append); page 0, the spare pages, the other layer and
    the tail of every last page keep the initial fill: zeros, or NaN / 0xFF (poison)"""
    indptr, indices, last, max_pages = kc.page_table(lens, P, seed)
    assert not (indices == 0).any(), "page 0 must stay unreferenced: invalid slots form their addresses from row 0"
    hd, hp = kc.empty_host_cache(kind, max_pages, L, K.shape[1], P, poison)
    data = torch.from_numpy(hd).to(dev) if kind == "int4" else torch.from_numpy(hd.view(np.int16)).to(dev).view(torch.bfloat16)
    param = torch.from_numpy(hp).to(dev) if hp is not None else None
    tbl = [i32(a, dev) for a in (indptr, indices, last)]
    mixedgemm.kv_append(data, param, *tbl, bf(K, dev), bf(V, dev), i32(kc.indptr_of(lens), dev), LAYER)
    return dict(data=data, param=param, tbl=tbl, tbl_h=(indptr, indices, last), pages=indices, P=P)


def prefill(cache, q, new, msl, sm_scale=None):
    return mixedgemm.paged_prefill(q, cache["data"], cache["param"], *cache["tbl"], i32(kc.indptr_of(new), q.device), LAYER, msl,
                                   sm_scale=sm_scale)


def decode_prefixes(cache, q, lens, msl, rows=None):
    """paged_decode of single-token queries over prefixes (lens[b] tokens) of the cache's ONE physical sequence"""
    rows = range(len(lens)) if rows is None else rows
    tbl = kc.prefix_table(cache["pages"], cache["P"], [lens[i] for i in rows])
    qq = q if len(rows) == len(lens) else q[list(rows)].contiguous()
    return mixedgemm.paged_decode(qq, cache["data"], cache["param"], *(i32(a, q.device) for a in tbl), LAYER, msl)


def expect_rows(o, want, labels, bound, what, grid=True):
    got = f64(o).reshape(-1, 128)
    msg = kc.describe_mismatch(got, want.reshape(-1, 128), labels, bound, grid)
    assert msg is None, f"{what}: {msg}"


def prefill_labels(c):
    seq = np.repeat(np.arange(len(c["new"])), c["new"])
    pos = np.concatenate([a + np.arange(n) for a, n in zip(c["prior"], c["new"])] + [np.zeros(0, np.int64)])
    return lambda i: f"query of seq {seq[i // c['Hq']]} (prior {c['prior'][seq[i // c['Hq']]]}) pos {pos[i // c['Hq']]} head {i % c['Hq']}"


def decode_labels(c):
    return lambda i: f"sequence {i // c['Hq']} of length {c['lens'][i // c['Hq']]} head {i % c['Hq']}"


def run_prefill_case(kind, c, dev, bound, poison=False, need_split=False, grid=True):
    cache = fill(kind, c["K"], c["V"], c["lens"], c["P"], dev, poison)
    q, msl = bf(c["q"], dev), max(c["lens"])
    if need_split:
        assert mixedgemm.paged_prefill_workspace_bytes(q.size(0), len(c["new"]), c["Hq"], c["Hkv"], msl) > 0, "must take the split path"
    outs = [prefill(cache, q, c["new"], m) for m in (msl, msl + 5000)]
    torch.cuda.synchronize()
    for o, what in zip(outs, ("tight bound", "loose bound")):
        expect_rows(o, c["expect"], prefill_labels(c), bound, f"{kind} g={c['g']} P={c['P']} {what}", grid)
    return outs[0]


def run_decode_case(kind, c, dev, bound, poison=False, groups=True):
    """all sequences in one launch (tight and loose bound), then in launches of 8 and of 1, which split the tokens into chunks"""
    cache = fill(kind, c["K"], c["V"], [c["N"]], c["P"], dev, poison)
    q, lens, Hq = bf(c["q"], dev), c["lens"], c["Hq"]
    msl, lab = max(lens), decode_labels(c)
    outs = [decode_prefixes(cache, q, lens, m) for m in (msl, msl + 5000)]
    torch.cuda.synchronize()
    for o, what in zip(outs, ("one launch, tight bound", "one launch, loose bound")):
        expect_rows(o, c["expect"], lab, bound, f"{kind} g={c['g']} P={c['P']} {what}")
    if groups:
        if msl >= 4096:
            assert mixedgemm.paged_decode_workspace_bytes(8, Hq, c["Hkv"], msl) > 0, "launches of 8 must take the split path"
        parts = [(list(range(i, min(i + 8, len(lens))))) for i in range(0, len(lens), 8)] + [[i] for i in range(min(4, len(lens)))]
        for rows in parts:
            o = decode_prefixes(cache, q, lens, msl, rows)
            expect_rows(o, c["expect"][rows], lambda i: lab(rows[i // Hq] * Hq + i % Hq), bound,
                        f"{kind} g={c['g']} P={c['P']} launch of sequences {rows[0]}..{rows[-1]}")
    return outs[0]


# ---- A. needle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(len(kc.NEEDLE_PREFILL_SHAPES)))
def test_needle_prefill(dev, kind, i):
    c = kc.needle_prefill_case(i)
    assert kc.needle_prefill_uncovered(c) == []
    run_prefill_case(kind, c, dev, kc.EXACT_BOUND)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(len(kc.NEEDLE_PREFILL_SHAPES)))
def test_needle_prefill_every_alignment(dev, kind, i):
    """priors 0 .. 63: the diagonal and p - 1 targets on every row of a query tile at every position within a 64-token kv tile"""
    run_prefill_case(kind, kc.needle_prefill_every_alignment(i), dev, kc.EXACT_BOUND)


@pytest.mark.parametrize("kind", KINDS)
def test_needle_prefill_32k_split(dev, kind):
    c = kc.needle_prefill_32k()
    assert kc.needle_prefill_uncovered(c) == []
    run_prefill_case(kind, c, dev, kc.EXACT_BOUND, need_split=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(len(kc.NEEDLE_DECODE_SHAPES)))
def test_needle_decode(dev, kind, i):
    c = kc.needle_decode_case(i)
    assert kc.needle_decode_uncovered(c) == []
    run_decode_case(kind, c, dev, kc.EXACT_BOUND)


# ---- B. ramp ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["rising", "falling"])
@pytest.mark.parametrize("gi", range(len(kc.G_VALUES)))
def test_ramp_prefill(dev, kind, sign, gi):
    g = kc.G_VALUES[gi]
    c = kc.ramp_prefill(g, 2, kc.PAGE_SIZES[gi % 4], sign)
    run_prefill_case(kind, c, dev, kc.EXACT_BOUND, need_split=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gi", range(len(kc.G_VALUES)))
def test_ramp_prefill_every_alignment(dev, kind, gi):
    """priors 0 .. 63: every row of a query tile meets every position within a 64-token kv tile"""
    c = kc.ramp_prefill(kc.G_VALUES[gi], 2, kc.PAGE_SIZES[(gi + 1) % 4], 1.0, priors=kc.RAMP_RESIDUES)
    run_prefill_case(kind, c, dev, kc.EXACT_BOUND)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["rising", "falling"])
def test_ramp_decode(dev, kind, sign):
    c = kc.ramp_decode(4, 2, 16, sign)
    run_decode_case(kind, c, dev, kc.EXACT_BOUND)


# ---- C. counting -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(len(kc.COUNT_PREFILL_CASES)))
def test_count_prefill(dev, kind, i):
    c = kc.count_prefill(*kc.COUNT_PREFILL_CASES[i])
    run_prefill_case(kind, c, dev, kc.bf16_ulp(c["expect"]).reshape(-1, 128), grid=False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(len(kc.COUNT_DECODE_SHAPES)))
def test_count_decode(dev, kind, i):
    c = kc.count_decode(*kc.COUNT_DECODE_SHAPES[i])
    cache = fill(kind, c["K"], c["V"], [c["N"]], c["P"], dev)
    q, lens, Hq = bf(c["q"], dev), c["lens"], c["Hq"]
    ulp = kc.bf16_ulp(c["expect"])
    for msl, rows in ((4096, None), (9000, None), (4096, list(range(len(lens) - 3, len(lens))))):   # one chunk / loose / split-KV
        o = decode_prefixes(cache, q, lens, msl, rows)
        sel = slice(None) if rows is None else rows
        base = 0 if rows is None else rows[0]
        expect_rows(o, c["expect"][sel], lambda i: decode_labels(c)(i + base * Hq), ulp[sel].reshape(-1, 128),
                    f"{kind} g={c['g']} P={c['P']} bound {msl} rows {rows}", grid=False)
    assert mixedgemm.paged_decode_workspace_bytes(3, Hq, c["Hkv"], 4096) > 0


# ---- D. poisoned cache -------------------------------------------------------------------------------------------------------
def same_bits(a, b, what):
    assert torch.isfinite(b.float()).all(), f"{what}: not finite over a poisoned cache"
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{what}: differs from the zero-initialised cache"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", [1, 4, 8])
def test_poison_needle_prefill(dev, kind, i):
    c = kc.needle_prefill_case(i)
    same_bits(run_prefill_case(kind, c, dev, kc.EXACT_BOUND), run_prefill_case(kind, c, dev, kc.EXACT_BOUND, poison=True), "needle prefill")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", [1, 2])
def test_poison_needle_decode(dev, kind, i):
    c = kc.needle_decode_case(i)
    same_bits(run_decode_case(kind, c, dev, kc.EXACT_BOUND, groups=False), run_decode_case(kind, c, dev, kc.EXACT_BOUND, poison=True),
              "needle decode")


def gauss(shape, rng, scale):
    return kc.to_bf16(rng.standard_normal(shape).astype(np.float32) * scale)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [1, 2, 4])
def test_poison_gaussian_decode(dev, kind, case):
    """the Gaussian cases of test_kvcache_gpu.py over a poisoned cache, with that file's bound"""
    Hq, Hkv, lens = t_dec.CASES[case]
    rng = np.random.default_rng(500 + case)
    T = sum(lens)
    K, V, q = gauss((T, Hkv, 128), rng, 1.0), gauss((T, Hkv, 128), rng, 0.5), bf(gauss((len(lens), Hq, 128), rng, 2.0), dev)
    outs = []
    for poison in (False, True):
        c = fill(kind, K, V, lens, 16, dev, poison, seed=case)
        outs.append(mixedgemm.paged_decode(q, c["data"], c["param"], *c["tbl"], LAYER, max(lens)))
    torch.cuda.synchronize()
    same_bits(outs[0], outs[1], "decode")
    hd, hp = t_dec.host(c["data"], c["param"])
    t_dec.check_attention(outs[1], ko.attention(t_dec.bits(q), hd, hp, *c["tbl_h"], LAYER), float(np.abs(V).max()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [1, 2, 4])
def test_poison_gaussian_prefill(dev, kind, case):
    """the Gaussian cases of test_kvprefill_gpu.py over a poisoned cache, with that file's bound"""
    Hq, Hkv, P, prior, new = t_pre.CASES[case]
    lens = [a + n for a, n in zip(prior, new)]
    rng = np.random.default_rng(600 + case)
    T = sum(lens)
    K, V, q = gauss((T, Hkv, 128), rng, 1.0), gauss((T, Hkv, 128), rng, 0.5), bf(gauss((sum(new), Hq, 128), rng, 2.0), dev)
    outs = []
    for poison in (False, True):
        c = fill(kind, K, V, lens, P, dev, poison, seed=case)
        outs.append(prefill(c, q, new, max(lens)))
    torch.cuda.synchronize()
    same_bits(outs[0], outs[1], "prefill")
    hd, hp = t_pre.host(c["data"], c["param"])
    qo = kc.indptr_of(new)
    want = kpo.attention(t_pre.bits(q), hd, hp, *c["tbl_h"], qo, LAYER)
    t_pre.check(outs[1], want, kpo.vmax(tuple(q.shape), hd, hp, *c["tbl_h"], qo, LAYER), "poisoned")


# ---- E. edge rows of kv_append -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", [1, 16])
def test_append_edge_rows_byte_exact(dev, kind, P):
    Hkv = 4
    k, v = kc.edge_batch(Hkv, seed=P)
    T = k.shape[0]
    new = [T - 12, 0, 5, 7]
    before = [0, 3, P - 1, 2 * P + 1]
    lens = [a + n for a, n in zip(before, new)]
    indptr, indices, last, max_pages = kc.page_table(lens, P, seed=P, free_page0=False)
    data, param = t_dec.empty_cache(kind, max_pages, 3, Hkv, P, dev)
    want_d, want_p = t_dec.host(data, param)
    app = kc.indptr_of(new)
    mixedgemm.kv_append(data, param, i32(indptr, dev), i32(indices, dev), i32(last, dev), bf(k, dev), bf(v, dev), i32(app, dev), 1)
    torch.cuda.synchronize()
    with np.errstate(over="ignore"):                   # max - min of the +-bf16-max row is inf by design
        ko.append(want_d, want_p, indptr, indices, last, kc.bf16_bits(k), kc.bf16_bits(v), app, 1)
    got_d, got_p = t_dec.host(data, param)
    if kind == "int4":
        # name the row family first: a plain count of differing bytes would not say which branch of the rule is off
        seq = np.repeat(np.arange(len(new)), new)
        for i in range(T):
            b = int(seq[i])
            pos = lens[b] - new[b] + (i - app[b])
            page, slot = indices[indptr[b] + pos // P], pos % P
            for which in (0, 1):
                for h in range(Hkv):
                    gd, wd = got_d[page, 1, which, h, slot], want_d[page, 1, which, h, slot]
                    gp, wp = got_p[page, 1, which, h, slot].view(np.uint16), want_p[page, 1, which, h, slot].view(np.uint16)
                    src = (v if which else k)[i, h]
                    name = next((n for n, r in kc.edge_rows().items() if np.array_equal(r.view(np.uint32), src.view(np.uint32))), "gaussian")
                    assert np.array_equal(gd, wd) and np.array_equal(gp, wp), (
                        f"{'V' if which else 'K'} row '{name}' (token {i}, head {h}): codes {sorted(set(ko.unpack_codes(gd).tolist()))} "
                        f"(scale, zero) {[hex(x) for x in gp]}, oracle {sorted(set(ko.unpack_codes(wd).tolist()))} {[hex(x) for x in wp]}")
        assert np.array_equal(got_p.view(np.uint16), want_p.view(np.uint16)), "params outside the target slots changed"
    assert np.array_equal(got_d, want_d), f"{int((got_d != want_d).sum())} cache bytes differ"


# ---- F. sm_scale ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sm_scale", [0.05, 0.25])
@pytest.mark.parametrize("lens, split", [([100, 7, 0, 64], False), ([17, 300, 4096], True)])
def test_sm_scale_decode(dev, kind, sm_scale, lens, split):
    Hq, Hkv = 32, 8
    assert (mixedgemm.paged_decode_workspace_bytes(len(lens), Hq, Hkv, max(lens)) > 0) == split
    rng = np.random.default_rng(700)
    T = sum(lens)
    K, V, q = gauss((T, Hkv, 128), rng, 1.0), gauss((T, Hkv, 128), rng, 0.5), bf(gauss((len(lens), Hq, 128), rng, 2.0), dev)
    c = fill(kind, K, V, lens, 16, dev)
    o = mixedgemm.paged_decode(q, c["data"], c["param"], *c["tbl"], LAYER, max(lens), sm_scale=sm_scale)
    torch.cuda.synchronize()
    hd, hp = t_dec.host(c["data"], c["param"])
    want = ko.attention(t_dec.bits(q), hd, hp, *c["tbl_h"], LAYER, sm_scale=sm_scale)
    assert np.abs(want - ko.attention(t_dec.bits(q), hd, hp, *c["tbl_h"], LAYER)).max() > 0.05, "the scale must matter"
    t_dec.check_attention(o, want, float(np.abs(V).max()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sm_scale", [0.05, 0.25])
@pytest.mark.parametrize("prior, new, split", [([0, 40], [100, 30], False), ([5000, 100], [17, 5], True)])
def test_sm_scale_prefill(dev, kind, sm_scale, prior, new, split):
    Hq, Hkv = 32, 8
    lens = [a + n for a, n in zip(prior, new)]
    assert (mixedgemm.paged_prefill_workspace_bytes(sum(new), len(new), Hq, Hkv, max(lens)) > 0) == split
    rng = np.random.default_rng(800)
    T = sum(lens)
    K, V, q = gauss((T, Hkv, 128), rng, 1.0), gauss((T, Hkv, 128), rng, 0.5), bf(gauss((sum(new), Hq, 128), rng, 2.0), dev)
    c = fill(kind, K, V, lens, 16, dev)
    o = prefill(c, q, new, max(lens), sm_scale=sm_scale)
    torch.cuda.synchronize()
    hd, hp = t_pre.host(c["data"], c["param"])
    qo = kc.indptr_of(new)
    want = kpo.attention(t_pre.bits(q), hd, hp, *c["tbl_h"], qo, LAYER, sm_scale=sm_scale)
    assert np.abs(want - kpo.attention(t_pre.bits(q), hd, hp, *c["tbl_h"], qo, LAYER)).max() > 0.05, "the scale must matter"
    t_pre.check(o, want, kpo.vmax(tuple(q.shape), hd, hp, *c["tbl_h"], qo, LAYER), f"sm_scale {sm_scale}")
