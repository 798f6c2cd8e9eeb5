"""GPU tests of the paged cache for 64-wide heads on inputs whose answer is known exactly (tests/kv_exact_cases_hd64.py; every
precondition is proved on the CPU in tests/test_kv_exact_hd64_cpu.py): WHO is attended, which the Gaussian tests of test_kv_hd64_gpu.py
and test_kv_prefill_hd64_gpu.py cannot tell under their bounds.

A needle   every query names the one token it must return: |o - V[target]| <= 2^-20, and a failure names the token that came back
B ramp     the score rises (falls) 64 nats per token: a query returns V of its own position (of position 0), <= 2^-20
C count    zero queries: the exact mean 1.875 count_d / n, within 1 bf16 ulp of the fp64 value

through paged_decode, paged_prefill (both workgroup shapes, asserted from the plan), a one-token prefill against the decode of the same
position, and the fresh-prompt route rope_kv_append_dense -> dense_attention.  Page sizes 1, 3, 16, 24, 64, 100 and every g of G_VALUES;
lengths and priors on both sides of every tile edge and of every chunk edge the library's plan reports for the bound in use.

Every cache is filled by the library's own kv_append or rope_kv_append (cos 1, sin 0) over NaN: bf16 NaN, or e4m3 NaN codes with NaN
params, in page 0 (which no sequence owns: the kernels form the addresses of masked tokens from row 0), in the spare pages, in the two
other layers and behind every sequence's last token.  Both kinds run in every case, and since every row is exact in fp8 the bf16 cache
holds the dequantized values of the fp8 one: the two outputs must be equal bit for bit (include/micromix_kv_hd64.h).  No bound here
comes from what a kernel produced; DESIGN 7ad has the errors observed.  The decode cases query prefixes of ONE physical sequence, so
the slots behind a prefix hold later, valid tokens; test_kv_edges_hd64_gpu.py has sequences that own their pages."""
import functools

import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
import kv_exact_cases_hd64 as k6
from kv_hd64_gpu_util import KINDS, LAYER, bf, device_cache, expect_rows, f64, fill, i32
import test_dense_attention_hd64_gpu as t_dense

pytestmark = pytest.mark.gpu

N_SHAPES = len(k6.SHAPES)
decode_plan = mixedgemm.paged_decode_hd64_plan
prefill_plan = lambda *a: tuple(mixedgemm.paged_prefill_hd64_plan(*a))


def prefill_labels(c):
    seq = np.repeat(np.arange(len(c["new"])), c["new"])
    pos = np.concatenate([a + np.arange(n) for a, n in zip(c["prior"], c["new"])] + [np.zeros(0, np.int64)])
    return lambda i: f"query of seq {seq[i // c['Hq']]} (prior {c['prior'][seq[i // c['Hq']]]}) pos {pos[i // c['Hq']]} head {i % c['Hq']}"


def decode_labels(c):
    return lambda i: f"sequence {i // c['Hq']} of length {c['lens'][i // c['Hq']]} head {i % c['Hq']}"


@functools.lru_cache(maxsize=None)
def lengths(Hkv):
    return tuple(k6.decode_lengths(decode_plan, Hkv))


@functools.lru_cache(maxsize=None)
def batch(i, rows):
    g, Hkv, P = k6.SHAPES[i]
    return k6.prefill_batch(g, Hkv, P, rows, prefill_plan)


def decode_all(cache, q, lens, msl):
    """paged_decode of single-token queries over prefixes (lens[b] tokens) of the cache's ONE physical sequence, DECODE_GROUP sequences
    per launch (so that the plan the lengths were derived from is the one in use)"""
    o = torch.empty_like(q)
    for rows in k6.decode_groups(len(lens)):
        tbl = k6.prefix_table(cache["pages"], cache["P"], [lens[b] for b in rows])
        idx = torch.tensor(rows, device=q.device)
        o[idx] = mixedgemm.paged_decode(q[idx], cache["data"], cache["param"], *(i32(a, q.device) for a in tbl), LAYER, msl)
    return o


def run_decode_case(c, dev, bound, what, grid=True, rope=False):
    """both kinds under the three bounds of decode_bounds: the exact answer, and fp8 == bf16 bit for bit; returns (caches, outputs)"""
    one, tight, loose = k6.decode_bounds()
    plans = [decode_plan(k6.DECODE_GROUP, c["Hkv"], b) for b in (one, tight, loose)]
    assert plans[0][0] == 1 and plans[1][0] > 1 and plans[2][0] > 1 and tuple(c["lengths"]) == lengths(c["Hkv"])
    q, caches, outs, worst = bf(c["q"], dev), {}, {}, 0.0
    for kind in KINDS:
        caches[kind] = fill(kind, c["K"], c["V"], [c["N"]], c["P"], dev, rope=rope)
        for msl in (one, tight, loose):
            outs[kind, msl] = decode_all(caches[kind], q, c["lens"], msl)
            worst = max(worst, expect_rows(outs[kind, msl], c["expect"], decode_labels(c), bound,
                                           f"{what} decode {kind} g={c['g']} P={c['P']} bound {msl}", grid))
    for msl in (one, tight, loose):
        assert torch.equal(outs["fp8", msl].view(torch.int16), outs["bf16", msl].view(torch.int16)), f"{what} decode bound {msl}: fp8 differs from bf16"
    print(f"kv_exact_hd64 {what} decode g={c['g']} P={c['P']}: worst error / bound {worst:.3g}")
    return caches, outs


def run_prefill_case(c, dev, bound, what, grid=True, rows=None, rope=False, split=True):
    """both kinds under a tight and a loose bound: the exact answer, and fp8 == bf16 bit for bit"""
    msl, T, B = max(c["lens"]), sum(c["new"]), len(c["new"])
    plan = prefill_plan(T, B, c["Hq"], c["Hkv"], msl)
    assert rows is None or plan[0] == rows, f"the plan must pick the {rows}-row workgroup, it reports {plan}"
    assert not split or plan[3] > 1, "must take the split path"
    q, qo, outs, worst = bf(c["q"], dev), i32(k6.indptr_of(c["new"]), dev), {}, 0.0
    for kind in KINDS:
        cache = fill(kind, c["K"], c["V"], c["lens"], c["P"], dev, rope=rope)
        for m in (msl, msl + 5000):
            outs[kind, m] = mixedgemm.paged_prefill(q, cache["data"], cache["param"], *cache["tbl"], qo, LAYER, m)
            worst = max(worst, expect_rows(outs[kind, m], c["expect"], prefill_labels(c), bound,
                                           f"{what} prefill {kind} g={c['g']} P={c['P']} rows {plan[0]} bound {m}", grid))
    for m in (msl, msl + 5000):
        assert torch.equal(outs["fp8", m].view(torch.int16), outs["bf16", m].view(torch.int16)), f"{what} prefill bound {m}: fp8 differs from bf16"
    print(f"kv_exact_hd64 {what} prefill g={c['g']} P={c['P']} rows {plan[0]}: worst error / bound {worst:.3g}")


# ---- decode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_needle_decode_and_one_token_prefill(dev, i):
    """every target of every length comes back; and a one-token prefill of the same positions returns the same V rows"""
    g, Hkv, P = k6.SHAPES[i]
    c = k6.needle_decode(g, Hkv, P, lengths(Hkv), seed=400 + i)
    assert k6.needle_decode_uncovered(c) == []
    caches, outs = run_decode_case(c, dev, k6.EXACT_BOUND, "needle")
    B, q = len(c["lens"]), bf(c["q"], dev)
    tbl = [i32(a, dev) for a in k6.prefix_table(caches["bf16"]["pages"], P, c["lens"])]
    for kind in KINDS:
        o = mixedgemm.paged_prefill(q, caches[kind]["data"], caches[kind]["param"], *tbl, i32(np.arange(B + 1), dev), LAYER, c["N"])
        expect_rows(o, c["expect"], decode_labels(c), k6.EXACT_BOUND, f"one-token prefill {kind} g={g} P={P}")
        assert np.array_equal(np.rint(8 * f64(o)), np.rint(8 * f64(outs[kind, c["N"]]))), "decode and a one-token prefill return different V rows"


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["rising", "falling"])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_ramp_decode(dev, i, sign):
    g, Hkv, P = k6.SHAPES[i]
    run_decode_case(k6.ramp_decode(g, Hkv, P, sign, lengths(Hkv)), dev, k6.EXACT_BOUND, "ramp", rope=True)


@pytest.mark.parametrize("i", range(N_SHAPES))
def test_count_decode(dev, i):
    g, Hkv, P = k6.SHAPES[i]
    c = k6.count_decode(g, Hkv, P, lengths(Hkv))
    run_decode_case(c, dev, k6.bf16_ulp(c["expect"]).reshape(-1, 64), "count", grid=False)


# ---- prefill ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [128, 64])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_needle_prefill(dev, i, rows):
    g, Hkv, P = k6.SHAPES[i]
    c = k6.needle_prefill(g, Hkv, P, *batch(i, rows), seed=300 + i, cover=6)
    assert k6.needle_prefill_uncovered(c) == []
    run_prefill_case(c, dev, k6.EXACT_BOUND, "needle", rows=rows)


@pytest.mark.parametrize("i", range(N_SHAPES))
def test_needle_prefill_every_alignment(dev, i):
    """priors 0 .. 63: the diagonal and p - 1 targets on every row of a query tile at every position within a 64-token kv tile"""
    g, Hkv, P = k6.SHAPES[i]
    c = k6.needle_prefill(g, Hkv, P, *k6.every_alignment(g), seed=350 + i)
    run_prefill_case(c, dev, k6.EXACT_BOUND, "needle, every alignment", rows=128, split=False)


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["rising", "falling"])
@pytest.mark.parametrize("rows", [128, 64])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_ramp_prefill(dev, i, rows, sign):
    g, Hkv, P = k6.SHAPES[i]
    run_prefill_case(k6.ramp_prefill(g, Hkv, P, sign, *batch(i, rows)), dev, k6.EXACT_BOUND, "ramp", rows=rows, rope=True)


@pytest.mark.parametrize("i", range(N_SHAPES))
def test_ramp_prefill_every_alignment(dev, i):
    g, Hkv, P = k6.SHAPES[(i + 1) % N_SHAPES]
    run_prefill_case(k6.ramp_prefill(g, Hkv, P, 1.0, *k6.every_alignment(g)), dev, k6.EXACT_BOUND, "ramp, every alignment", rows=128, split=False)


@pytest.mark.parametrize("rows", [128, 64])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_count_prefill(dev, i, rows):
    g, Hkv, P = k6.SHAPES[i]
    c = k6.count_prefill(g, Hkv, P, *batch(i, rows))
    run_prefill_case(c, dev, k6.bf16_ulp(c["expect"]).reshape(-1, 64), "count", grid=False, rows=rows)


# ---- fresh prompt ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["needle", "rising", "falling"])
@pytest.mark.parametrize("i", [0, 3, 5, 8])
def test_fresh_prompt(dev, i, what):
    """rope_kv_append_dense into an empty, poisoned cache, then dense_attention over what it returns, at the sequence lengths of
    test_dense_attention_hd64_gpu.py (the BQ / BK edges of the dense kernel): a wrong row of the dense kernel is named too"""
    g, Hkv, P = k6.SHAPES[i]
    new = list(t_dense.LENS)
    prior = [0] * len(new)
    assert max(new) == t_dense.LONG <= k6.MAX_LEN and {0, 1, t_dense.BK, t_dense.BQ} <= set(new)
    c = (k6.needle_prefill(g, Hkv, P, prior, new, seed=500 + i) if what == "needle" else
         k6.ramp_prefill(g, Hkv, P, 1.0 if what == "rising" else -1.0, prior, new))
    indptr, indices, last, max_pages = k6.page_table(new, P, seed=i)
    T, outs = sum(new), {}
    one = torch.ones((T, 64), dtype=torch.bfloat16, device=dev)
    for kind in KINDS:
        data, param = device_cache(kind, max_pages, Hkv, P, dev)
        q, k, v = bf(c["q"], dev), bf(c["K"], dev), bf(c["V"], dev)
        q_rot, k_seen, v_seen = mixedgemm.rope_kv_append_dense(data, param, *(i32(a, dev) for a in (indptr, indices, last)), q, k, v, one,
                                                               torch.zeros_like(one), i32(k6.indptr_of(new), dev), LAYER)
        assert torch.equal(q_rot, q) and torch.equal(k_seen, k) and torch.equal(v_seen, v), "cos 1, sin 0 over exact rows returns them"
        outs[kind] = mixedgemm.dense_attention(q_rot, k_seen, v_seen, i32(k6.indptr_of(new), dev))
        expect_rows(outs[kind], c["expect"], prefill_labels(c), k6.EXACT_BOUND, f"fresh prompt {what} {kind} g={g} P={P}")
        # and the cache it wrote answers the same through the paged kernel
        o = mixedgemm.paged_prefill(q_rot, data, param, *(i32(a, dev) for a in (indptr, indices, last)), i32(k6.indptr_of(new), dev), LAYER, max(new))
        expect_rows(o, c["expect"], prefill_labels(c), k6.EXACT_BOUND, f"fresh prompt {what} {kind} g={g} P={P}, paged")
    assert torch.equal(outs["fp8"].view(torch.int16), outs["bf16"].view(torch.int16))
