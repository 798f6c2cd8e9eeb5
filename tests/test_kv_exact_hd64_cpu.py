"""CPU proofs of what tests/test_kv_exact_hd64_gpu.py relies on (tests/kv_exact_cases_hd64.py): the 64-wide grids, codes, ramps and
counts survive both cache kinds bit for bit (tests/kv_fp8_oracle.py), the code book leaves 40 nats among 4608 tokens, the targets cover
every edge, the batches make the library's plan report the workgroup shape and the chunk edges they claim, and a plain fp64 softmax over
the built q, K, V returns the constructed answers within the stated bounds -- so the cases are proved before a kernel sees them."""
import functools

import numpy as np
import pytest

from micromix_amd import _lib, mixedgemm
import kv_exact_cases as kc
import kv_exact_cases_hd64 as k6
import kv_fp8_oracle as kf

decode_plan = mixedgemm.paged_decode_hd64_plan
prefill_plan = lambda *a: tuple(mixedgemm.paged_prefill_hd64_plan(*a))
N_SHAPES = len(k6.SHAPES)


@functools.lru_cache(maxsize=None)
def lengths(Hkv):
    return tuple(k6.decode_lengths(decode_plan, Hkv))


@functools.lru_cache(maxsize=None)
def batch(i, rows):
    g, Hkv, P = k6.SHAPES[i]
    return k6.prefill_batch(g, Hkv, P, rows, prefill_plan)


def assert_fp8_exact(x, e_want, what):
    """every row of x [.., 64] comes back from the fp8 rule bit for bit, under the exponent the module's docstring states"""
    rows = np.unique(kc.bf16_bits(x).reshape(-1, 64), axis=0)
    codes, e = kf.quantize_row(rows)
    assert np.array_equal(kf.dequantize(codes, kf.param_pair(e)), rows), f"{what}: a row changes in the fp8 cache"
    assert e_want is None or (e == e_want).all(), f"{what}: exponents {sorted(set(e.tolist()))}, expected {e_want}"


def attend(c, b0, K, V, q, pos):
    """fp64 causal attention of the queries q [n, Hq, 64] at positions pos over K, V [len, Hkv, 64]"""
    g, n = c["g"], q.shape[0]
    out = np.empty(q.shape, dtype=np.float64)
    keep = np.repeat(np.arange(K.shape[0])[None, :] <= np.asarray(pos)[:, None], g, axis=0)          # [n * g, len]
    for h in range(c["Hkv"]):                                # query heads h g .. h g + g - 1 read kv head h (repeat_kv)
        s = q[:, h * g:(h + 1) * g].reshape(n * g, 64).astype(np.float64) @ K[:, h].astype(np.float64).T * k6.SM_SCALE
        s = np.where(keep, s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        out[:, h * g:(h + 1) * g] = ((p / p.sum(-1, keepdims=True)) @ V[:, h].astype(np.float64)).reshape(n, g, 64)
    return out


def prefill_fp64(c):
    out, t0, q0 = np.zeros(c["expect"].shape), 0, 0
    for b, (a, n) in enumerate(zip(c["prior"], c["new"])):
        if n:
            out[q0:q0 + n] = attend(c, b, c["K"][t0:t0 + a + n], c["V"][t0:t0 + a + n], c["q"][q0:q0 + n], a + np.arange(n))
        t0, q0 = t0 + a + n, q0 + n
    return out


def decode_fp64(c, rows=None):
    rows = range(len(c["lens"])) if rows is None else rows
    return np.stack([attend(c, 0, c["K"][:c["lens"][b]], c["V"][:c["lens"][b]], c["q"][b:b + 1], [c["lens"][b] - 1])[0] for b in rows])


def test_the_tiles_are_the_library_s_and_the_shapes_cover_every_g_and_page_size():
    assert k6.TILE == _lib.KV_HD64["MM_KV_HD64_DECODE_TILE"] == _lib.KV_PREFILL_HD64["MM_KV_PREFILL_HD64_TILE"] == 64
    assert _lib.KV_HD64["MM_KV_HD64_DECODE_WAVES"] * k6.TILE == k6.decode_bounds()[0]
    assert sorted(s[0] for s in k6.SHAPES) == sorted(k6.G_VALUES) == sorted(kc.G_VALUES)
    assert {s[2] for s in k6.SHAPES} == set(k6.PAGE_SIZES) == {1, 3, 16, 24, 64, 100}
    assert all(g * Hkv >= 3 for g, Hkv, _ in k6.SHAPES)
    assert k6.MAX_LEN == 72 * 64 and k6.EXACT_BOUND == 2.0 ** -20 and k6.MARGIN_NATS == 40.0


def test_v_grid_is_exact_in_fp8_and_names_its_token():
    pos = np.array([0, 1, 2, 63, 64, 4095, 4096, 4607, 32767])
    v = k6.v_grid(np.arange(16)[:, None, None], pos[None, :, None], np.arange(8)[None, None, :]).reshape(-1, 64)
    assert v.min() == -1.0 and v.max() == 0.875 and np.array_equal(v * 8, np.round(v * 8))
    assert (v[:, 0] == -1.0).all() and (v[:, 1] == 0.875).all() and (v[:, 46:] == 0).all()
    assert len(np.unique(v, axis=0)) == len(v)
    assert_fp8_exact(v, -8, "v_grid")
    assert k6.v_decode(k6.v_grid(3, 4097, 2)) == "seq 3 pos 4097 head 2"
    two = k6.v_grid(0, np.array([5, 7]), 1)
    assert (two[0] != two[1]).sum() == 2 and np.abs(two[0] - two[1]).max() == 1.0
    # 1000 random rows of the grid's kind: both ends present, multiples of 1/8
    rng = np.random.default_rng(0)
    rows = rng.integers(-8, 8, (1000, 64)).astype(np.float32) / 8
    rows[:, 0], rows[:, 1] = -1.0, 0.875
    assert_fp8_exact(rng.permuted(rows, axis=1), -8, "random grid rows")
    msg = k6.describe_mismatch(k6.v_grid(0, np.array([9]), 0), k6.v_grid(0, np.array([8]), 0).astype(np.float64), lambda i: "row", 2.0 ** -20)
    assert "expects seq 0 pos 8 head 0, got seq 0 pos 9 head 0" in msg


def test_the_128_builders_return_what_they_returned():
    """kv_exact_cases.describe_mismatch gained an argument; its default is the 128 grid's decoder"""
    got, want = kc.v_grid(0, np.array([9]), 0), kc.v_grid(0, np.array([8]), 0).astype(np.float64)
    assert "expects seq 0 pos 8 head 0, got seq 0 pos 9 head 0" in kc.describe_mismatch(got, want, lambda i: "row", 2.0 ** -20)
    assert np.array_equal(k6.ramp_k(np.arange(4608)), kc.ramp_k(np.arange(4608))[:, :64]) and kc.ramp_k(5).shape == (128,)


def test_needle_margin_is_44_nats():
    """from the code book: the worst off-target correlation of the first 4608 codes of 64 dims, per kv head"""
    assert k6.worst_correlation(0) == 42 and k6.worst_correlation(1) == 40
    for h in range(4):
        assert k6.worst_correlation(h) <= 44                            # (64 - 44) * 16 / 8 = 40
    assert k6.needle_margin_nats(2) == 44.0 and k6.needle_margin_nats(4) >= k6.MARGIN_NATS
    assert np.exp(-k6.MARGIN_NATS) * k6.MAX_LEN < 2e-14                  # all other tokens together
    assert (64 - 42) * 8.0 * k6.SM_SCALE == 22.0                         # 8 u, the 128 suite's query, would leave 22 nats
    assert_fp8_exact(k6.code(0, k6.MAX_LEN).astype(np.float32), -8, "needle K")
    # and on the built case: the score lead of a target over every other token
    c = k6.needle_decode(5, 2, 100, [k6.MAX_LEN], seed=1)
    for b in (0, len(c["lens"]) - 1):
        for hq in range(c["Hq"]):
            s = c["K"][:, hq // c["g"]].astype(np.float64) @ c["q"][b, hq].astype(np.float64) * k6.SM_SCALE
            t = c["targets"][b, hq]
            assert s[t] == 128.0 and s[t] - np.delete(s, t).max() >= 44.0


def test_ramp_and_count_rows_are_exact():
    t = np.arange(k6.MAX_LEN)
    assert_fp8_exact(k6.ramp_k(t), -4, "ramp K")
    assert_fp8_exact(k6.count_v(t), -7, "count V")
    q = k6.ramp_q()
    assert np.array_equal(kc.to_bf16(q), q) and q.shape == (64,)
    s = (k6.ramp_k(t) * q).sum(-1, dtype=np.float32)
    assert np.array_equal(s, (512 * t).astype(np.float32)) and 512 * k6.MAX_LEN < 2 ** 24 and 512 * k6.SM_SCALE == 64.0
    assert np.array_equal(k6.count_expect(np.array([0, 63, 64, 200])), np.stack([k6.count_expect(p, np.ones(300, bool)) for p in (0, 63, 64, 200)]))
    assert not k6.count_expect(np.array(-1)).any()
    # one lost token among 4608 moves its dimension by 3.3 ulps: outside the 1-ulp bound, and further outside for every shorter length
    want = k6.count_expect(k6.MAX_LEN - 1)
    assert (1.875 / k6.MAX_LEN) / k6.bf16_ulp(want)[0] >= 3.0


def test_decode_lengths_stand_on_the_plan_s_chunk_edges():
    for Hkv in (2, 4):
        ls, (one, tight, loose) = lengths(Hkv), k6.decode_bounds()
        assert decode_plan(k6.DECODE_GROUP, Hkv, one)[0] == 1
        assert set(k6.BASE_LENGTHS) | {k6.MAX_LEN} <= set(ls) and max(ls) == k6.MAX_LEN
        for bound in (tight, loose):
            nc, cl = decode_plan(k6.DECODE_GROUP, Hkv, bound)
            assert nc > 1 and cl % 256 == 0
            assert all(c * cl + s in ls for c in range(1, nc) for s in (-1, 0, 1) if c * cl + s <= k6.MAX_LEN)
        assert decode_plan(k6.DECODE_GROUP, Hkv, tight)[1] != decode_plan(k6.DECODE_GROUP, Hkv, loose)[1]
    assert all(len(grp) == k6.DECODE_GROUP for grp in k6.decode_groups(13)) and sorted({b for grp in k6.decode_groups(13) for b in grp}) == list(range(13))


@pytest.mark.parametrize("i", range(N_SHAPES))
def test_needle_decode_covers_every_edge_and_fp64_returns_the_targets(i):
    g, Hkv, P = k6.SHAPES[i]
    c = k6.needle_decode(g, Hkv, P, lengths(Hkv), seed=400 + i)
    assert k6.needle_decode_uncovered(c) == [] and set(c["lens"]) == set(c["lengths"]) and len(c["lens"]) >= k6.DECODE_GROUP
    req = k6.decode_required(k6.MAX_LEN, k6.MAX_LEN, P)
    assert {0, k6.MAX_LEN - 1, k6.MAX_LEN - 2} <= set(req) and all(e in req for m in range(P, k6.MAX_LEN, P) for e in (m - 1, m))
    assert all(e in k6.decode_required(1000, k6.MAX_LEN, P) for m in range(64, 1000, 64) for e in (m - 1, m))
    # the check itself bites: hide one edge
    broken = dict(c, targets=np.where(c["targets"] == 63, 0, c["targets"]))
    assert any(e == 63 for _, e in k6.needle_decode_uncovered(broken))
    rows = np.random.default_rng(i).choice(len(c["lens"]), 40, replace=False)
    assert np.abs(decode_fp64(c, rows) - c["expect"][rows]).max() <= k6.EXACT_BOUND


@pytest.mark.parametrize("rows", [128, 64])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_prefill_batches_make_the_plan_report_their_shape_and_edges(i, rows):
    g, Hkv, P = k6.SHAPES[i]
    prior, new = batch(i, rows)
    bq = rows // g
    assert new[:6] == [0, 1, bq - 1, bq, bq + 1, 2 * bq + 3] and new[6] > 2 * bq
    plan = prefill_plan(sum(new), len(new), g * Hkv, Hkv, k6.MAX_LEN)
    assert plan[0] == rows and plan[1] == bq and plan[3] > 1 and plan[4] % 64 == 0
    assert max(a + n for a, n in zip(prior, new)) == k6.MAX_LEN
    for c in range(1, plan[3]):
        assert {c * plan[4] - 1, c * plan[4]} <= set(prior), "a chunk edge of the plan without a sequence that starts on it"
    if rows == 64:
        assert {(a, 1) for a in range(64)} <= set(zip(prior, new))
    a_prior, a_new = k6.every_alignment(g)
    assert a_prior == list(range(64)) and prefill_plan(sum(a_new), 64, g * Hkv, Hkv, max(a_prior) + a_new[0])[0] == 128


@pytest.mark.parametrize("rows", [128, 64])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_needle_prefill_covers_every_edge_and_fp64_returns_the_targets(i, rows):
    g, Hkv, P = k6.SHAPES[i]
    c = k6.needle_prefill(g, Hkv, P, *batch(i, rows), seed=300 + i, cover=6)
    assert k6.needle_prefill_uncovered(c) == []
    edge = next(e for e in k6.edge_positions(299, P) if 0 < e < 250)
    assert edge in k6.needle_prefill_uncovered(dict(c, targets=np.where(c["targets"] == edge, 0, c["targets"])))
    if i in (0, 4, 8):
        assert np.abs(prefill_fp64(c) - c["expect"]).max() <= k6.EXACT_BOUND
        assert_fp8_exact(c["K"], -8, "needle prefill K")
        assert_fp8_exact(c["V"], -8, "needle prefill V")


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_ramp_fp64_returns_own_position_or_position_0(sign):
    g, Hkv, P = k6.SHAPES[1]
    c = k6.ramp_prefill(g, Hkv, P, sign, *batch(1, 64))
    assert np.abs(prefill_fp64(c) - c["expect"]).max() <= k6.EXACT_BOUND
    assert_fp8_exact(c["K"], -4, "ramp K")
    assert_fp8_exact(c["V"], -8, "ramp V")
    d = k6.ramp_decode(g, Hkv, P, sign, lengths(Hkv))
    assert np.abs(decode_fp64(d) - d["expect"]).max() <= k6.EXACT_BOUND
    a = k6.ramp_prefill(7, 2, 1, sign, *k6.every_alignment(7))
    assert np.abs(prefill_fp64(a) - a["expect"]).max() <= k6.EXACT_BOUND


def test_count_fp64_returns_the_mean():
    g, Hkv, P = k6.SHAPES[2]
    c = k6.count_prefill(g, Hkv, P, *batch(2, 64))
    assert np.abs(prefill_fp64(c) - c["expect"]).max() <= 1e-13
    assert_fp8_exact(c["V"], None, "count V")
    d = k6.count_decode(g, Hkv, P, lengths(Hkv))
    assert np.abs(decode_fp64(d) - d["expect"]).max() <= 1e-13


def test_poisoned_images_and_page_0():
    d8, p8 = k6.empty_host_cache("fp8", 2, 3, 2, 3)
    d16, _ = k6.empty_host_cache("bf16", 2, 3, 2, 3)
    assert d8.shape == d16.shape == (2, 3, 2, 2, 3, 64) and (d8 == 0x7F).all() and np.isnan(p8.astype(np.float32)).all()
    assert (kf.dequantize(d8, p8) == 0x7FC0).all() and (d16 == 0x7FC0).all()
    for P in k6.PAGE_SIZES:
        assert 0 not in k6.page_table([40, 3, 4608], P, 5)[1]
