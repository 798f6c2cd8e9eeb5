"""Every claim of tests/golden/rms_sentinels.json, re-derived with the oracle alone (no GPU).

The fixture lists rows on which a wrongly ordered RMSNorm sum of squares (tests/rms_order_cases.py) changes the bytes the quantizer
produces.  Here: the seeded row stream is the LCG of tests/golden/lcg.py; every listed row regenerates to the recorded bits; under
the named wrong order the oracle's bytes differ, first at the recorded column; every (K, integer_round, wrong order) has at least
two such rows or is vacuous -- the order coincides with the oracle's at that K, shown on 4096 rows; and the control that is the
reason for all of this: on 64 random rows per K the same wrong orders change the bytes of next to none."""
import zlib

import numpy as np
import pytest

import rms_order_cases as c
from oracle import mx_oracle as o

FIX = c.load_fixture()
KS = sorted(c.SPLITS)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_fixture_covers_the_cases_of_this_module():
    assert FIX["eps"] == c.EPS and FIX["per_case"] >= 2
    assert sorted(int(k) for k in FIX["vacuous"]) == KS
    assert {s["K"] for s in FIX["sentinels"]} == set(KS)
    assert all(s["order"] in c.ORDERS for s in FIX["sentinels"])
    assert all(k < 384 or all(s > 0 for s in c.SPLITS[k]) for k in KS)            # three segments wherever K >= 384


def test_seeded_stream_is_the_golden_lcg():
    assert np.array_equal(c.lcg_words(77, 100000, 70000), c.lcg.lcg_u32(77, 170000)[100000:])
    k = 2176
    words = c.lcg.lcg_u32(k, 3 * k)[2 * k:]
    assert np.array_equal(c.seeded_row(k, 2), o.f32_to_bf16(c._bell(words)))
    x = o.bf16_to_f32(c.seeded_rows(4096, 0, 64))
    assert abs(float(x.mean())) < 0.01 and 0.98 < float(x.std()) < 1.02          # roughly N(0, 1), as the issue's rates assume
    assert np.array_equal(np.sort(c.reorder_index(k)), np.arange(k))


@pytest.mark.parametrize("k", KS)
def test_every_sentinel_detects_its_wrong_order(k):
    mine = [s for s in FIX["sentinels"] if s["K"] == k]
    numbers = sorted({s["row"] for s in mine})
    x = np.stack([c.seeded_row(k, n) for n in numbers])
    right, wrong = c.rvars(x)
    assert np.array_equal(bits(right), bits(o.rmsnorm_rvar(x, c.EPS)))
    for s in mine:
        i = numbers.index(s["row"])
        assert zlib.crc32(x[i].tobytes()) == s["crc32"], s
        bad = wrong[s["order"]][i:i + 1]
        assert bits(bad)[0] != bits(right)[i], s
        assert 0 <= s["column"] < k and c.flip_column(x[i], k, s["integer_round"], bad) == s["column"], s


@pytest.mark.parametrize("k", KS)
def test_two_sentinels_per_wrong_order_or_vacuous_by_name(k):
    vacuous = FIX["vacuous"][str(k)]
    for ir in (True, False):
        for name in c.ORDERS:
            rows = {s["row"] for s in FIX["sentinels"] if (s["K"], s["integer_round"], s["order"]) == (k, ir, name)}
            if name in vacuous:
                assert not rows
            else:
                assert len(rows) >= 2, (k, ir, name)
    assert "ulp_up" not in vacuous and "ulp_down" not in vacuous
    # vacuous: the order IS the oracle's at this K -- equal rvar bits on 4096 rows of the stream
    if vacuous:
        step = max(1, (1 << 21) // k)
        for first in range(0, 4096, step):
            right, wrong = c.rvars(c.seeded_rows(k, first, min(step, 4096 - first)), vacuous)
            for name in vacuous:
                assert np.array_equal(bits(right), bits(wrong[name])), (k, name)


@pytest.mark.parametrize("k", KS)
def test_control_random_rows_do_not_notice(k):
    """why the sentinels exist: 64 random rows per K, the same wrong orders, and the bytes of fewer than a quarter of the rows change
    (in fact of 0 to 3 of them) although rvar itself moved in up to all 64"""
    split, w, idx = c.SPLITS[k], c.norm_weight(k), c.reorder_index(k)
    x = c.seeded_rows(k, 1 << 30, 64)                       # far from every row the generator walked
    right, wrong = c.rvars(x)
    moved_any = False
    for name in c.ORDERS:
        moved = np.flatnonzero(bits(wrong[name]) != bits(right))
        moved_any |= len(moved) > 0
        if not len(moved):
            continue
        a = c.normalised_bits(x[moved], w, idx, right[moved])
        b = c.normalised_bits(x[moved], w, idx, wrong[name][moved])
        seen = moved[np.any(a != b, axis=1)]                # no element of the normalised row differs: no byte can
        for ir in (True, False):
            changed = 0
            if len(seen):
                good = o.rmsnorm_quantize(x[seen], w, c.EPS, idx, *split, integer_round=ir)
                bad = o.rmsnorm_quantize(x[seen], w, c.EPS, idx, *split, integer_round=ir, rvar=wrong[name][seen])
                gc, gs = c.codes_of(good, split)
                bc, bs = c.codes_of(bad, split)
                changed = int((np.any(gc != bc, axis=1) | np.any(gs != bs, axis=1)).sum())
            assert changed < 16, (k, name, ir, changed, len(moved))
    assert moved_any


@pytest.mark.parametrize("k", c.DECODE_KS)
def test_a_one_hot_weight_at_the_flip_column_carries_the_flip_to_an_output(k):
    """the decode tests (tests/test_rms_order_decode_gpu.py) give output feature f a weight that is one-hot at the flip column of
    sentinel f: the oracle product of the wrong-order codes then differs from the true product in that feature, in both weight modes"""
    for s in (s for s in FIX["sentinels"] if s["K"] == k):
        x = c.seeded_row(k, s["row"])
        bad = c.rvars(x, (s["order"],))[1][s["order"]]
        assert c.one_hot_output_differs(x, k, s["integer_round"], bad, s["column"]), s


def test_rvar_argument_of_the_oracle_defaults_to_rmsnorm_rvar():
    k = 384
    x = c.seeded_rows(k, 0, 5)
    w, idx = c.norm_weight(k), c.reorder_index(k)
    a = o.rmsnorm_quantize(x, w, c.EPS, idx, 128, 128, 128)
    b = o.rmsnorm_quantize(x, w, c.EPS, idx, 128, 128, 128, rvar=o.rmsnorm_rvar(x, c.EPS))
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    twice = o.rmsnorm_quantize(x, w, c.EPS, idx, 128, 128, 128, rvar=2 * o.rmsnorm_rvar(x, c.EPS))
    assert not np.array_equal(a[5], twice[5])               # the scales moved by one
